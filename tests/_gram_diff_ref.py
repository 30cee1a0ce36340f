"""Float64 restatement of the difference-form covariances (mxf_gram_diff) in torch: the three formulae (components()); gradients come from
torch's automatic differentiation.  Beside them the file holds the scales the error bars need: majorant(), a linearisation of the same formulae
whose derivatives are the slopes' envelopes (sines and cosines at 1), checked against closed forms in tests/test_gram_diff_host.py, and
amplification().  Every function takes ONE sample: X (N, Q), X2 (N2, Q) and per kind
  'periodic': variance (1,), lengthscale (Q|1,), period (Q|1,)      'rq': variance (1,), lengthscale (Q|1,), alpha (1,)
  'sm': weights (A,), means (A, Q), scales (A, Q).
components() returns the summed terms (C, N, N2) -- C = 1, or the A mixture components -- so that a caller has both an output and the sum of
the absolute values of its terms, which is what an error bar of a sum is proportional to."""
import math

import torch
from torch.func import jvp

KINDS = ('periodic', 'rq', 'sm')
NAMES = {'periodic': ('variance', 'lengthscale', 'period'), 'rq': ('variance', 'lengthscale', 'alpha'), 'sm': ('weights', 'means', 'scales')}


def components(kind, X, X2, p0, p1, p2):
    tau = X[:, None, :] - X2[None, :, :]                                      # (N, N2, Q)
    if kind == 'periodic':
        return (p0 * torch.exp(-0.5 * (torch.sin(math.pi * tau / p2) ** 2 / p1 ** 2).sum(-1)))[None]
    if kind == 'rq':
        r2 = (tau ** 2 / p1 ** 2).sum(-1)
        return (p0 * (1 + r2 / (2 * p2)) ** (-p2))[None]
    if kind == 'sm':
        t = tau[None]                                                         # (1, N, N2, Q) against (A, 1, 1, Q)
        mu, s = p1[:, None, None, :], p2[:, None, None, :]
        return p0[:, None, None] * torch.exp(-2 * math.pi ** 2 * (t ** 2 * s ** 2).sum(-1)) * torch.cos(2 * math.pi * t * mu).prod(-1)
    raise ValueError(kind)


def majorant(kind, X, X2, p0, p1, p2, at):
    """A function of the same operands whose derivatives at the point `at` (plain tensors X, X2, p0, p1, p2) are, in absolute value, the
    derivatives of components() with every sine and cosine at 1 and every contribution of the same sign: what the error of ONE pair's term
    of a gradient is proportional to (a phase rounded by eps |phase| moves a sine or cosine by that much absolutely, however close to zero it
    is; with the term itself as the scale, single-pair gradients next to such a zero measured 185 to 927 roundoffs on the device in float32
    and float64 alike).  It is linear in the phases around `at` and works on |tau|.  RQ has no trigonometric factor: its own terms."""
    if kind == 'rq':
        return components(kind, X, X2, p0, p1, p2)
    X0, Z0, q0, q1, q2 = at
    a, a0 = (X[:, None, :] - X2[None, :, :]).abs(), (X0[:, None, :] - Z0[None, :, :]).abs()
    if kind == 'periodic':          # k0 (p0 / q0) (1 - sum_d [(phi_d - phi0_d) / (2 l0_d^2) + (l_d^-2 - l0_d^-2) / 2]): slopes k pi / (2 l^2 p), k / l^3, ...
        k0 = components(kind, X0, Z0, q0, q1, q2)[0]
        lin = 0.5 / q1 ** 2 * (math.pi * a / p2 - math.pi * a0 / q2) + 0.5 * (p1 ** -2 - q1 ** -2) + 0 * a
        return (k0 * (p0 / q0) * (1 - lin.sum(-1)))[None]
    a, a0 = a[None], a0[None]       # sm: w exp(-E) (1 - sum_d (phi_d - phi0_d))
    mu, s, mu0 = p1[:, None, None, :], p2[:, None, None, :], q1[:, None, None, :]
    return p0[:, None, None] * torch.exp(-2 * math.pi ** 2 * (a ** 2 * s ** 2).sum(-1)) * (1 - (2 * math.pi * (a * mu - a0 * mu0)).sum(-1))


def gram(kind, X, X2, p0, p1, p2):
    """(K, T): the Gram (N, N2) and the sum of the absolute values of each element's terms: |K| for the one-component kinds; for the spectral
    mixture the components with their cosines at 1 -- a phase rounded by eps |phase| moves a cosine by that much absolutely, however close
    to zero the cosine is, so one element's error is proportional to the envelope of its terms (measured on the device with the terms
    themselves as T: ratios of 2e4 in float32 AND float64 alike, at the elements next to a cosine's zero)"""
    Z = X if X2 is None else X2
    c = components(kind, X, Z, p0, p1, p2)
    return c.sum(0), (components(kind, X, Z, p0, torch.zeros_like(p1), p2) if kind == 'sm' else c).abs().sum(0)


def kdiag(kind, p0):
    return p0.sum()


def amplification(kind, X, X2, p0, p1, p2):
    """1 + the largest phase or exponent argument of the case: what one rounding of an operand is multiplied by on its way into K"""
    tau = (X[:, None, :] - (X if X2 is None else X2)[None, :, :]).abs()
    if kind == 'periodic':
        return 1 + float((math.pi * tau / p2 / p1 ** 2).max())
    if kind == 'sm':
        return 1 + float((2 * math.pi * tau[None] * p1[:, None, None, :].abs()).max())
    r2 = (tau ** 2 / p1 ** 2).sum(-1)
    return 1 + float((p2 * torch.log1p(r2 / (2 * p2))).max())


def grads(kind, X, X2, p0, p1, p2, dK, need=('X', 'X2', 'p0', 'p1', 'p2')):
    """{name: (gradient, T)} of sum(dK * K) for the operands in `need`; T has the gradient's shape and holds the sum over the pairs (and
    components) of |dK_ij| times the envelope of |dK_ij/dtheta| (majorant()).  X2 None: both roles of X flow into 'X'.  One forward-mode pass per operand element (per coordinate
    for X and X2: row i of K alone depends on row i of X)."""
    square = X2 is None
    Z = X if square else X2
    ops = {'X': X, 'X2': Z, 'p0': p0, 'p1': p1, 'p2': p2}
    order = ('X', 'X2', 'p0', 'p1', 'p2')
    f = lambda *a: components(kind, *a)
    prim = tuple(ops[n] for n in order)
    fm = lambda *a: majorant(kind, *a, at=prim)
    out = {}

    def tangent(name, t):
        return tuple(t if n == name else torch.zeros_like(ops[n]) for n in order)

    for name in order:
        if name == 'X2' and square:
            continue
        if name not in need:
            continue
        op = ops[name]
        g, T = torch.zeros_like(op), torch.zeros_like(op)
        if name in ('X', 'X2'):
            roles = (('X', -1), ('X2', -2)) if square else ((name, -1 if name == 'X' else -2),)
            for role, red in roles:
                for d in range(op.shape[-1]):
                    e = torch.zeros_like(op)
                    e[:, d] = 1
                    J = jvp(f, prim, tangent(role, e))[1] * dK           # (C, N, N2)
                    g[:, d] += J.sum(0).sum(red)
                    T[:, d] += (jvp(fm, prim, tangent(role, e))[1] * dK).abs().sum(0).sum(red)
        else:
            gf, Tf, e = g.view(-1), T.view(-1), torch.zeros_like(op)
            for i in range(op.numel()):
                e.view(-1)[i] = 1
                J = jvp(f, prim, tangent(name, e))[1] * dK
                gf[i], Tf[i] = J.sum(), (jvp(fm, prim, tangent(name, e))[1] * dK).abs().sum()
                e.view(-1)[i] = 0
        out[name] = (g, T)
    return out
