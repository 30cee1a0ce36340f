"""CPU restatements for the per-sample log-pdf and score-function tests (tests/test_gpu_logpdf_per_sample.py, test_gpu_score_function.py):
plain torch / numpy, float64 unless a dtype is asked for, no code shared with the package.

Tolerances are the project's (tests/test_gpu_univariate.py header).  float64: 1e-9 relative to the summed magnitudes of the addends a result
is reduced from; the magnitudes used here are the |values| of the reduced elements (sum_i |scale log p[s,i]| for out[s], sum |w scale
d log p| over what a gradient is summed over, plus the pre-filled value) -- a lower bound of the sum over a formula's individual terms, so
never wider than the rule allows.  float32: rtol 1e-4, atol 1e-5, after the same formula in float32 on the CPU met that bar."""
import itertools
import math

import numpy as np
import torch

KINDS = ('normal', 'gamma', 'gamma_mv', 'beta', 'laplace', 'uniform', 'bernoulli')
F64_BAR, F32_RTOL, F32_ATOL = 1e-9, 1e-4, 1e-5


def tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def rnd(a, dtype):
    """inputs exactly representable in the dtype under test, as float64: kernel and restatement see the same numbers"""
    return np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64)


def logp(kind, x, a, b):
    """log p(x | a, b) elementwise, the reference's formulas (normal.py:52-70, gamma.py:45-59, :127-159, beta.py:46-68, laplace.py:37-55,
    uniform.py:38-62, bernoulli.py:62-78) in torch, any dtype"""
    if kind == 'normal':
        return -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(b) - (x - a) ** 2 / (2 * b)
    if kind == 'gamma_mv':
        kind, a, b = 'gamma', a * a / b, a / b
    if kind == 'gamma':
        return (a - 1) * torch.log(x) - b * x - torch.lgamma(a) + a * torch.log(b)
    if kind == 'beta':
        return (a - 1) * torch.log(x) + (b - 1) * torch.log1p(-x) - torch.lgamma(a) - torch.lgamma(b) + torch.lgamma(a + b)
    if kind == 'laplace':
        return -torch.log(2 * b) - torch.abs(x - a) / b
    if kind == 'bernoulli':
        return x * torch.log(a) + (1 - x) * torch.log1p(-a)
    lp = -torch.log(b - a) + torch.zeros_like(x)
    return torch.where((a <= x) & (x < b), lp, torch.full_like(lp, -float('inf')))


def partials(kind, x, a, b, dtype=torch.float64):
    """log p (S, n) and d log p / d(x, a, b), each (S, n), float64 numpy; computed by CPU autograd in `dtype`.  x (S, n); a, b broadcastable
    against it.  Elements outside the Uniform's support carry no gradient; Bernoulli's second slot has none."""
    S, n = x.shape
    leaves = [torch.as_tensor(np.broadcast_to(np.asarray(t), (S, n)).copy(), dtype=dtype).requires_grad_(True) for t in (x, a, b)]
    lp = logp(kind, *leaves)
    tot = torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp)).sum()
    g = torch.autograd.grad(tot, leaves, allow_unused=True)
    g = [np.zeros((S, n)) if t is None else t.double().numpy() for t in g]
    if kind == 'bernoulli':
        g[2] = np.zeros((S, n))
    return [lp.detach().double().numpy()] + g


LAYOUTS = ('1', 'n', 'sn')          # a single element; per element; per sample and element


def param(values, layout, S, n):
    """an (S, n) array of parameter values cut down to the layout's own array"""
    return {'1': values[0, :1], 'n': values[0], 'sn': values}[layout].copy()


def fold(g, layout):
    """the (S, n) per-element contributions to a parameter's gradient, summed over what the layout shares"""
    return {'1': g.sum().reshape(1), 'n': g.sum(axis=0), 'sn': g}[layout]


def make_inputs(kind, S, n, la, lb, dtype, seed=0):
    """x (S, n) and the two parameters in their layouts, float64 values representable in `dtype`; chosen so that the sums over the elements
    of a sample do not cancel (log p < 0 throughout: moderate shape parameters, x below the mode of no density)"""
    r = np.random.RandomState(seed + 7 * n + S + 31 * LAYOUTS.index(la) + 97 * LAYOUTS.index(lb))
    U = lambda lo, hi: r.uniform(lo, hi, (S, n))
    if kind == 'normal':
        A, B = r.randn(S, n), U(0.5, 2.0)
    elif kind == 'gamma':
        A, B = U(0.5, 6.5), U(0.5, 2.0)
    elif kind == 'gamma_mv':
        A, B = U(0.5, 3.0), U(0.5, 2.0)
    elif kind == 'beta':
        A, B = U(2.0, 6.5), U(0.5, 6.5)
    elif kind == 'laplace':
        A, B = r.randn(S, n), U(0.5, 2.0)
    elif kind == 'uniform':
        A, B = U(-1.0, -0.5), U(0.5, 2.0)
    else:
        A = U(0.1, 0.9)
        B = A
    a, b = rnd(param(A, la, S, n), dtype), rnd(param(B, lb, S, n), dtype)
    if kind == 'bernoulli':
        b = a = rnd(param(A, la, S, n), dtype)
        lb = la
    Ab = np.broadcast_to(a.reshape((-1, n) if a.size > 1 else (1, 1)), (S, n))
    Bb = np.broadcast_to(b.reshape((-1, n) if b.size > 1 else (1, 1)), (S, n))
    if kind == 'normal':
        x = Ab + np.sqrt(Bb) * 3.0 * r.randn(S, n)
    elif kind == 'gamma':
        x = (Ab / Bb) * U(2.0, 4.0)                     # in the right tail: every term of the sum is well below zero
    elif kind == 'gamma_mv':
        x = Ab * U(2.0, 4.0)
    elif kind == 'beta':
        x = U(0.001, 0.01)                              # near zero: the term (a - 1) log x dominates every element
    elif kind == 'laplace':
        x = Ab + Bb * (2 * r.randn(S, n) + 1)
        x[0, 0] = Ab[0, 0]                              # x == location: sign(0) = 0
    elif kind == 'uniform':
        x = U(-0.45, 0.45)
        x[0, 0] = Ab[0, 0]                              # x == low: inside
        if S >= 2:
            x[S - 1, n - 1] = Bb[S - 1, n - 1]          # x == high: outside the support, in the last sample only
    else:
        x = (r.rand(S, n) < 0.5).astype(np.float64)
    return rnd(x, dtype), a, b


def weights(S, dtype, seed=0):
    """mixed signs, one exact zero (S >= 2)"""
    base = np.array([-1.5, 0.0, 0.7, 2.0, -0.3])
    w = base[:S] if S <= 5 else np.random.RandomState(seed + S).randn(S)
    if S > 5:
        w[3] = 0.0
    return rnd(w, dtype)


def expected(kind, x, a, b, la, lb, w, scale, dtype=torch.float64):
    """out (S,) = scale * sum_i log p, the gradients dx (S, n), da, db (in their layouts) of sum_s w[s] out[s], and the magnitudes of each"""
    lp, gx, ga, gb = partials(kind, x, a, b, dtype)
    ws = (np.asarray(w) * scale)[:, None]
    with np.errstate(invalid='ignore'):
        out = scale * lp.sum(axis=1)
    vals = [out, ws * gx, fold(ws * ga, la), fold(ws * gb, lb)]
    mags = [np.abs(scale * np.where(np.isfinite(lp), lp, 0.0)).sum(axis=1), np.abs(ws * gx), fold(np.abs(ws * ga), la), fold(np.abs(ws * gb), lb)]
    return vals, mags


def assert_close(what, got, want, mag, dtype, prefill=0.0):
    """got against prefill + want under the dtype's bar; infinities must agree exactly"""
    got, want, mag = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(mag, dtype=np.float64)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), (what, got[inf], want[inf])
    got, want, mag = got[~inf], want[~inf] + prefill, mag[~inf] + abs(prefill)
    err = np.abs(got - want)
    bar = F64_BAR * mag if dtype == 'float64' else F32_ATOL + F32_RTOL * np.abs(want)
    bad = ~(err <= bar)
    assert not bad.any(), (what, dtype, float(err[bad].max()), float(bar[bad].min()), int(bad.sum()))


def assert_float32_formula_meets_the_bar(what, vals32, vals64):
    """the float32 precondition: the same formula in float32 on the CPU is within rtol 1e-4, atol 1e-5 of float64 on these inputs"""
    for k, (v32, v64) in enumerate(zip(vals32, vals64)):
        fin = np.isfinite(v64)
        err = np.abs(v32[fin] - v64[fin])
        bar = F32_ATOL + F32_RTOL * np.abs(v64[fin])
        assert (err <= bar).all(), ('the float32 formula on the CPU misses the bar on these inputs', what, k, float((err - bar).max()))


# ---- the estimators ------------------------------------------------------------------------------------------------------------------

def loo(f):
    """b_s = (sum_t f_t - f_s) / (S - 1)"""
    return (f.sum() - f) / (f.shape[0] - 1)


def score_gradient(q_of, leaves, f, baseline):
    """(1/S) sum_s (f_s - b_s) grad log q(z_s): q_of() -> (S,) log q(z_s) as a function of `leaves`; f (S,) detached weights"""
    w = f - (loo(f) if baseline == 'loo' else 0.0)
    return torch.autograd.grad((q_of() * w.detach()).mean(), leaves, allow_unused=True)


def softplus(x):
    return torch.nn.functional.softplus(x)


def lognormal(x, mean, var):
    return -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(var) - (x - mean) ** 2 / (2 * var)


def bernoulli_configs(K):
    return torch.tensor(list(itertools.product([0.0, 1.0], repeat=K)), dtype=torch.float64)
