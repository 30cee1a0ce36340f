"""Float64 reference of the non-Gaussian SVGP (torch on the CPU, SciPy for the special functions), written from the formulas of the
bound -- not from the kernel:

  g(f) = log p(y | f), its derivatives and mu(f) = E[y | f] of the three likelihood kinds;
  E_{N(f; m, v)}[g] by Gauss-Hermite quadrature, d/dm by autograd through that sum and d/dv in the Price form E[g''] / 2;
  the bound  c sum E[g] - KL(q(u) || p(u))  with the marginals of q(f), by autograd through torch.linalg.
"""
import math

import numpy as np
import torch
from scipy import special

KINDS = ('bernoulli_logit', 'bernoulli_probit', 'poisson_exp')
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def rule(nq):
    x, w = np.polynomial.hermite.hermgauss(nq)
    return torch.as_tensor(x), torch.as_tensor(w / math.sqrt(math.pi))


# ---- pointwise, NumPy / SciPy (float64 arrays) ----------------------------------------------------------------------------------------
def mills_np(z):
    """(lambda, lambda + z) with lambda(z) = phi(z) / Phi(z): exp(log phi - log_ndtr) for z >= -5; below, the continued fraction of the Mills
    ratio, lambda + z = 1 / (t + 2 / (t + 3 / ...)) with t = -z, to depth 120 (within 2e-15 at depth 24 from t = 5 on), where lambda + z is all
    cancellation"""
    z = np.asarray(z, dtype=np.float64)
    lam = np.exp(-0.5 * z * z - LOG_SQRT_2PI - special.log_ndtr(z))
    c = lam + z
    t = -np.minimum(z, -5.0)
    cf = np.zeros_like(t)
    for k in range(120, 0, -1):
        cf = k / (t + cf)
    far = z < -5.0
    return np.where(far, t + cf, lam), np.where(far, cf, c)


def g_np(kind, y, f):
    """(g, g', g'') at float64 arrays y, f"""
    y, f = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(f, dtype=np.float64))
    if kind == 'poisson_exp':
        e = np.exp(f)
        return y * f - e - special.gammaln(y + 1.0), y - e, -e
    sg = 2.0 * y - 1.0
    z = sg * f
    if kind == 'bernoulli_logit':
        return special.log_expit(z), sg * special.expit(-z), -special.expit(z) * special.expit(-z)
    lam, c = mills_np(z)
    return special.log_ndtr(z), sg * lam, -lam * c


def mu_np(kind, f):
    f = np.asarray(f, dtype=np.float64)
    return {'bernoulli_logit': special.expit, 'bernoulli_probit': special.ndtr, 'poisson_exp': np.exp}[kind](f)


# ---- torch (float64, differentiable in f) ---------------------------------------------------------------------------------------------
def g_torch(kind, y, f):
    if kind == 'poisson_exp':
        return y * f - torch.exp(f) - torch.lgamma(y + 1.0)
    z = (2.0 * y - 1.0) * f
    return torch.nn.functional.logsigmoid(z) if kind == 'bernoulli_logit' else torch.special.log_ndtr(z)


def nodes_at(m, v, x):
    """f_k = m + sqrt(2 max(v, 0)) x_k: m (..., N, P), v (..., N) -> (..., N, P, K)"""
    return m.unsqueeze(-1) + torch.sqrt(2.0 * torch.clamp(v, min=0.0))[..., None, None] * x


def expect_elem(kind, y, m, v, nq=20):
    """sum_k w_k g(f_k), shaped like m; differentiable in m (and, through the sqrt, in v > 0)"""
    x, w = rule(nq)
    return (g_torch(kind, y.unsqueeze(-1), nodes_at(m, v, x)) * w).sum(-1)


def expect_grads(kind, y, m, v, nq=20):
    """(dm, dv) of sum_k w_k g(f_k) per element: dm (..., N, P) = sum_k w_k g'(f_k), dv (..., N) = 1/2 sum_p sum_k w_k g''(f_k) (Price)"""
    x, w = rule(nq)
    f = nodes_at(m, v, x).detach()
    _, g1, g2 = g_np(kind, y.unsqueeze(-1).numpy(), f.numpy())
    return (torch.as_tensor(g1) * w).sum(-1), 0.5 * (torch.as_tensor(g2) * w).sum(-1).sum(-1)


def moments(kind, m, v, nq=20):
    x, w = rule(nq)
    u = torch.as_tensor(mu_np(kind, nodes_at(m, v, x).numpy()))
    return (u * w).sum(-1), (u * u * w).sum(-1)


def predictive(kind, m, v, nq=20):
    e1, e2 = moments(kind, m, v, nq)
    return e1, (e1 + e2 - e1 * e1 if kind == 'poisson_exp' else e1 - e1 * e1)


class _ExpectSum(torch.autograd.Function):
    """sum over (N, P) of expect_elem per sample; backward: d/dm by autograd through the forward sum, d/dv in the Price form"""

    @staticmethod
    def forward(ctx, kind, nq, y, m, v):
        ctx.kind, ctx.nq = kind, nq
        ctx.save_for_backward(y, m, v)
        return expect_elem(kind, y, m, v, nq).sum((-1, -2))

    @staticmethod
    def backward(ctx, g):
        y, m, v = ctx.saved_tensors
        with torch.enable_grad():
            mm = m.detach().clone().requires_grad_(True)
            dm, = torch.autograd.grad(expect_elem(ctx.kind, y, mm, v.detach(), ctx.nq).sum(), mm)
        _, dv = expect_grads(ctx.kind, y, m.detach(), v.detach(), ctx.nq)
        return None, None, None, dm * g[..., None, None], dv * g[..., None]


def expect_sum(kind, y, m, v, nq=20):
    y, m, v = torch.broadcast_tensors(y, m, v.unsqueeze(-1))
    return _ExpectSum.apply(kind, nq, y, m, v[..., 0])


# ---- kernels and the bound ------------------------------------------------------------------------------------------------------------
def rbf(X, X2, ls, var):
    d = (X.unsqueeze(-2) - X2.unsqueeze(-3)) / ls
    return var * torch.exp(-0.5 * (d * d).sum(-1))


def linear(X, X2, variances):
    return (X * variances) @ X2.transpose(-1, -2)


def make_kernel(which, p):
    """(K(X, X2), Kdiag(X)) of 'rbf' (p: ls (Q,), var (1,)) or 'rbf+linear' (p: + variances (Q|1,))"""
    if which == 'rbf':
        return (lambda A, B: rbf(A, B, p['ls'], p['var'])), (lambda A: p['var'] * torch.ones(A.shape[:-1], dtype=A.dtype))
    return (lambda A, B: rbf(A, B, p['ls'], p['var']) + linear(A, B, p['variances'])), \
        (lambda A: p['var'] * torch.ones(A.shape[:-1], dtype=A.dtype) + (A * A * p['variances']).sum(-1))


def marginals(K, Kdiag, X, Z, qm, qW, qd, jitter=0., mean=None):
    """m (N, P), v (N,) of q(f) at X, and (L, L^-1 mu, L^-1 S L^-T) for the KL term"""
    M = Z.shape[0]
    L = torch.linalg.cholesky(K(Z, Z) + jitter * torch.eye(M, dtype=Z.dtype))
    A = torch.linalg.solve_triangular(L, K(Z, X), upper=False)
    Lmu = torch.linalg.solve_triangular(L, qm, upper=False)
    S = qW @ qW.T + torch.diag(qd)
    B = torch.linalg.solve_triangular(L, torch.linalg.solve_triangular(L, S, upper=False).T, upper=False)
    m = A.T @ Lmu
    if mean is not None:
        m = m + mean
    v = Kdiag(X) - (A * A).sum(0) + ((B @ A) * A).sum(0)
    return m, v, (L, Lmu, B, S)


def svgp_bound(kind, K, Kdiag, X, Y, Z, qm, qW, qd, jitter=0., scaling=1.0, mean=None, nq=20):
    """c sum_{n,p} E[g] - KL(q(u) || p(u)), one sample (no leading axis)"""
    m, v, (L, Lmu, B, S) = marginals(K, Kdiag, X, Z, qm, qW, qd, jitter, mean)
    M, P = qm.shape
    kl = 0.5 * (P * torch.trace(B) + (Lmu * Lmu).sum() - P * M + P * (2.0 * torch.log(torch.diagonal(L)).sum() - torch.logdet(S)))
    return scaling * expect_sum(kind, Y, m, v, nq) - kl
