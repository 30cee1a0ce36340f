"""A float64 torch restatement on the CPU of the RBF psi statistics, the collapsed bound of the Bayesian GP-LVM (Titsias & Lawrence 2010), its
KL term and its prediction: the reference of tests/test_psi_host.py, tests/test_gpu_psi.py and tests/test_gpu_bayesian_gplvm.py.  Autograd on
it gives every reference gradient.  Written from the formulas, term by term over the (N, M, M) intermediate; it shares no code with the
library.  mu, s (N, Q), Z (M, Q), ls (Q,) or (1,), var (1,); a leading sample axis is the caller's loop."""
import math

import torch


def _l2(ls, Q):
    return (ls * ls).expand(Q)


def rbf(X, X2, ls, var):
    l2 = _l2(ls, X.shape[-1])
    d = X[:, None, :] - X2[None, :, :]
    return var * torch.exp(-0.5 * (d * d / l2).sum(-1))


def psi0(mu, var):
    return mu.shape[0] * var[0]


def psi1(mu, s, Z, ls, var):
    """(M, N)"""
    l2 = _l2(ls, mu.shape[-1])
    c = torch.prod((1.0 + s / l2) ** -0.5, -1)
    d = mu[None, :, :] - Z[:, None, :]
    return var * c[None, :] * torch.exp(-0.5 * (d * d / (s + l2)[None]).sum(-1))


def psi2n(mu, s, Z, ls, var):
    """(N, M, M)"""
    l2 = _l2(ls, mu.shape[-1])
    c = torch.prod((1.0 + 2.0 * s / l2) ** -0.5, -1)
    dz = Z[:, None, :] - Z[None, :, :]
    zbar = 0.5 * (Z[:, None, :] + Z[None, :, :])
    e = mu[:, None, None, :] - zbar[None]
    ex = -(dz * dz / (4.0 * l2)).sum(-1)[None] - (e * e / (2.0 * s + l2)[:, None, None, :]).sum(-1)
    return var * var * c[:, None, None] * torch.exp(ex)


def psi2(mu, s, Z, ls, var):
    return psi2n(mu, s, Z, ls, var).sum(0)


def kl_standard_normal(mu, s):
    """KL(N(mu, diag s) || N(0, I))"""
    return 0.5 * (s + mu * mu - 1.0 - torch.log(s)).sum()


def factors(mu, s, Z, ls, var, noise, Y, jitter=0.0):
    M = Z.shape[0]
    eye = torch.eye(M, dtype=torch.float64)
    L = torch.linalg.cholesky(rbf(Z, Z, ls, var) + jitter * eye)
    Li = torch.linalg.solve_triangular(L, eye, upper=False)
    B = Li @ psi2(mu, s, Z, ls, var) @ Li.T
    LA = torch.linalg.cholesky(eye + B / noise)
    c = torch.linalg.solve_triangular(LA, Li @ (psi1(mu, s, Z, ls, var) @ Y), upper=False)
    return L, Li, B, LA, c


def bound(mu, s, Z, ls, var, noise, Y, jitter=0.0, latent_prior=False):
    """F of the issue; noise (1,), Y (N, P)"""
    P = Y.shape[1]
    L, Li, B, LA, c = factors(mu, s, Z, ls, var, noise, Y, jitter)
    F = -P * torch.log(torch.diagonal(LA)).sum() - 0.5 * (Y * Y / noise + math.log(2 * math.pi) + torch.log(noise)).sum()
    F = F + (c * c).sum() / (2.0 * noise[0] ** 2) - P * psi0(mu, var) / (2.0 * noise[0]) + P * torch.trace(B) / (2.0 * noise[0])
    if latent_prior:
        F = F - kl_standard_normal(mu, s)
    return F


def predict(Xt, mu, s, Z, ls, var, noise, Y, jitter=0.0):
    """noise-free mean (Nt, P) and variance (Nt,) at deterministic test inputs"""
    L, Li, B, LA, c = factors(mu, s, Z, ls, var, noise, Y, jitter)
    wv = Li.T @ torch.linalg.solve_triangular(LA.T, c, upper=True) / noise[0]
    Kxt = rbf(Z, Xt, ls, var)
    A1 = Li @ Kxt
    A2 = torch.linalg.solve_triangular(LA, A1, upper=False)
    return Kxt.T @ wv, var[0] - (A1 * A1).sum(0) + (A2 * A2).sum(0)
