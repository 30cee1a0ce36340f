"""A float64 torch restatement on the CPU of the per-row contraction of the Psi2 terms and of the prediction of the Bayesian GP-LVM at
uncertain test inputs x* ~ N(mu*, diag(s*)), built on tests/_psi_ref.py: the reference of tests/test_psi_predict_host.py,
tests/test_gpu_psi_quad.py and tests/test_gpu_gplvm_uncertain_predict.py.  It shares no code with the library."""
import torch

import _psi_ref as R


def quad(mu, s, Z, ls, var, A):
    """R[n, j] = sum_{m,m'} A[j, m, m'] psi2n[n, m, m']: (N, J) from A (J, M, M)"""
    return torch.einsum('jab,nab->nj', A, R.psi2n(mu, s, Z, ls, var))


def predict_uncertain(Xt_mean, Xt_var, mu, s, Z, ls, var, noise, Y, jitter=0.0, noise_free=True):
    """mean (Nt, P) and variance (Nt, P) of the prediction under x*_n ~ N(Xt_mean[n], diag(Xt_var[n])), from the factors of the bound:
    wv = L^-T LA^-T c / noise, C = L^-T (I - LA^-T LA^-1) L^-1, mean = Psi1*^T wv, var_p = variance + sum (wv_p wv_p^T - C) psi2n* - mean_p^2"""
    M = Z.shape[0]
    eye = torch.eye(M, dtype=torch.float64)
    L, Li, B, LA, c = R.factors(mu, s, Z, ls, var, noise, Y, jitter)
    wv = Li.T @ torch.linalg.solve_triangular(LA.T, c, upper=True) / noise[0]
    LAi = torch.linalg.solve_triangular(LA, eye, upper=False)
    C = Li.T @ (eye - LAi.T @ LAi) @ Li
    mean = R.psi1(Xt_mean, Xt_var, Z, ls, var).T @ wv
    A = wv.T[:, :, None] * wv.T[:, None, :] - C[None]
    v = var[0] + quad(Xt_mean, Xt_var, Z, ls, var, A) - mean * mean
    return mean, v if noise_free else v + noise[0]
