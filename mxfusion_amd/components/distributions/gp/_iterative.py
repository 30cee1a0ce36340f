"""The iterative solver of matrix-free exact GP regression (Gardner et al. 2018, "GPyTorch: blackbox matrix-matrix Gaussian process inference";
Wang et al. 2019, "Exact Gaussian processes on a million data points"): batched preconditioned conjugate gradients, the pivoted-Cholesky
preconditioner and stochastic Lanczos quadrature.  Plain torch on the operands' device -- vectors of length N, never an N x N matrix; the
one N^2 cost, the product with the covariance matrix, is the caller's `matvec` (StationaryKernel.matvec: mxf_kmv).  The small dense pieces
(a rank x rank inverse, the probes' tridiagonals) are factorised on the host in float64.

No sample axis here: a column block is (N, C)."""
import math

import torch


class Preconditioner(object):
    """P = L L^T + sigma2 I with L (N, r) from pivoted_cholesky; r = 0: P = sigma2 I.  solve() is the Woodbury identity
    P^-1 v = (v - L (sigma2 I + L^T L)^-1 L^T v) / sigma2, logdet = (N - r) log sigma2 + log|sigma2 I + L^T L|."""

    def __init__(self, L, sigma2, N):
        self.L, self.sigma2, self.N = L, float(sigma2), int(N)
        self.rank = 0 if L is None else int(L.shape[1])
        if self.rank:
            M = (L.t() @ L).double().cpu() + self.sigma2 * torch.eye(self.rank, dtype=torch.float64)
            C = torch.linalg.cholesky(M)
            self._Minv = torch.cholesky_inverse(C).to(device=L.device, dtype=L.dtype)
            self.logdet = (self.N - self.rank) * math.log(self.sigma2) + 2.0 * float(torch.log(torch.diagonal(C)).sum())
        else:
            self.logdet = self.N * math.log(self.sigma2)

    def solve(self, V):
        if not self.rank:
            return V / self.sigma2
        return (V - self.L @ (self._Minv @ (self.L.t() @ V))) / self.sigma2

    def sample(self, eps):
        """z = sigma eps[:N] + L eps[N:] ~ N(0, P) for eps (N + r, T) of unit normals: the draw contract of the probes."""
        z = math.sqrt(self.sigma2) * eps[:self.N]
        return z + self.L @ eps[self.N:] if self.rank else z


def pivoted_cholesky(row, diag, rank, return_pivots=False):
    """L (N, r), r <= rank, of the greedy pivoted Cholesky of a positive semi-definite matrix: `row(i)` is its row at the 0-d index tensor i,
    (N,), and `diag` its diagonal (N,).  Stops early at a pivot below 1e-12 of the largest diagonal entry; rank 0 gives None.  The pivot
    stays on the device: the one host read per column is the stopping test.  With return_pivots, (L, pivots): the r pivot rows in the order
    they were taken, an int64 tensor on the device (the rows that greedily maximise the conditional variance)."""
    N = int(diag.shape[0])
    rank = min(int(rank), N)
    if rank <= 0:
        return (None, torch.zeros(0, dtype=torch.int64, device=diag.device)) if return_pivots else None
    d = diag.clone()
    floor = 1e-12 * float(d.max())
    L = torch.zeros((N, rank), dtype=diag.dtype, device=diag.device)
    pivots = []
    done = rank
    for m in range(rank):
        piv = torch.argmax(d)
        dp = d[piv]
        if float(dp) <= floor:
            done = m
            break
        col = (row(piv) - L[:, :m] @ L[piv, :m]) / torch.sqrt(dp)
        L[:, m] = col
        d = (d - col * col).clamp_min(0.0)
        d[piv] = 0.0
        pivots.append(piv)
    if done < rank:
        L = L[:, :done].contiguous() if done else None
    if return_pivots:
        return L, (torch.stack(pivots) if pivots else torch.zeros(0, dtype=torch.int64, device=diag.device))
    return L


def pcg(matvec, B, precond=None, tol=1e-8, max_iter=1000, check_every=10):
    """Solves A X = B for the columns of B (N, C) by preconditioned conjugate gradients, all columns in one `matvec(V) = A V` per iteration.
    A column stops changing once ||r|| <= tol ||b|| (its coefficients are frozen at 0 on the device); the host reads one flag per
    `check_every` iterations.  Returns (X, iterations (C,), alpha (K, C), beta (K, C)): the CG coefficients of every column, of which the
    first iterations[c] are meaningful and give the column's Lanczos tridiagonal (lanczos_tridiagonals)."""
    solve = (lambda V: V) if precond is None else precond.solve
    X = torch.zeros_like(B)
    R = B.clone()
    Z = solve(R)
    P = Z.clone()
    rz = (R * Z).sum(0)
    bnorm = B.norm(dim=0).clamp_min(torch.finfo(B.dtype).tiny)
    active = R.norm(dim=0) > tol * bnorm
    iters = torch.zeros(B.shape[1], dtype=torch.int64, device=B.device)
    alphas, betas = [], []
    zero, one = torch.zeros_like(rz), torch.ones_like(rz)
    for k in range(int(max_iter)):
        if k % check_every == 0 and not bool(active.any()):
            break
        AP = matvec(P)
        pAp = (P * AP).sum(0)
        alpha = torch.where(active, rz / torch.where(active, pAp, one), zero)
        X = X + alpha * P
        R = R - alpha * AP
        Z = solve(R)
        rz_new = (R * Z).sum(0)
        beta = torch.where(active, rz_new / torch.where(active, rz, one), zero)
        P = torch.where(active, Z + beta * P, P)
        rz = torch.where(active, rz_new, rz)
        iters = iters + active.to(torch.int64)
        alphas.append(alpha)
        betas.append(beta)
        active = active & (R.norm(dim=0) > tol * bnorm)
    if not alphas:
        alphas, betas = [zero], [zero]
    return X, iters, torch.stack(alphas), torch.stack(betas)


def lanczos_tridiagonals(alpha, beta, iters):
    """(C, K, K) float64 on the host: column c's Lanczos tridiagonal of the preconditioned operator from its CG coefficients,
    T[k, k] = 1 / alpha_k + beta_{k-1} / alpha_{k-1}, T[k, k+1] = sqrt(beta_k) / alpha_k, of order iters[c]; the rest of the K x K block is
    the identity, which adds nothing to a quadrature of the logarithm."""
    a, b, it = alpha.double().cpu(), beta.double().cpu(), iters.cpu()
    K, C = a.shape
    k = torch.arange(K).unsqueeze(1)
    on = k < it.unsqueeze(0)                        # (K, C): iteration k of column c ran
    safe = torch.where(on, a, torch.ones_like(a))
    d = 1.0 / safe
    d[1:] = d[1:] + torch.where(on[1:], b[:-1] / safe[:-1], torch.zeros_like(d[1:]))
    d = torch.where(on, d, torch.ones_like(d))
    e = torch.zeros_like(d)
    e[:-1] = torch.where(on[1:], torch.sqrt(b[:-1].clamp_min(0.0)) / safe[:-1], torch.zeros_like(d[:-1]))
    T = torch.diag_embed(d.t())
    if K > 1:
        T = T + torch.diag_embed(e[:-1].t(), offset=1) + torch.diag_embed(e[:-1].t(), offset=-1)
    return T


def slq_logdet(alpha, beta, iters, rz0, precond_logdet):
    """log|A| ~ log|P| + 1/T sum_i ||P^-1/2 z_i||^2 e_1^T log(T_i) e_1 over the T probe columns z_i ~ N(0, P) of a pcg() run: stochastic
    Lanczos quadrature of tr log(P^-1/2 A P^-1/2).  rz0 (T,) = z_i^T P^-1 z_i.  A float."""
    T = lanczos_tridiagonals(alpha, beta, iters)
    lam, Q = torch.linalg.eigh(T)
    quad = (Q[:, 0, :] ** 2 * torch.log(lam.clamp_min(1e-300))).sum(1)
    return float(precond_logdet) + float((rz0.double().cpu() * quad).mean())
