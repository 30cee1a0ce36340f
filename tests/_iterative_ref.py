"""Host restatement of matrix-free exact GP regression (IterativeGPRegressionLogPdf) on a DENSE float64 covariance matrix from
tests/_gram_ref.py: the same preconditioned CG recurrence (one column at a time), pivoted Cholesky, stochastic Lanczos quadrature and
gradient estimator, with the unit-normal draws `eps` (N + r, T) as an argument.  Plain module, numpy only.

    Khat = K + noise I        P = L_r L_r^T + noise I        Z = sqrt(noise) eps[:N] + L_r eps[N:]
    value = -1/2 sum_p y_p^T alpha_p - 1/2 P logdet - 1/2 N P log 2 pi,   logdet = log|P| + 1/T sum_i (z_i^T P^-1 z_i) e_1^T log(T_i) e_1
    G = 1/2 sum_p alpha_p alpha_p^T - P / (2 T) sum_i u_i w_i^T,          d value / d theta = sum_ij G_ij dKhat_ij / d theta
"""
import numpy as np

import _gram_ref as GR


def pivoted_cholesky(K, rank):
    N = K.shape[0]
    d = np.diag(K).copy()
    floor = 1e-12 * d.max()
    L = np.zeros((N, min(rank, N)))
    for m in range(L.shape[1]):
        piv = int(np.argmax(d))
        if d[piv] <= floor:
            return L[:, :m]
        col = (K[piv] - L[:, :m] @ L[piv, :m]) / np.sqrt(d[piv])
        L[:, m] = col
        d = np.maximum(d - col * col, 0.0)
        d[piv] = 0.0
    return L


def precond(L, noise, N):
    """(solve, logdet) of P = L L^T + noise I by the Woodbury identity"""
    r = L.shape[1]
    if r == 0:
        return (lambda v: v / noise), N * np.log(noise)
    M = L.T @ L + noise * np.eye(r)
    C = np.linalg.cholesky(M)
    Minv = np.linalg.inv(M)
    return (lambda v: (v - L @ (Minv @ (L.T @ v))) / noise), (N - r) * np.log(noise) + 2.0 * np.log(np.diag(C)).sum()


def pcg(A, b, solve, tol, max_iter):
    """one column; (x, alphas, betas) of the iterations that ran: stops once ||r|| <= tol ||b||"""
    x, r = np.zeros_like(b), b.copy()
    z = solve(r)
    p, rz = z.copy(), r @ z
    bn = np.linalg.norm(b)
    al, be = [], []
    for _ in range(max_iter):
        if np.linalg.norm(r) <= tol * bn:
            break
        Ap = A @ p
        a = rz / (p @ Ap)
        x, r = x + a * p, r - a * Ap
        z = solve(r)
        rz_new = r @ z
        bt = rz_new / rz
        p, rz = z + bt * p, rz_new
        al.append(a)
        be.append(bt)
    return x, np.array(al), np.array(be), np.linalg.norm(r) / bn


def quadrature(al, be):
    """e_1^T log(T) e_1 of the Lanczos tridiagonal of a column's CG coefficients"""
    k = len(al)
    if k == 0:
        return 0.0
    T = np.zeros((k, k))
    for i in range(k):
        T[i, i] = 1.0 / al[i] + (be[i - 1] / al[i - 1] if i else 0.0)
        if i + 1 < k:
            T[i, i + 1] = T[i + 1, i] = np.sqrt(max(be[i], 0.0)) / al[i]
    lam, Q = np.linalg.eigh(T)
    return float((Q[0] ** 2 * np.log(lam)).sum())


def logpdf(kind, X, Y, noise, ls, var, eps, rank, tol, max_iter):
    """X (N, Q), Y (N, P), noise and var floats, ls (Q,) or (1,), eps (N + r, T) with r the rank the pivoted Cholesky reaches.  A dict: value,
    logdet, dls, dvar, dnoise, dY, alpha, iterations, residual (the worst final relative residual), and `scale`, the absolute sums of the
    terms of dls / dvar / dnoise / value that a bar is relative to."""
    N, P = Y.shape
    K = GR.gram_ref(kind, X[None], None, np.asarray(ls, float)[None], np.array([[var]]))[0]
    Khat = K + noise * np.eye(N)
    L = pivoted_cholesky(K, rank)
    r = L.shape[1]
    assert eps.shape[0] == N + r, (eps.shape, N, r)
    T = eps.shape[1]
    solve, logdetP = precond(L, noise, N)
    Z = np.sqrt(noise) * eps[:N] + (L @ eps[N:] if r else 0.0)
    W = solve(Z)
    alpha, U, quad, its, res = np.zeros((N, P)), np.zeros((N, T)), [], [], 0.0
    for p in range(P):
        alpha[:, p], al, be, rr = pcg(Khat, Y[:, p], solve, tol, max_iter)
        its.append(len(al))
        res = max(res, rr)
    for i in range(T):
        U[:, i], al, be, rr = pcg(Khat, Z[:, i], solve, tol, max_iter)
        quad.append((Z[:, i] @ W[:, i]) * quadrature(al, be))
        its.append(len(al))
        res = max(res, rr)
    logdet = logdetP + float(np.mean(quad))
    value = -0.5 * (Y * alpha).sum() - 0.5 * P * logdet - 0.5 * N * P * np.log(2 * np.pi)
    Ga, Gt = 0.5 * alpha @ alpha.T, -0.5 * P / T * U @ W.T
    g, s = GR.gram_bwd_ref(kind, X[None], None, np.asarray(ls, float)[None], np.array([[var]]), (Ga + Gt)[None])
    sa = GR.gram_bwd_ref(kind, X[None], None, np.asarray(ls, float)[None], np.array([[var]]), Ga[None])[0]
    st = GR.gram_bwd_ref(kind, X[None], None, np.asarray(ls, float)[None], np.array([[var]]), Gt[None])[0]
    scale = dict(dls=np.abs(sa['dls'][0]) + np.abs(st['dls'][0]), dvar=abs(sa['dvar'][0, 0]) + abs(st['dvar'][0, 0]),
                 dnoise=abs(np.trace(Ga)) + abs(np.trace(Gt)), value=0.5 * abs((Y * alpha).sum()) + 0.5 * P * abs(logdet) + 0.5 * N * P * np.log(2 * np.pi),
                 dY=np.abs(alpha).max())
    return dict(value=value, logdet=logdet, dls=g['dls'][0], dvar=g['dvar'][0, 0], dnoise=np.trace(Ga + Gt), dY=-alpha, alpha=alpha,
                iterations=its, residual=res, scale=scale, rank=r)


def exact_probes(N, r=0):
    """the N + r draws sqrt(N + r) e_i: their outer products average to the identity, so Hutchinson's trace is exact"""
    return np.sqrt(N + r) * np.eye(N + r)
