"""float64 CPU restatement of what mxfusion_amd/util/inducing.py and the nearest-centre kernel compute, written from the formulas and sharing
no code with the library (numpy only):
    nearest(X, C)                 idx[n] = the smallest m that minimises sum_q (X[n,q] - C[m,q])^2, d2[n] that minimum
    lloyd_step(X, C, idx)         the mean of the rows assigned to each centre (C[m] where none is), and the counts
    kmeanspp_rows(X, u)           D^2 sampling from given uniforms
    greedy_variance(K, M)         the rows that greedily maximise the conditional variance, from explicit conditional variances"""
import numpy as np


def lattice():
    """(X (49, 3), C (7, 3)) of small integers: every squared distance, and every float64 sum of them, is exact in float32 and float64.
    C[2] duplicates C[1] and C[5] duplicates C[0]; rows such as (1, 0, .) are equidistant from distinct centres."""
    g = np.arange(-3, 4)
    a, b = np.meshgrid(g, g, indexing='ij')
    X = np.stack([a.ravel(), b.ravel(), (a.ravel() + b.ravel()) % 2], 1).astype(np.float64)
    C = np.array([[0, 0, 0], [2, 0, 0], [2, 0, 0], [0, 2, 0], [-2, -2, 0], [0, 0, 0], [3, 3, 0]], dtype=np.float64)
    return X, C


def nearest(X, C):
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    D = np.zeros((X.shape[0], C.shape[0]))
    for q in range(X.shape[1]):
        D += (X[:, q:q + 1] - C[None, :, q]) ** 2
    idx = np.argmin(D, axis=1)              # numpy returns the first of equal minima: the smallest index
    return idx, D[np.arange(X.shape[0]), idx]


def lloyd_step(X, C, idx):
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    counts = np.bincount(idx, minlength=C.shape[0])
    C_new = C.copy()
    for m in range(C.shape[0]):
        if counts[m]:
            C_new[m] = X[idx == m].sum(0) / counts[m]
    return C_new, counts


def kmeanspp_rows(X, u):
    """row floor(u_0 N); then the first row whose float64 cumulative sum of d2 exceeds u_k total, clamped to N - 1; d2 is the squared distance
    to the nearest row chosen so far, exactly 0 at the chosen rows.  Raises where fewer distinct rows exist than uniforms."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    rows = [min(int(np.floor(u[0] * N)), N - 1)]
    d2 = ((X - X[rows[0]]) ** 2).sum(1)
    for k in range(1, len(u)):
        d2[rows] = 0.0
        cs = np.cumsum(d2)
        if cs[-1] == 0.0:
            raise ValueError('only %d distinct rows' % k)
        r = min(int(np.searchsorted(cs, u[k] * cs[-1], side='right')), N - 1)
        rows.append(r)
        d2 = np.minimum(d2, ((X - X[r]) ** 2).sum(1))
    return np.array(rows)


def conditional_variances(K, chosen):
    """diag(K) - diag(K[:, S] K[S, S]^-1 K[S, :]) for the rows S chosen so far"""
    if not chosen:
        return np.diag(K).copy()
    S = np.array(chosen)
    return np.diag(K) - np.einsum('ns,sn->n', K[:, S], np.linalg.solve(K[np.ix_(S, S)], K[S, :]))


def greedy_variance(K, M):
    """(rows, gaps): the M rows taken, and at every step (best - second best) / best of the conditional variances over the rows not yet taken.
    Among exactly equal maxima the smallest index is taken (numpy's argmax, and torch's): under a stationary kernel the first step is such a
    tie of N identical prior variances, gap 0."""
    K = np.asarray(K, dtype=np.float64)
    chosen, gaps = [], []
    for _ in range(M):
        v = conditional_variances(K, chosen)
        v[chosen] = -np.inf
        best = int(np.argmax(v))
        gaps.append((v[best] - np.delete(v, best).max()) / v[best])
        chosen.append(best)
    return np.array(chosen), np.array(gaps)
