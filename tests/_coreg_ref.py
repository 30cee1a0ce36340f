"""Float64 torch restatement of the intrinsic coregionalisation model (host reference of mxf_gram_icm / mxf_gram_icm_bwd and of the
Coregionalize kernel): plain module, no fixtures.

    K[s, i, j] = gram(X, X2)[s, i, j] * B[s|0, idx[i], idx2[j]],        B = W W^T + diag(kappa)

The Gram is the difference form of tests/_gram_ref.py (d = (x - z) / l first, r2 = sum d^2 after; the Matern kinds use sqrt(max(r2, CLIP))
and keep the un-clipped r2 in Matern52's 5/3 r2 term), restated in torch so that autograd gives the gradients; tests/test_gram_icm_host.py
ties it to _gram_ref.gram_ref.  Every operand carries the sample axis first (extent 1: shared)."""
import math

import numpy as np
import torch

import _gram_ref as G

KINDS = G.KINDS
t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def gram(kind, X, X2, ls, var):
    """(S, N, N2) from X (S|1, N, Q), X2 (S|1, N2, Q) or None, ls (S|1, Q|1), var (S|1, 1)"""
    Z = X if X2 is None else X2
    d = (X[..., :, None, :] - Z[..., None, :, :]) / ls[..., None, None, :]
    r2 = (d * d).sum(-1)
    v = var[..., None]
    if kind == 'rbf':
        return v * torch.exp(-0.5 * r2)
    r = torch.sqrt(torch.clamp(r2, min=G.CLIP))
    if kind == 'matern12':
        return v * torch.exp(-r)
    if kind == 'matern32':
        return v * (1 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
    if kind == 'matern52':
        return v * (1 + math.sqrt(5.0) * r + 5.0 / 3.0 * r2) * torch.exp(-math.sqrt(5.0) * r)
    raise ValueError(kind)


def coreg_matrix(kappa, W=None):
    """B (S|1, T, T) from kappa (S|1, T) and W (S|1, T, R) or None"""
    B = torch.diag_embed(kappa)
    return B if W is None else B + W @ W.transpose(-1, -2)


def gather(B, idx, idx2=None):
    """B[..., idx[:, None], idx2[None, :]] for integer index vectors (numpy or torch)"""
    i = torch.as_tensor(np.asarray(idx)).long()
    j = i if idx2 is None else torch.as_tensor(np.asarray(idx2)).long()
    return B[..., i[:, None], j[None, :]]


def icm(kind, X, X2, idx, idx2, ls, var, B, diag_add=None, jitter=0.0):
    K = gram(kind, X, X2, ls, var) * gather(B, idx, None if X2 is None else idx2)
    if X2 is None and (diag_add is not None or jitter):
        eye = torch.eye(X.shape[-2], dtype=K.dtype)
        K = K + eye * ((0.0 if diag_add is None else diag_add[..., None]) + jitter)
    return K


def icm_grads(kind, X, X2, idx, idx2, ls, var, B, dK):
    """(K, {name: gradient}) by autograd for the cotangent dK; names X, X2 (absent when square), ls, var, B; shapes of the primals (a
    shared operand's gradient is summed over the samples).  Matern12 with one input dimension takes the closed form of
    _gram_ref.gram_bwd_ref on the effective cotangent dK * B[idx][:, idx2] (and dB from its forward value) in extended precision, as
    test_gram_bwd_vs_autograd does: the slope -k / 2r of coincident and near-coincident points is refereed there."""
    names = ['X'] + ([] if X2 is None else ['X2']) + ['ls', 'var', 'B']
    prim = dict(X=X, X2=X2, ls=ls, var=var, B=B)
    if kind == 'matern12' and X.shape[-1] == 1:
        Bg = gather(B, idx, None if X2 is None else idx2).expand(dK.shape[0], -1, -1)
        n = lambda t: None if t is None else t.numpy()
        g, _ = G.gram_bwd_ref(kind, n(X), n(X2), n(ls), n(var), (dK * Bg).numpy(), dtype=G.HI)
        Kst = torch.as_tensor(G.gram_ref(kind, n(X), n(X2), n(ls), n(var), dtype=G.HI, S=dK.shape[0]).astype(np.float64))
        i = torch.as_tensor(np.asarray(idx)).long()
        j = i if X2 is None else torch.as_tensor(np.asarray(idx2)).long()
        T = B.shape[-1]
        dB = torch.zeros(dK.shape[0], T * T, dtype=torch.float64)
        dB.index_add_(1, (i[:, None] * T + j[None, :]).reshape(-1), (dK * Kst).reshape(dK.shape[0], -1))
        dB = dB.reshape(-1, T, T)
        if B.shape[0] == 1:
            dB = dB.sum(0, keepdim=True)
        out = {k: torch.as_tensor(g['d' + k].astype(np.float64)) for k in names if k != 'B'}
        out['B'] = dB
        return Kst * Bg, out
    leaves = {k: prim[k].clone().requires_grad_(True) for k in names}
    K = icm(kind, leaves['X'], leaves.get('X2'), idx, idx2, leaves['ls'], leaves['var'], leaves['B'])
    K = K.expand(dK.shape[0], -1, -1)
    grads = torch.autograd.grad((K * dK).sum(), [leaves[k] for k in names])
    return K.detach(), dict(zip(names, grads))


def make_case(seed, N, N2, Q, S, T, ard, f32=False, rank=2):
    """Operands of one call as float64 torch tensors: inputs uniform(-2, 2) with the sample axis (X2 shared by the samples), lengthscales in
    [0.8, 1.8] and a variance in [0.5, 1.5] (shared), B (S, T, T) from random W and kappa in [0.5, 1.5], random unsorted indices, dK standard
    normal.  N2 None: square.  f32: every value is rounded to float32 first."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(-2, 2, (S, N, Q))
    X2 = None if N2 is None else rng.uniform(-2, 2, (1, N2, Q))
    ls = rng.uniform(0.8, 1.8, (1, Q if ard else 1))
    var = rng.uniform(0.5, 1.5, (1, 1))
    W, kappa = rng.randn(S, T, rank), rng.uniform(0.5, 1.5, (S, T))
    B = coreg_matrix(t64(kappa), t64(W)).numpy()
    idx = rng.randint(0, T, N).astype(np.int32)
    idx2 = None if N2 is None else rng.randint(0, T, N2).astype(np.int32)
    dK = rng.randn(S, N, N if N2 is None else N2)
    r = (lambda a: None if a is None else t64(np.asarray(a, np.float32))) if f32 else (lambda a: None if a is None else t64(a))
    return dict(X=r(X), X2=r(X2), idx=idx, idx2=idx2, ls=r(ls), var=r(var), B=r(B), dK=r(dK))


def gp_logpdf(K, Y):
    """log N(Y; 0, K) summed over the columns of Y (N, P), K (N, N) with the noise already on its diagonal"""
    L = torch.linalg.cholesky(K)
    A = torch.cholesky_solve(Y, L)
    N, P = Y.shape
    return -0.5 * (Y * A).sum() - P * torch.log(torch.diagonal(L)).sum() - 0.5 * N * P * math.log(2 * math.pi)


def gp_predict(K, Ks, kss_diag, Y):
    """posterior mean (Nt, P) and latent variance (Nt,) at test points: K (N, N) with noise, Ks (N, Nt), kss_diag (Nt,)"""
    L = torch.linalg.cholesky(K)
    mean = Ks.T @ torch.cholesky_solve(Y, L)
    V = torch.linalg.solve_triangular(L, Ks, upper=False)
    return mean, kss_diag - (V * V).sum(0)
