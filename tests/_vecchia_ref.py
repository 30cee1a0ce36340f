"""float64 CPU restatement of the nearest-neighbour (Vecchia) GP kernels (csrc/knn.hip, csrc/vecchia.hip), written from the formulas and
sharing no code with the package:
    knn(X, C, k, causal)                          brute force, (d2, j) order, -1 / +inf padding
    terms(kind, X, Y, nbr, ls, var, noise)        the l_i by a batched gather and torch.linalg.cholesky on padded tiles; differentiable
    cond(kind, Xt, X, Y, nbr, ls, var, noise)     the conditional used for prediction (latent mean and variance)
    logpdf(...)                                   value, terms, gradients by autograd, the per-row summands of every gradient, and the
                                                  largest cond_1(A_i) of the case
With c the neighbours of row i (|c| <= k, entries -1 are empty slots), A = K(X_c, X_c) + noise I, kappa = K(X_c, x_i), a = k(x_i, x_i) + noise:
    b = A^-1 kappa, alpha = A^-1 Y_c, s = a - kappa^T b, r = y_i - kappa^T alpha, l_i = -P/2 log 2 pi - P/2 log s - |r|^2 / (2 s).
The covariance functions carry the package's clip rule: the Matern kinds evaluate r = sqrt(max(r^2, 1e-14)), also on the diagonal, and the
clip carries no slope; the predictor's k(x*, x*) is the variance itself."""
import math

import numpy as np
import torch

KINDS = ('rbf', 'matern12', 'matern32', 'matern52')


def knn(X, C, k, causal):
    X = np.asarray(X, dtype=np.float64)
    C = X if C is None else np.asarray(C, dtype=np.float64)
    D = np.zeros((X.shape[0], C.shape[0]))
    for q in range(X.shape[1]):
        D += (X[:, q:q + 1] - C[None, :, q]) ** 2
    idx = np.full((X.shape[0], k), -1, dtype=np.int32)
    d2 = np.full((X.shape[0], k), np.inf)
    for n in range(X.shape[0]):
        m = n if causal else C.shape[0]
        order = np.lexsort((np.arange(m), D[n, :m]))[:k]
        idx[n, :len(order)] = order
        d2[n, :len(order)] = D[n, order]
    return idx, d2


def cov(kind, r2, var):
    """the covariance from the scaled squared distance r2 (any shape)"""
    if kind == 'rbf':
        return var * torch.exp(-0.5 * r2)
    r = torch.sqrt(torch.clamp(r2, min=1e-14))
    if kind == 'matern12':
        return var * torch.exp(-r)
    if kind == 'matern32':
        return var * (1 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
    return var * (1 + math.sqrt(5.0) * r + 5.0 / 3.0 * r2) * torch.exp(-math.sqrt(5.0) * r)


def _tiles(kind, Xo, X, Y, nbr, ls, var, noise):
    """A (R, k, k) padded with the unit matrix on empty slots, kappa (R, k) and Y_c (R, k, P) with zeros there"""
    nbr = torch.as_tensor(np.asarray(nbr), dtype=torch.int64)
    valid = nbr >= 0
    j = nbr.clamp(min=0)
    Xc, Yc = X[j] / ls, Y[j] * valid[..., None]
    k = nbr.shape[1]
    eye = torch.eye(k, dtype=torch.float64)
    K = cov(kind, ((Xc[:, :, None, :] - Xc[:, None, :, :]) ** 2).sum(-1), var) + noise * eye
    both = valid[:, :, None] & valid[:, None, :]
    A = torch.where(both, K, eye.expand_as(K))
    kap = cov(kind, ((Xc - (Xo / ls)[:, None, :]) ** 2).sum(-1), var) * valid
    return A, kap, Yc


def _solve(A, kap, Yc):
    L = torch.linalg.cholesky(A)
    return torch.cholesky_solve(kap[..., None], L)[..., 0], torch.cholesky_solve(Yc, L)


def terms(kind, X, Y, nbr, ls, var, noise, parts=False):
    X, Y, ls, var, noise = [torch.as_tensor(t, dtype=torch.float64) for t in (X, Y, ls, var, noise)]
    A, kap, Yc = _tiles(kind, X, X, Y, nbr, ls, var, noise)
    b, alpha = _solve(A, kap, Yc)
    a = cov(kind, torch.zeros((), dtype=torch.float64), var) + noise
    s = a - (kap * b).sum(-1)
    r = Y - (kap[..., None] * alpha).sum(1)
    P = Y.shape[1]
    t = -0.5 * P * math.log(2 * math.pi) - 0.5 * P * torch.log(s) - (r * r).sum(-1) / (2 * s)
    if parts:       # the magnitudes of a term's three summands, and the conditioning of its tile
        mag = 0.5 * P * math.log(2 * math.pi) + 0.5 * P * torch.log(s).abs() + (r * r).sum(-1) / (2 * s)
        return t, mag.detach(), float(torch.linalg.cond(A.detach(), p=1).max())
    return t


def cond(kind, Xt, X, Y, nbr, ls, var, noise):
    Xt, X, Y, ls, var, noise = [torch.as_tensor(t, dtype=torch.float64) for t in (Xt, X, Y, ls, var, noise)]
    A, kap, Yc = _tiles(kind, Xt, X, Y, nbr, ls, var, noise)
    b, alpha = _solve(A, kap, Yc)
    return ((kap[..., None] * alpha).sum(1).numpy(), (var - (kap * b).sum(-1)).numpy(), float(torch.linalg.cond(A, p=1).max()))


def logpdf(kind, X, Y, nbr, ls, var, noise):
    """dict: value, terms, dls, dvar, dnoise, dY; scale[...]: for the terms the summed magnitudes of a term's summands, for the value and each
    gradient its own magnitude plus that of its largest per-row summand; cond_max"""
    X = torch.as_tensor(X, dtype=torch.float64)
    leaves = [torch.as_tensor(np.atleast_1d(t), dtype=torch.float64).clone().requires_grad_(True) for t in (ls, var, noise, Y)]
    ls_, var_, noise_, Y_ = leaves
    t, mag, cmax = terms(kind, X, Y_, nbr, ls_, var_[0], noise_[0], parts=True)
    # the per-row summands of a gradient: the backward pass is linear in the cotangent v, so d (v . grad) / dv has them
    v = torch.ones_like(t).requires_grad_(True)
    g = torch.autograd.grad(t, leaves, grad_outputs=v, create_graph=True)
    out = dict(value=float(t.detach().sum()), terms=t.detach().numpy(), cond_max=cmax)
    scale = dict(terms=mag.numpy(), value=abs(float(t.detach().sum())) + float(mag.max()))
    for name, gi in zip(('dls', 'dvar', 'dnoise'), g[:3]):
        rows = torch.stack([torch.autograd.grad(c, v, retain_graph=True)[0] for c in gi.reshape(-1)])
        out[name] = gi.detach().numpy().copy()
        scale[name] = np.abs(out[name]) + rows.abs().max(1)[0].numpy()
    out['dY'] = g[3].detach().numpy().copy()
    scale['dY'] = np.abs(out['dY']) + np.abs(out['dY']).max()        # an element's summands are rows of the same scatter
    out['dvar'], out['dnoise'] = float(out['dvar'][0]), float(out['dnoise'][0])
    scale['dvar'], scale['dnoise'] = float(scale['dvar'][0]), float(scale['dnoise'][0])
    out['scale'] = scale
    return out
