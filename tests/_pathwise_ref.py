"""Float64 restatement on the CPU of pathwise GP posterior sampling (Wilson et al. 2020), written from the formulas; it shares no code with
the library.  Plain module, torch only.  A kernel is a list of blocks (kind, lengthscale (Q,) or (1,), variance ()), summed.

    ft(x) = sum_d sqrt(2 var / D) w_d cos(omega_d . x + b_d),   omega_d = omegat_d / l,   omegat = z (RBF) or z sqrt(2 nu / g) (Matern-nu)
    SVGP:      f = ft + K(., Z) Kuu^-1 (u - ft(Z)),   u = m + chol(S_W S_W^T + diag(S_diag)) xi
    exact GP:  f = ft + K(., X) (K + noise I)^-1 (Y - ft(X) - sqrt(noise) eps)
    sparse GP: f = ft + K(., Z) (wv + L^-T LA^-T xi - Kuu^-1 ft(Z)),   L L^T = Kuu, LA LA^T = I + L^-1 Kuf Kfu L^-T / noise,
               wv = L^-T LA^-T LA^-1 L^-1 Kuf Y / noise

The draws are inputs, in the order the library asks its generator for them: per block z (D, Q), for Matern g (D,), the phases (D,); then the
weights (S, D_total, P); then xi (S, M, P) or eps (S, N, P)."""
import math

import torch

NU = {'rbf': None, 'matern12': 0.5, 'matern32': 1.5, 'matern52': 2.5}
t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)


def kern(blocks, X, X2=None):
    X2 = X if X2 is None else X2
    K = torch.zeros(X.shape[0], X2.shape[0], dtype=torch.float64)
    for kind, ls, var in blocks:
        d = (X[:, None, :] - X2[None, :, :]) / ls
        r2 = (d * d).sum(-1)
        r = torch.sqrt(r2.clamp_min(1e-14))
        if kind == 'rbf':
            f = torch.exp(-0.5 * r2)
        elif kind == 'matern12':
            f = torch.exp(-r)
        elif kind == 'matern32':
            f = (1 + math.sqrt(3) * r) * torch.exp(-math.sqrt(3) * r)
        else:
            f = (1 + math.sqrt(5) * r + 5.0 / 3.0 * r2) * torch.exp(-math.sqrt(5) * r)
        K = K + var * f
    return K


def basis(blocks, draws):
    """(Omega (D_total, Q), phase (D_total,), amplitude (D_total,)); consumes the leading draws and returns the rest as well"""
    draws = list(draws)
    Om, ph, amp = [], [], []
    for kind, ls, var in blocks:
        z = t64(draws.pop(0))
        if NU[kind] is not None:
            z = z * torch.sqrt(2 * NU[kind] / t64(draws.pop(0)))[:, None]
        Om.append(z / ls)
        ph.append(t64(draws.pop(0)))
        amp.append(torch.sqrt(2 * var / z.shape[0]).expand(z.shape[0]))
    return torch.cat(Om), torch.cat(ph), torch.cat(amp), draws


def features(X, Omega, phase):
    return torch.cos(X @ Omega.T + phase)                  # (N, D)


def prior(X, Omega, phase, Wa):
    """Wa (S, D, P): the weights times the amplitude -> (S, N, P)"""
    return torch.einsum('nd,sdp->snp', features(X, Omega, phase), Wa)


def _solve_chol(L, B):
    return torch.cholesky_solve(B, L)


def svgp_u(m, S_W, S_diag, xi):
    Ls = torch.linalg.cholesky(S_W @ S_W.T + torch.diag(S_diag))
    return m[None] + Ls @ xi                               # (S, M, P)


def svgp_condition(blocks, Xt, Z, ft_t, ft_Z, u, jitter=0.0):
    Kuu = kern(blocks, Z) + jitter * torch.eye(Z.shape[0], dtype=torch.float64)
    return ft_t + kern(blocks, Xt, Z) @ torch.linalg.solve(Kuu, u - ft_Z)


def gp_condition(blocks, Xt, X, Y, noise, ft_t, ft_X, eps, jitter=0.0):
    Kn = kern(blocks, X) + (noise + jitter) * torch.eye(X.shape[0], dtype=torch.float64)
    return ft_t + kern(blocks, Xt, X) @ torch.linalg.solve(Kn, Y[None] - ft_X - torch.sqrt(noise) * eps)


def sgp_posterior(blocks, X, Y, Z, noise, jitter=0.0):
    M = Z.shape[0]
    L = torch.linalg.cholesky(kern(blocks, Z) + jitter * torch.eye(M, dtype=torch.float64))
    LinvKuf = torch.linalg.solve_triangular(L, kern(blocks, Z, X), upper=False)
    LA = torch.linalg.cholesky(torch.eye(M, dtype=torch.float64) + LinvKuf @ LinvKuf.T / noise)
    c = torch.linalg.solve_triangular(LA, LinvKuf @ Y, upper=False)
    wv = torch.linalg.solve_triangular(L.T, torch.linalg.solve_triangular(LA.T, c, upper=True), upper=True) / noise
    return L, LA, wv


def sgp_condition(blocks, Xt, Z, L, LA, wv, ft_t, ft_Z, xi):
    a = torch.linalg.solve_triangular(L.T, torch.linalg.solve_triangular(LA.T, xi, upper=True), upper=True)
    return ft_t + kern(blocks, Xt, Z) @ (wv[None] + a - _solve_chol(L, ft_Z))


def _prior_at(blocks, draws, pts):
    Om, ph, amp, rest = basis(blocks, draws)
    Wa = t64(rest.pop(0)) * amp[None, :, None]
    return [prior(p, Om, ph, Wa) for p in pts], rest


def svgp_paths(blocks, Xt, Z, m, S_W, S_diag, draws, jitter=0.0):
    (ft_t, ft_Z), rest = _prior_at(blocks, draws, (Xt, Z))
    return svgp_condition(blocks, Xt, Z, ft_t, ft_Z, svgp_u(m, S_W, S_diag, t64(rest[0])), jitter)


def gp_paths(blocks, Xt, X, Y, noise, draws, jitter=0.0):
    (ft_t, ft_X), rest = _prior_at(blocks, draws, (Xt, X))
    return gp_condition(blocks, Xt, X, Y, noise, ft_t, ft_X, t64(rest[0]), jitter)


def sgp_paths(blocks, Xt, Z, L, LA, wv, draws):
    (ft_t, ft_Z), rest = _prior_at(blocks, draws, (Xt, Z))
    return sgp_condition(blocks, Xt, Z, L, LA, wv, ft_t, ft_Z, t64(rest[0]))


# ---- the kernel alone: out[s,n,j] = sum_d cos(X[s,n] . Omega[s,d] + phase[s,d]) W[s,d,j], operands with a sample axis of extent 1 or S ----------
def rff_eval(X, Omega, phase, W):
    """(out (S, N, J), the sum of the magnitudes of each element's terms sum_d |W[d,j]|)"""
    S = max(t.shape[0] for t in (X, Omega, phase, W))
    e = lambda t: t.expand((S,) + tuple(t.shape[1:]))
    arg = torch.einsum('snq,sdq->snd', e(X), e(Omega)) + e(phase)[:, None, :]
    out = torch.einsum('snd,sdj->snj', torch.cos(arg), e(W))
    return out, e(W).abs().sum(1)[:, None, :].expand_as(out)


def rff_bwd_scale(X, Omega, phase, W, G):
    """sum_d |Omega[d,q]| sum_j |G[n,j] W[d,j]| per element of dX, summed over the samples an X without a sample axis is shared by"""
    S = G.shape[0]
    e = lambda t: t.expand((S,) + tuple(t.shape[1:]))
    sc = torch.einsum('snd,sdq->snq', torch.einsum('snj,sdj->snd', G.abs(), e(W).abs()), e(Omega).abs())
    return sc if X.shape[0] == S else sc.sum(0, keepdim=True)
