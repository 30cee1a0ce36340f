"""Float64 reference of the robust-max multi-class SVGP (torch on the CPU), written from the formulas of the likelihood -- not from the kernel:

  p = P(f_y is the largest) = sum_k w_k prod_{c != y} Phi((m_y - m_c) / sqrt(max(v, 1e-12)) + sqrt(2) x_k), term by term over (N, nodes, C);
  E[log p(y | f)] = L0 + p (L1 - L0), L1 = log(1 - eps), L0 = log(eps / (C - 1));  probs[c] = p with the label set to c;
  the bound  c sum_n E[log p] - w KL(q(u) || p(u))  over C latent functions, with the marginals and the KL term of tests/_lik_ref.py.

Every reference gradient is autograd on these (torch.clamp passes the gradient in v from the floor upwards and none below it)."""
import math

import torch

import _lik_ref as L

FLOOR = 1e-12


def labels(y, C):
    """the label column as the kernel reads it: truncated toward zero, clamped to [0, C - 1]; (..., N, 1) -> (..., N) int64"""
    return torch.clamp(torch.trunc(torch.as_tensor(y, dtype=torch.float64)[..., 0]), 0, C - 1).long()


def node_products(y, m, v, nq=20):
    """P_k = prod_{c != y} Phi(z_kc), (..., N, K), and the rule's weights: y (..., N) int64, m (..., N, C), v (..., N)"""
    x, w = L.rule(nq)
    C = m.shape[-1]
    my = torch.gather(m, -1, y.unsqueeze(-1))
    d = (my - m) / torch.sqrt(torch.clamp(v, min=FLOOR)).unsqueeze(-1)             # (..., N, C)
    z = d.unsqueeze(-2) + math.sqrt(2.0) * x[:, None]                               # (..., N, K, C)
    own = torch.nn.functional.one_hot(y, C).bool().unsqueeze(-2)
    logphi = torch.where(own, torch.zeros((), dtype=z.dtype), torch.special.log_ndtr(z))
    return torch.exp(logphi.sum(-1)), w


def p_correct(y, m, v, nq=20):
    P, w = node_products(y, m, v, nq)
    return (P * w).sum(-1)


def log_levels(eps, C):
    return math.log(eps / (C - 1)), math.log1p(-eps)


def expect_elem(y, m, v, eps, nq=20):
    """E[log p(y | f)] per row, (..., N)"""
    l0, l1 = log_levels(eps, m.shape[-1])
    return l0 + (l1 - l0) * p_correct(y, m, v, nq)


def probs(m, v, nq=20):
    """P(f_c is the largest) for every class, (..., N, C); not renormalised"""
    C = m.shape[-1]
    return torch.stack([p_correct(torch.full(m.shape[:-1], c, dtype=torch.int64), m, v, nq) for c in range(C)], -1)


def svgp_bound(K, Kdiag, X, y, Z, qm, qW, qd, eps, jitter=0., scaling=1.0, kl_weight=1.0, nq=20):
    """scaling * sum_n E[log p(y_n | f_n)] - kl_weight * KL(q(u) || p(u)), one sample: y (N,) int64, qm (M, C)"""
    m, v, (Lc, Lmu, B, S) = L.marginals(K, Kdiag, X, Z, qm, qW, qd, jitter)
    M, P = qm.shape
    kl = 0.5 * (P * torch.trace(B) + (Lmu * Lmu).sum() - P * M + P * (2.0 * torch.log(torch.diagonal(Lc)).sum() - torch.logdet(S)))
    return scaling * expect_elem(y, m, v, eps, nq).sum() - kl_weight * kl
