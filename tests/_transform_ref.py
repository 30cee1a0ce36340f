"""CPU restatements for tests/test_normal_prec_host.py, tests/test_gpu_normal_prec.py and tests/test_gpu_logistic.py, written from the
formulas: the Normal by mean and precision, log p = (log b - log 2 pi) / 2 - b (x - a)^2 / 2, and the two variable transformations of the
segmented kernel, softplus(x) + offset and lower + (upper - lower) sigmoid(x).  numpy where a value is enough, torch where autograd
differentiates the same expression; `dtype` chooses the precision the expression itself is evaluated in (float32: the fairness check of the
float32 inputs)."""
import numpy as np
import torch

F64_BAR = 1e-9                   # relative to the sum of the magnitudes of the addends
F32_RTOL, F32_ATOL = 1e-4, 1e-5  # the bar of tests/test_gpu_normal.py
LOG2PI = float(np.log(2 * np.pi))


def tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def rounded(a, dtype):
    """values exactly representable in the dtype under test, as float64: kernel and reference see the same numbers"""
    return np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64)


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=tdt(dtype)).cuda()


def check(got, want, mag, dtype, what, worst=None):
    """float64: |got - want| <= 1e-9 * mag elementwise; float32: rtol 1e-4, atol 1e-5.  `worst` (a dict) collects the largest error seen,
    as a fraction of the bound."""
    got = got.detach().double().cpu().numpy().reshape(np.shape(want)) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    bound = F64_BAR * np.broadcast_to(mag, err.shape) if dtype == 'float64' else F32_ATOL + F32_RTOL * np.abs(want)
    if worst is not None and err.size:
        k = int(np.argmax(err / np.maximum(bound, np.finfo(np.float64).tiny)))
        frac = float(err.reshape(-1)[k] / max(float(np.reshape(bound, -1)[k]), np.finfo(np.float64).tiny))
        if frac >= worst.get(dtype, (0.0, 0.0, ''))[0]:
            worst[dtype] = (frac, float(err.reshape(-1)[k]), what)
    assert np.isfinite(got).all(), '%s: not finite' % what
    assert (err <= bound).all(), '%s: worst error %.3e against bound %.3e' % (what, err[err > bound].max(), np.asarray(bound)[err > bound].min())


# ---- NormalMeanPrecision -----------------------------------------------------------------------------------------------------------------

def normal_prec_logpdf(x, a, b):
    """torch, any dtype"""
    d = x - a
    return 0.5 * (torch.log(b) - LOG2PI) - 0.5 * b * d * d


def gamma_logpdf(x, alpha, beta):
    """torch, in the dtype of x; alpha, beta python floats: alpha log beta - lgamma(alpha) + (alpha - 1) log x - beta x"""
    import math
    return alpha * math.log(beta) - math.lgamma(alpha) + (alpha - 1.0) * torch.log(x) - beta * x


def normal_prec_reference(x, a, b, w, dtype=torch.float64):
    """log p (S, n) and the per-(s, i) gradients of sum(w * log p) w.r.t. x, a, b, each (S, n), by CPU autograd in `dtype`; float64 numpy"""
    S, n = x.shape
    leaves = [torch.as_tensor(np.broadcast_to(t, (S, n)).copy(), dtype=dtype).requires_grad_(True) for t in (x, a, b)]
    lp = normal_prec_logpdf(*leaves)
    g = torch.autograd.grad((lp * torch.as_tensor(np.broadcast_to(w, (S, n)).copy(), dtype=dtype)).sum(), leaves)
    return lp.detach().double().numpy(), [t.double().numpy() for t in g]


def normal_prec_magnitudes(x, a, b, w):
    """sum of the magnitudes of the addends of log p and of its three weighted partial derivatives, each (S, n)"""
    w = np.abs(w) + np.zeros_like(x)
    d = np.abs(x - a)
    return (0.5 * np.abs(np.log(b)) + 0.5 * LOG2PI + 0.5 * b * d * d + np.zeros_like(x), w * b * d, w * b * d, w * 0.5 * (1 / b + d * d))


# ---- transformations ---------------------------------------------------------------------------------------------------------------------

def sigmoid(x):
    """numpy, in the dtype of x, without overflow"""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def sigmoid_slope(x):
    e = np.exp(-np.abs(x))
    return e / ((1 + e) * (1 + e))


def logistic(x, lower, upper):
    return lower + (upper - lower) * sigmoid(x)


def logistic_slope(x, lower, upper):
    return (upper - lower) * sigmoid_slope(x)


def softplus(x, offset=0.0):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))) + offset


def logistic_t(x, lower, upper):
    """torch, for autograd"""
    return lower + (upper - lower) * torch.sigmoid(x)
