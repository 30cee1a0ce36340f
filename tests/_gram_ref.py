"""Host reference of the stationary Gram reverse mode (mxf_gram_bwd): the closed-form gradient in the DIFFERENCE form, in a precision of
the caller's choice.  Plain module, no fixtures, numpy only.

    d_q = (x_q - z_q) / l_q        r2 = sum_q d_q^2        k = var f(r2)        W = 2 G var f'(r2)          (G = dK, the upstream gradient)

    dvar   = sum_ij G f
    dX_iq  =  sum_j W_ij d_q / l_q
    dX2_jq = -sum_i W_ij d_q / l_q            (square Gram, X2 = None: both roles flow into dX)
    dl_q   = -sum_ij W d_q^2 / l_q            (isotropic length-scale: summed over q)

and every operand shared by the samples (leading extent 1) collects the sum over s.  The conventions at r2 -> 0 are the library's and the
reference project's (autograd through sqrt(clamp(r2, 1e-14))): Matern kinds use r = sqrt(max(r2, CLIP)); where r2 < CLIP the slope f' is 0 for
Matern12 and Matern32 and 5/3 e^(-sqrt(5) r) for Matern52 (whose 5/3 r2 term keeps the un-clipped r2).

Besides each gradient the functions return the same sum over the ABSOLUTE values of its terms: the scale a rounding-error bound is relative
to (|got - ref| <= c u abs_sum per element), as |A||B| is for a matrix product.

The difference form is exact where the expansion form |x|^2 - 2 x.z + |z|^2 of the oracle loses ~1e-8 on close pairs, so it serves the
Matern12 / Q = 1 cases the oracle cannot referee."""
import numpy as np

KINDS = ('rbf', 'matern12', 'matern32', 'matern52')
KIND_ID = {'rbf': 0, 'matern12': 1, 'matern32': 2, 'matern52': 3}
CLIP = 1e-14

# the bar of the GPU tests: |got - ref| <= BAR_C u abs_sum per element (u = 2^-53 / 2^-24); how the constants were set is written down in the
# header of tests/test_gpu_gram_bwd_axes.py
BAR_C = {'f64': 2.0 ** 14, 'f32': 2.0 ** 13}

LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 2e-19)        # x87 extended (64-bit significand) or better
HI = np.longdouble if LONGDOUBLE_OK else np.float64              # the precision float64 results are compared in


def f_and_slope(kind, r2):
    """unit-variance covariance f(r2) and slope df/d(r2), elementwise, in r2's dtype"""
    dt = r2.dtype.type
    if kind == 'rbf':
        f = np.exp(dt(-0.5) * r2)
        return f, dt(-0.5) * f
    clipped = r2 < dt(CLIP)
    r = np.sqrt(np.where(clipped, dt(CLIP), r2))
    zero = np.zeros_like(r2)
    if kind == 'matern12':
        f = np.exp(-r)
        return f, np.where(clipped, zero, -f / (dt(2) * r))
    if kind == 'matern32':
        s3 = np.sqrt(dt(3))
        e = np.exp(-s3 * r)
        return (dt(1) + s3 * r) * e, np.where(clipped, zero, dt(-1.5) * e)
    if kind == 'matern52':
        s5 = np.sqrt(dt(5))
        e = np.exp(-s5 * r)
        f = (dt(1) + s5 * r + dt(5) / dt(3) * r2) * e
        return f, np.where(clipped, dt(5) / dt(3) * e, dt(-5) / dt(6) * (dt(1) + s5 * r) * e)
    raise ValueError(kind)


def _operands(X, X2, ls, var, dtype):
    X, ls, var = (np.asarray(a, dtype=dtype) for a in (X, ls, var))
    X2 = None if X2 is None else np.asarray(X2, dtype=dtype)
    assert X.ndim == 3 and ls.ndim == 2 and var.ndim == 2 and (X2 is None or X2.ndim == 3)
    return X, X2, ls, var


def _sample(a, s):
    return a[s if a.shape[0] > 1 else 0]


def gram_ref(kind, X, X2, ls, var, dtype=np.float64, S=None):
    """forward value K (S, N, N2) in `dtype` with the same conventions (the function the gradients below differentiate)"""
    X, X2, ls, var = _operands(X, X2, ls, var, dtype)
    S = S or max(a.shape[0] for a in (X, ls, var) + (() if X2 is None else (X2,)))
    out = []
    for s in range(S):
        x, l, v = _sample(X, s), _sample(ls, s), _sample(var, s)
        z = x if X2 is None else _sample(X2, s)
        d = (x[:, None, :] - z[None, :, :]) / l
        out.append(v[0] * f_and_slope(kind, (d * d).sum(-1))[0])
    return np.stack(out)


def gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=np.float64):
    """X (S|1, N, Q), X2 (S|1, N2, Q) or None (square), ls (S|1, Q) (ARD) or (S|1, 1), var (S|1, 1), dK (S, N, N2): anything numpy converts.
    Returns (grad, scale): dicts with the keys 'dX', 'dX2' (None when square), 'dls', 'dvar', shaped like the primals, dtype `dtype`;
    scale[k] is the sum of the absolute values of the terms of grad[k].  One sample and one coordinate at a time: the temporaries are (N, N2)."""
    X, X2, ls, var = _operands(X, X2, ls, var, dtype)
    S, N, N2 = np.shape(dK)
    Q = X.shape[-1]
    square = X2 is None
    assert X.shape[1] == N and (N2 == N if square else X2.shape[1:] == (N2, Q)) and ls.shape[1] in (1, Q) and var.shape[1] == 1
    names = ('dX', 'dX2', 'dls', 'dvar')
    prim = dict(dX=X, dX2=X2, dls=ls, dvar=var)
    grad = {k: None if prim[k] is None else np.zeros(prim[k].shape, dtype) for k in names}
    scale = {k: None if prim[k] is None else np.zeros(prim[k].shape, dtype) for k in names}
    for s in range(S):
        ix, il, iv = (s if a.shape[0] > 1 else 0 for a in (X, ls, var))
        iz = ix if square else (s if X2.shape[0] > 1 else 0)
        x, z = X[ix], (X[ix] if square else X2[iz])
        l = np.broadcast_to(ls[il], (Q,))
        v = var[iv, 0]
        G = np.asarray(dK[s], dtype=dtype)
        d = [(x[:, None, q] - z[None, :, q]) / l[q] for q in range(Q)]
        r2 = np.zeros((N, N2), dtype)
        for dq in d:
            r2 += dq * dq
        f, fp = f_and_slope(kind, r2)
        W = dtype(2) * G * v * fp
        aW = np.abs(W)
        grad['dvar'][iv, 0] += (G * f).sum()
        scale['dvar'][iv, 0] += (np.abs(G) * f).sum()
        for q in range(Q):
            t = W * d[q] / l[q]
            at = np.abs(t)
            grad['dX'][ix, :, q] += t.sum(1)
            scale['dX'][ix, :, q] += at.sum(1)
            cg, cs = ('dX', ix) if square else ('dX2', iz)
            grad[cg][cs, :, q] -= t.sum(0)
            scale[cg][cs, :, q] += at.sum(0)
            ql = q if ls.shape[1] > 1 else 0
            grad['dls'][il, ql] -= (W * d[q] * d[q]).sum() / l[q]
            scale['dls'][il, ql] += (aW * d[q] * d[q]).sum() / l[q]
    return grad, scale


# ---- the sample-axis patterns: which of X, X2, ls, var carry the sample axis (True) and which are shared by the samples (extent 1) ---------------
RECT_PATTERNS = [(a, b, c, d) for a in (False, True) for b in (False, True) for c in (False, True) for d in (False, True)]      # (X, X2, ls, var)
SQUARE_PATTERNS = [(a, None, c, d) for a in (False, True) for c in (False, True) for d in (False, True)]                       # X2 = None


def pattern_id(p):
    return ''.join(n + ('-' if f is None else 'S' if f else '1') for n, f in zip(('X', 'Z', 'l', 'v'), p))


def make_case(seed, N, N2, Q, ard, pattern, S=3, f32=False):
    """random operands of one call as float64 numpy arrays: inputs uniform(-2, 2), length-scales in [0.8, 1.8], variance in [0.5, 1.5], dK
    standard normal of shape (S, N, N2); N2 = None or pattern[1] = None: square.  f32: every value is rounded to float32 first, so a float32
    run and its float64 reference start from the same numbers."""
    rng = np.random.RandomState(seed)
    sx, sz, sl, sv = pattern
    square = N2 is None or sz is None
    e = lambda flag: S if flag else 1
    X = rng.uniform(-2, 2, (e(sx), N, Q))
    X2 = None if square else rng.uniform(-2, 2, (e(sz), N2, Q))
    ls = rng.uniform(0.8, 1.8, (e(sl), Q if ard else 1))
    var = rng.uniform(0.5, 1.5, (e(sv), 1))
    dK = rng.randn(S, N, N if square else N2)
    if f32:
        X, ls, var, dK = (a.astype(np.float32).astype(np.float64) for a in (X, ls, var, dK))
        X2 = None if X2 is None else X2.astype(np.float32).astype(np.float64)
    return X, X2, ls, var, dK


def worst_ratio(got, ref, scale, u):
    """max over the elements of |got - ref| / (u scale) -- in units of roundoffs of the absolute sum.  An element whose scale is 0 has no
    non-zero term: it must be reproduced exactly (ratio 0) and counts as infinitely wrong otherwise; a non-finite result is infinitely wrong."""
    got = np.asarray(got, dtype=ref.dtype).reshape(ref.shape)
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float('inf')
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(scale > 0, err / (ref.dtype.type(u) * scale), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0
