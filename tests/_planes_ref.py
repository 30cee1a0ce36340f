"""Host reference of the split-plane operand formats (mxfusion_amd/csrc/gemm_split.hip, split_device.h, gram.hip).  Plain module, no
fixtures, numpy only; every function restates its definition, none calls the library.

Layout ("k16-blocked"): plane p of an (R x K) operand is K16 = ceil(K / 16) blocks of (R rows x 16 k); element (r, k) sits at
((k // 16) * R + r) * 16 + k % 16, the columns K .. 16 K16 - 1 of the last block are zero, and the NP planes follow one another.

    f16x2  : x * s = hi + lo, two f16 terms, s = scale_from_max(max |x|)
    bf16x3 : x = h + m + l, three bf16 terms

Both are round-to-nearest-even at every step, so the planes are determined by the operand bit for bit."""
import numpy as np

import _gram_ref as G


def plane_elems(R, K):
    return ((K + 15) // 16) * R * 16


def encode(terms, R, K):
    """terms: NP arrays (R, K) of 16-bit patterns (any 2-byte dtype) -> the flat int16 planes, k padding zero"""
    K16 = (K + 15) // 16
    out = []
    for t in terms:
        t = np.ascontiguousarray(t).view(np.int16).reshape(R, K)
        pad = np.zeros((R, K16 * 16), np.int16)
        pad[:, :K] = t
        out.append(pad.reshape(R, K16, 16).transpose(1, 0, 2).reshape(-1))
    return np.concatenate(out)


def decode(planes, R, K, NP):
    """flat planes -> int16 (NP, R, 16 * K16): the k padding is returned too (columns K ..), so that a test can look at it"""
    K16 = (K + 15) // 16
    n = K16 * R * 16
    p = np.ascontiguousarray(planes).view(np.int16).reshape(-1)
    assert p.size == NP * n, (p.size, NP, n)
    return np.stack([p[q * n:(q + 1) * n].reshape(K16, R, 16).transpose(1, 0, 2).reshape(R, K16 * 16) for q in range(NP)])


def scale_from_max(x):
    """The power of two s that puts the maximum magnitude x (a float32 value) at x * s in [2^13, 2^14), its exponent clamped to +-100;
    1 for a zero, denormal or non-finite maximum (split_device.h)."""
    x = float(np.float32(abs(x)))
    if not np.isfinite(x) or x < 2.0 ** -126:
        return 1.0
    _, ex = np.frexp(x)                  # x in [2^(ex - 1), 2^ex)
    e = min(100, max(-100, 14 - int(ex)))
    return 2.0 ** e


def max_word(X):
    """bit pattern (as int32) of max |X| over a float32 array"""
    X = np.asarray(X, np.float32)
    if X.size == 0:
        return 0
    return int(np.abs(X).max().view(np.int32))


def f16x2_ref(X):
    """(hi, lo, s): hi = f16(x s), lo = f16(x s - hi) as float16 arrays shaped like X (float32).  x s is exact (a power of two; formed in
    float64) and so is the residual, so each term is ONE round-to-nearest-even conversion."""
    X = np.asarray(X, np.float32)
    s = scale_from_max(np.abs(X).max() if X.size else 0.0)
    xs = X.astype(np.float64) * s
    with np.errstate(over='ignore'):
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float64)).astype(np.float16)
    return hi, lo, s


def f16x2_planes_ref(X):
    """(planes int16, max word) as mxf_f16x2_split writes them"""
    X = np.asarray(X, np.float32)
    hi, lo, _ = f16x2_ref(X)
    return encode([hi, lo], X.shape[0], X.shape[1]), max_word(X)


def to_bf16(x):
    """float32 array -> (uint16 bit patterns, the same values as float32), round-to-nearest-even (finite inputs)"""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return r, (r.astype(np.uint32) << 16).view(np.float32)


def bf16x3_ref(X):
    """(h, m, l) bit patterns (uint16) and their float32 values: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m); the residuals are exact
    in float32 (formed in float64 and cast back, which checks nothing away: the cast is exact)"""
    X = np.asarray(X, np.float32)
    hb, h = to_bf16(X)
    r1 = (X.astype(np.float64) - h).astype(np.float32)
    mb, m = to_bf16(r1)
    r2 = (r1.astype(np.float64) - m).astype(np.float32)
    lb, l = to_bf16(r2)
    return (hb, mb, lb), (h, m, l)


def bf16x3_planes_ref(X):
    X = np.asarray(X, np.float32)
    return encode(list(bf16x3_ref(X)[0]), X.shape[0], X.shape[1])


def f16_ulp(h):
    """spacing of float16 at |h| (float64 array): 2^(e - 10) for a normal h in [2^e, 2^(e+1)), 2^-24 below 2^-14"""
    a = np.abs(np.asarray(h, np.float64))
    _, ex = np.frexp(np.where(a > 0, a, 1.0))
    return np.where(a >= 2.0 ** -14, 2.0 ** (ex - 1 - 10), 2.0 ** -24)


def gram64(kind, Xmin, Xmaj, ls, var, majs=None, mins=None, period=1):
    """float64 stationary Gram cov(Xmin[r], Xmaj[k]) (R x Kn) in the difference form (tests/_gram_ref.py), times majs[k % period] and / or
    mins[r % period].  ls: (Q,) or (1,)."""
    Xmin, Xmaj = np.asarray(Xmin, np.float64), np.asarray(Xmaj, np.float64)
    K = G.gram_ref(kind, Xmin[None], Xmaj[None], np.asarray(ls, np.float64).reshape(1, -1), np.asarray(var, np.float64).reshape(1, 1))[0]
    R, Kn = K.shape
    if majs is not None:
        K = K * np.asarray(majs, np.float64)[np.arange(Kn) % period][None, :]
    if mins is not None:
        K = K * np.asarray(mins, np.float64)[np.arange(R) % period][:, None]
    return K
