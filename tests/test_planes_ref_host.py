"""CPU tests of the split-plane reference (tests/_planes_ref.py) the GPU tests of the plane producers compare against bit for bit, and of
the mxf_gram_planes entry point's declaration.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import _planes_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_gram_planes',)


def test_new_entry_point_is_declared_bound_and_exported():
    from mxfusion_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert callable(ops.gram_planes)
    for doc in ('INTEGRATION.md', 'DESIGN.md'):
        assert 'mxf_gram_planes' in open(os.path.join(ROOT, doc)).read(), doc


@pytest.mark.parametrize('R,K', [(1, 1), (3, 15), (5, 16), (7, 17), (65, 50), (2, 67)])
@pytest.mark.parametrize('NP', [2, 3])
def test_encode_decode_round_trip(R, K, NP):
    rng = np.random.RandomState(R * 100 + K)
    terms = [rng.randint(-2 ** 15, 2 ** 15, (R, K)).astype(np.int16) for _ in range(NP)]
    flat = P.encode(terms, R, K)
    K16 = (K + 15) // 16
    assert flat.dtype == np.int16 and flat.size == NP * P.plane_elems(R, K) == NP * K16 * R * 16
    dec = P.decode(flat, R, K, NP)
    assert dec.shape == (NP, R, K16 * 16)
    for q in range(NP):
        assert np.array_equal(dec[q][:, :K], terms[q])
        assert not dec[q][:, K:].any()
    # the address formula itself, element by element
    n = P.plane_elems(R, K)
    for q in range(NP):
        for r in (0, R // 2, R - 1):
            for k in (0, K // 2, K - 1):
                assert flat[q * n + ((k // 16) * R + r) * 16 + k % 16] == terms[q][r, k]


def _operand(seed, R, K, mag):
    rng = np.random.RandomState(seed)
    X = rng.randn(R, K) * np.exp(rng.randn(R, 1)) * mag
    X[rng.rand(R, K) < 0.05] = -0.0
    return X.astype(np.float32)


@pytest.mark.parametrize('mag', [1.0, 3e-6, 7e5, 1.5 * 2.0 ** -86, 1.5 * 2.0 ** 113])
def test_hi_plus_lo_reproduces_the_scaled_operand(mag):
    X = _operand(1, 70, 33, 1.0)
    X = (X / np.abs(X).max() * np.float32(mag)).astype(np.float32)
    hi, lo, s = P.f16x2_ref(X)
    assert np.isfinite(hi.astype(np.float64)).all()
    xs = X.astype(np.float64) * s
    assert 2.0 ** 13 <= np.abs(xs).max() < 2.0 ** 14
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - xs)
    assert (err <= 2.0 ** -22 * np.abs(xs) + 2.0 ** -25).all(), float((err / (2.0 ** -22 * np.abs(xs) + 2.0 ** -25)).max())
    # lo is a residual of hi: at most half a unit in the last place of hi
    assert (np.abs(lo.astype(np.float64)) <= P.f16_ulp(hi) / 2).all()
    # and the float32 arithmetic of the kernel gives the same bits (x s and the residual are exact in float32)
    xs32 = X * np.float32(s)
    hi32 = xs32.astype(np.float16)
    lo32 = (xs32 - hi32.astype(np.float32)).astype(np.float16)
    assert np.array_equal(hi32.view(np.int16), hi.view(np.int16)) and np.array_equal(lo32.view(np.int16), lo.view(np.int16))


def test_three_bf16_terms_sum_to_the_operand_exactly():
    for mag in (1.0, 3e-6, 7e5):
        X = _operand(2, 64, 40, mag)
        (hb, mb, lb), (h, m, l) = P.bf16x3_ref(X)
        nz = X != 0
        assert (np.abs(X[nz]) >= 2.0 ** -100).all()           # normal floats, far from the underflow of the third term
        tot = h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)
        assert np.array_equal(tot, X.astype(np.float64))
        # every term is a bf16: the low 16 bits of its float32 pattern are zero; -0.0 keeps its sign in h and leaves m = l = +0
        for t in (h, m, l):
            assert not (t.view(np.uint32) & 0xffff).any()
        z = (X == 0) & np.signbit(X)
        assert z.any() and (hb[z] == 0x8000).all() and not mb[z].any() and not lb[z].any()
    # round to nearest EVEN at the tie: 1 + 2^-8 sits half way between the bf16 neighbours 1 and 1 + 2^-7
    b, v = P.to_bf16(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)], np.float32))
    assert list(v) == [1.0, 1 + 2.0 ** -6, -1.0] and list(b) == [0x3f80, 0x3f82, 0xbf80]


def test_scale_at_powers_of_two_and_at_both_clamp_ends():
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))
    for k in (-80, -20, -1, 0, 1, 13, 14, 15, 60, 110):
        m = 2.0 ** k
        assert P.scale_from_max(m) == 2.0 ** (13 - k), k                 # 2^k -> exactly 2^13
        assert P.scale_from_max(-m) == 2.0 ** (13 - k)
        assert P.scale_from_max(below(m)) == 2.0 ** (14 - k), k          # one ulp below 2^k -> just under 2^14
        assert P.scale_from_max(1.5 * m) == 2.0 ** (13 - k)
    # the clamp: e = 14 - (ex - 126) = 140 - ex for the biased exponent ex, held to +-100, i.e. ex in [40, 240]
    assert P.scale_from_max(1.5 * 2.0 ** -86) == 2.0 ** 99 and P.scale_from_max(2.0 ** -87) == 2.0 ** 100      # ex = 41, 40
    assert P.scale_from_max(below(2.0 ** -87)) == 2.0 ** 100 and P.scale_from_max(2.0 ** -120) == 2.0 ** 100   # ex < 40: clamped
    assert P.scale_from_max(1.5 * 2.0 ** 113) == 2.0 ** -100 and P.scale_from_max(below(2.0 ** 113)) == 2.0 ** -99   # ex = 240, 239
    assert P.scale_from_max(2.0 ** 114) == 2.0 ** -100 and P.scale_from_max(2.0 ** 127) == 2.0 ** -100         # ex > 240: clamped
    # zero, denormal and non-finite maxima leave the operand unscaled
    for m in (0.0, -0.0, 2.0 ** -127, 2.0 ** -149, float('inf'), float('nan')):
        assert P.scale_from_max(m) == 1.0, m
    assert P.scale_from_max(2.0 ** -126) == 2.0 ** 100
    # the bit-level form of split_device.h gives the same over a sweep of exponents
    for ex in range(0, 256, 3):
        for frac in (0, 1, 0x7fffff):
            bits = np.uint32((ex << 23) | frac)
            e = 140 - ex
            want = 1.0 if ex in (0, 255) else 2.0 ** min(100, max(-100, e))
            assert P.scale_from_max(np.array([bits], np.uint32).view(np.float32)[0]) == want, (ex, frac)


def test_max_word_ignores_the_sign_and_negative_zero():
    X = np.array([[0.5, -3.25, 1.0], [-0.0, 2.0, 3.0]], np.float32)
    assert P.max_word(X) == int(np.float32(3.25).view(np.int32))
    assert P.max_word(np.array([[-0.0, 0.0]], np.float32)) == 0
    planes, word = P.f16x2_planes_ref(np.zeros((3, 5), np.float32))
    assert word == 0 and not planes.any()


def test_gram64_weights_follow_the_period():
    rng = np.random.RandomState(0)
    Xmin, Xmaj = rng.uniform(-2, 2, (9, 3)), rng.uniform(-2, 2, (11, 3))
    ls, var = np.array([1.1, 0.9, 1.4]), np.array([1.3])
    K = P.gram64('rbf', Xmin, Xmaj, ls, var)
    d = (Xmin[4] - Xmaj[7]) / ls
    assert abs(K[4, 7] - 1.3 * np.exp(-0.5 * (d * d).sum())) <= 1e-15
    majs, mins = rng.uniform(0.2, 1, 4), rng.uniform(0.2, 1, 4)
    Kw = P.gram64('rbf', Xmin, Xmaj, ls, var, majs=majs, mins=mins, period=4)
    assert abs(Kw[6, 9] - K[6, 9] * majs[1] * mins[2]) <= 1e-16
