"""The three producers of split planes, each on its own against a host reference (tests/_planes_ref.py):

  (a) mxf_f16x2_split  -- split_planes_kernel<2> + the max-abs word: bit for bit
  (b) the two max-abs kernels behind it, on the same values
  (c) mxf_f32x3_split  -- split_planes_kernel<3>: bit for bit
  (d) mxf_gram_planes  -- gram_planes_lean_kernel: values against the float64 Gram at the float32 Gram's own bound, structure exactly
  (e) mxf_gram_planes  -- the fused row U = w^T K and the majs / mins weights

Every output buffer is pre-filled with a sentinel and followed by GUARD more sentinel words: an element the kernel must write (the k padding
included) cannot pass by luck, and a store behind the buffer is seen.  The entry points are called through _lib.call with explicit pointers
and leading dimensions (ops.* makes its operands contiguous and allocates the outputs itself)."""
import numpy as np
import pytest
import torch

import _planes_ref as P
import _strided as SV

pytestmark = pytest.mark.gpu

GUARD = 64
SENT16 = 0x5A5B                  # as f16 about 203: no k padding, and no Gram plane element by accident
SENT32 = SV.SENTINEL


def _ctx():
    from mxfusion_amd import _lib
    return _lib, _lib.handle(torch.cuda.current_device()), torch.cuda.current_stream().cuda_stream


def _guarded16(n):
    return torch.full((n + GUARD,), SENT16, dtype=torch.int16, device='cuda')


def _take(buf, n, what):
    """the n payload words as numpy, after checking that the guard words behind them still hold the sentinel"""
    host = buf.cpu().numpy()
    assert (host[n:] == host.dtype.type(SENT16 if host.dtype == np.int16 else SENT32)).all(), '%s: guard words behind the buffer were written' % what
    return host[:n]


def _split(mode, X):
    """mxf_f16x2_split / mxf_f32x3_split of a 2-D float32 device view (any row stride, any alignment) into a guarded buffer"""
    lib, h, st = _ctx()
    R, K = X.shape
    NP = 2 if mode == 'f16x2' else 3
    n = NP * lib.load().mxf_f32x3_plane_elems(R, K)
    assert n == NP * P.plane_elems(R, K)
    buf = _guarded16(n)
    if mode == 'f16x2':
        word = torch.zeros(1, dtype=torch.int32, device='cuda')
        lib.call('mxf_f16x2_split', h, R, K, X.data_ptr(), X.stride(0), buf.data_ptr(), word.data_ptr(), st)
        return _take(buf, n, mode), int(word.item())
    lib.call('mxf_f32x3_split', h, R, K, X.data_ptr(), X.stride(0), buf.data_ptr(), st)
    return _take(buf, n, mode), None


# (R, K, layout): layout is a tests/_strided.py variant -- 'plain' contiguous and 16-byte aligned (float4 loads where K % 4 == 0 and k + 3 < K),
# 'ld+8' the float4 path with ld != K, ('odd', 3, 1, 0) a row-slice view at an odd element offset with ld % 4 != 0 (scalar loads; the
# allocation around the view is NaN, so an over-read shows in the max word)
ODD = ('odd', 3, 1, 0)
SHAPES = [(1, 1, 'plain'), (63, 15, 'plain'), (64, 16, 'plain'), (65, 17, 'plain'), (130, 50, 'plain'), (200, 67, 'plain'),
          (70, 64, ODD), (70, 64, 'ld+8')]
SCALE_CASES = ('pow2', 'pow2-ulp', 'clamp-lo', 'clamp-hi')
CASES = ('mag1', 'mag3e-6', 'mag7e5', 'negmax', 'lastmax', 'negzero', 'zero') + SCALE_CASES


def _contents(case, R, K):
    """float32 (R, K): both signs, per-row magnitudes spread over e^N(0,1), a few -0.0 entries, and what `case` names"""
    rng = np.random.RandomState(R * 1000 + K)
    X = rng.randn(R, K) * np.exp(rng.randn(R, 1))
    X[rng.rand(R, K) < 0.03] = -0.0
    X = X.astype(np.float32)
    top = float(np.abs(X).max()) or 1.0
    at = (int(rng.randint(R)), int(rng.randint(K)))         # where a planted maximum goes
    if case.startswith('mag'):
        X = (X * np.float32(float(case[3:]))).astype(np.float32)
    elif case == 'negmax':
        X[at] = -1.5 * top
    elif case == 'lastmax':
        X[R - 1, K - 1] = 2.0 * top
    elif case == 'negzero':
        X[rng.rand(R, K) < 0.3] = -0.0
        X[R // 2, :] = -0.0
    elif case == 'zero':
        X = np.zeros((R, K), np.float32)
    elif case in ('pow2', 'pow2-ulp'):                       # the boundaries of scale_from_maxbits: max = 2^3, and one ulp below it
        X = (X / np.float32(top) * np.float32(7.0)).astype(np.float32)
        X[at] = np.float32(8.0) if case == 'pow2' else -np.nextafter(np.float32(8.0), np.float32(0))
    elif case in ('clamp-lo', 'clamp-hi'):                   # the last exponents inside the +-100 clamp: e = 140 - ex = 99 and -100
        m = 1.5 * 2.0 ** (-86 if case == 'clamp-lo' else 113)
        X = (X.astype(np.float64) / top * (0.9 * m)).astype(np.float32)
        X[at] = -m if case == 'clamp-lo' else m
    else:
        raise ValueError(case)
    return X


def _assert_planes_equal(got, want, R, K, NP, what):
    if not torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(want.copy())):
        g, w = P.decode(got, R, K, NP), P.decode(want, R, K, NP)
        bad = np.argwhere(g != w)
        raise AssertionError('%s: %d of %d plane words differ; first (plane, r, k) = %s: got 0x%04x, want 0x%04x'
                             % (what, len(bad), g.size, tuple(bad[0]), int(g[tuple(bad[0])]) & 0xffff, int(w[tuple(bad[0])]) & 0xffff))


def _assert_padding_zero(got, R, K, NP, what):
    assert not P.decode(got, R, K, NP)[:, :, K:].any(), '%s: the k padding of the last block is not zero' % what


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('R,K,layout', SHAPES, ids=lambda v: v if isinstance(v, str) else (v[0] if isinstance(v, tuple) else str(v)))
def test_f16x2_split_bit_for_bit(R, K, layout, case):
    """Planes and max word of mxf_f16x2_split equal the reference as integers: the scale is a power of two (x s exact), the residual x s - hi
    is exact in float32, and both conversions round to nearest even -- f16 denormals included (lo of small elements is one)."""
    Xh = _contents(case, R, K)
    X = SV.carve_as(Xh, layout)
    snap = SV.snapshot(X)
    got, word = _split('f16x2', X)
    SV.assert_unchanged(X, snap)
    want, wword = P.f16x2_planes_ref(Xh)
    assert word == wword, (hex(word), hex(wword))
    assert word == int(torch.from_numpy(Xh).abs().max().view(torch.int32))
    _assert_padding_zero(got, R, K, 2, case)
    _assert_planes_equal(got, want, R, K, 2, case)
    if case == 'zero':
        assert word == 0 and not got.any()
    elif np.abs(Xh).max() > 0:              # the case is what it says: the scaled maximum sits in [2^13, 2^14)
        hi =P.decode(got, R, K, 2)[0].view(np.float16).astype(np.float64)
        assert 2.0 ** 13 <= np.abs(hi).max() <= 2.0 ** 14
        if case == 'pow2':
            assert np.abs(hi).max() == 2.0 ** 13
        if case == 'pow2-ulp':
            assert np.abs(hi).max() == 2.0 ** 14        # 2^14 (1 - 2^-24) rounds up to 2^14 in f16: the closed end of [2^13, 2^14]


def test_gemm_f16x2_at_both_ends_of_the_scale_clamp():
    """The clamp ends through their consumer: A with maximum 1.5 * 2^113 (scale 2^-100) times B with maximum 1.5 * 2^-86 (scale 2^99) is
    within the 6e-7 of sum |a||b| that tests/test_gpu_gemm.py asks of every mxf_gemm_f16x2 product, measured in float64."""
    from mxfusion_amd import ops
    A = torch.from_numpy(_contents('clamp-hi', 128, 64)).cuda()
    B = torch.from_numpy(_contents('clamp-lo', 128, 64)).cuda()
    assert float(A.abs().max()) == 1.5 * 2.0 ** 113 and float(B.abs().max()) == 1.5 * 2.0 ** -86
    C = ops.gemm_f16x2(A, B)
    ref = A.double() @ B.double().T
    scale = A.double().abs() @ B.double().abs().T
    e = float(((C.double() - ref).abs() / scale).max())
    print('gemm_f16x2 at the clamp ends: %.3g of sum|a||b|' % e)
    assert torch.isfinite(C).all() and e < 6e-7, e


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------
def test_both_maxabs_kernels_on_the_same_values():
    """mxf_maxabs_internal launches maxabs_flat_kernel (16-byte loads over the flat operand) when ld == K, R K % 4 == 0, the pointer is
    16-byte aligned and R K >= 2^22, and maxabs_kernel (element-wise, two divisions per element) otherwise.  R = 2, K = 2^21 + 2 gives
    R K = 2^22 + 4 contiguous elements: the first operand takes the flat kernel, the same values at ld = K + 4 take the element-wise one.
    The maximum sits among the last four elements (the flat kernel's last 16-byte load).  Both words equal the reference and the two plane
    sets are bit-equal to each other and to the reference."""
    R, K = 2, 2 ** 21 + 2
    rng = np.random.RandomState(7)
    Xh = (rng.randn(R, K) * 3.0).astype(np.float32)
    Xh[R - 1, K - 3] = -1.25 * float(np.abs(Xh).max())
    flat, padded = SV.carve(Xh, device='cuda'), SV.carve(Xh, ld_pad=4, device='cuda')
    assert flat.is_contiguous() and flat.stride(0) == K and flat.data_ptr() % 16 == 0 and (R * K) % 4 == 0 and R * K >= 2 ** 22
    assert padded.stride(0) == K + 4
    p1, w1 = _split('f16x2', flat)
    p2, w2 = _split('f16x2', padded)
    want, wword = P.f16x2_planes_ref(Xh)
    assert w1 == wword and w2 == wword, (hex(w1), hex(w2), hex(wword))
    assert torch.equal(torch.from_numpy(p1), torch.from_numpy(p2))
    assert torch.equal(torch.from_numpy(p1), torch.from_numpy(want))


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in CASES if c not in SCALE_CASES])
@pytest.mark.parametrize('R,K,layout', SHAPES, ids=lambda v: v if isinstance(v, str) else (v[0] if isinstance(v, tuple) else str(v)))
def test_f32x3_split_bit_for_bit(R, K, layout, case):
    """The three bf16 planes of mxf_f32x3_split equal h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (round to nearest even, exact
    residuals) as integers; k padding zero, guard words untouched, the operand unchanged."""
    Xh = _contents(case, R, K)
    X = SV.carve_as(Xh, layout)
    snap = SV.snapshot(X)
    got, _ = _split('f32x3', X)
    SV.assert_unchanged(X, snap)
    _assert_padding_zero(got, R, K, 3, case)
    _assert_planes_equal(got, P.bf16x3_planes_ref(Xh), R, K, 3, case)
    if case == 'zero':
        assert not got.any()
    else:                                   # what the format promises, on the kernel's own output: the three terms sum to x exactly
        t = (P.decode(got, R, K, 3)[:, :, :K].astype(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        assert np.array_equal(t.sum(0), Xh.astype(np.float64))


# ---- (d), (e): the Gram planes pass --------------------------------------------------------------------------------------------------------
KIND_ID = {'rbf': 0, 'matern12': 1, 'matern32': 2, 'matern52': 3}
VAR = 1.3
f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(f32(a))).cuda()


def _gram_planes(kind, Xmin, Xmaj, ls, ard, w=None, majs=None, mins=None, period=1, var=VAR):
    """mxf_gram_planes on float32 copies of the arguments, planes and U in pre-filled guarded buffers.  Returns (planes int16, U or None)."""
    lib, h, st = _ctx()
    (R, Q), Kn = np.shape(Xmin), np.shape(Xmaj)[0]
    n = 2 * P.plane_elems(R, Kn)
    assert n == 2 * lib.load().mxf_f32x3_plane_elems(R, Kn)
    buf = _guarded16(n)
    t = [dev(a) for a in (Xmin, Xmaj, ls, [var], w, majs, mins)]
    Pw = 0 if w is None else np.shape(w)[1]
    ubuf = None if w is None else torch.full((Pw * R + GUARD,), SENT32, dtype=torch.float32, device='cuda')
    ptr = lambda x: None if x is None else x.data_ptr()
    lib.call('mxf_gram_planes', h, KIND_ID[kind], R, Kn, Q, ptr(t[0]), ptr(t[1]), ptr(t[2]), int(bool(ard)), ptr(t[3]), buf.data_ptr(),
             ptr(t[4]), Pw, ptr(ubuf), R, ptr(t[5]), ptr(t[6]), int(period), st)
    planes = _take(buf, n, 'gram planes')
    U = None if w is None else _take(ubuf, Pw * R, 'U').reshape(Pw, R).astype(np.float64)
    return planes, U


def _inputs(seed, R, Kn, Q, ard, shift=0.0):
    """X uniform on [-2, 2] (+ shift), ls in [0.8, 1.8] sqrt(Q), all rounded to float32 and returned as float64"""
    rng = np.random.RandomState(seed)
    Xmin = f32(shift + rng.uniform(-2, 2, (R, Q))).astype(np.float64)
    Xmaj = f32(shift + rng.uniform(-2, 2, (Kn, Q))).astype(np.float64)
    ls = f32(rng.uniform(0.8, 1.8, Q if ard else 1) * np.sqrt(Q)).astype(np.float64)
    return Xmin, Xmaj, ls


def _dense(planes, R, Kn, var=VAR):
    """(dense float64 (R, Kn), hi, lo as float64 incl. the k padding)"""
    d = P.decode(planes, R, Kn, 2).view(np.float16).astype(np.float64)
    return (d[0] + d[1])[:, :Kn] * (float(np.float32(var)) / 2.0 ** 14), d[0], d[1]


def _structure(planes, R, Kn, what):
    """the exact properties of every Gram planes buffer: zero k padding; finite, non-negative; lo a residual of hi (|lo| <= ulp(hi) / 2 --
    swapped planes, a lo from the wrong lane after the half-wave exchange, or a lo that is not a residual all break it)"""
    _assert_padding_zero(planes, R, Kn, 2, what)
    _, hi, lo = _dense(planes, R, Kn)
    assert np.isfinite(hi).all() and np.isfinite(lo).all() and (hi >= 0).all() and (hi <= 2.0 ** 14).all(), what
    bad = np.abs(lo) > P.f16_ulp(hi) / 2
    assert not bad.any(), '%s: |lo| > ulp(hi) / 2 at (r, k) = %s' % (what, tuple(np.argwhere(bad)[0]))


def _ratio(dense, ref, var=VAR):
    """worst |dense - ref| / (1e-5 |ref| + 1e-5 var): the bar of test_gram_shapes_vs_oracle for a float32 Gram, <= 1 passes"""
    return float((np.abs(dense - ref) / (1e-5 * np.abs(ref) + 1e-5 * float(np.float32(var)))).max())


# every listed R, Kn, Q and kind at least once; ARD and isotropic
GRID = [('rbf', 1, 1, 1, False), ('matern12', 40, 15, 3, True), ('matern32', 63, 16, 8, False), ('matern52', 64, 17, 9, True),
        ('rbf', 65, 130, 16, True), ('matern32', 130, 300, 3, False), ('rbf', 130, 17, 9, False), ('matern12', 65, 300, 16, True),
        ('matern52', 40, 130, 1, True), ('rbf', 100, 300, 8, True), ('matern12', 63, 1, 9, False), ('matern52', 1, 300, 8, False)]


@pytest.mark.parametrize('kind,R,Kn,Q,ard', GRID)
def test_gram_planes_values_and_structure(kind, R, Kn, Q, ard):
    """dense = (hi + lo) var / 2^14 against the float64 Gram of the same float32-rounded inputs at rtol = 1e-5, atol = 1e-5 var -- the bar of
    test_gram_shapes_vs_oracle for the float32 mxf_gram, whose own worst ratio on the same inputs is printed next to it.  With X on [-2, 2]
    and ls >= 0.8 sqrt(Q), r^2 <= 25: every covariance is >= e^-12.5 var, every scaled hi a normal f16, no element is excluded.
    Worst observed error as a fraction of that bar over this grid on an MI355X, planes (float32 mxf_gram on the same inputs): rbf 0.010
    (0.010), matern12 0.0074 (0.0067), matern32 0.013 (0.013), matern52 0.016 (0.015) -- the planes carry 22 bits of a float32 covariance
    and sit where mxf_gram sits, errors of 1e-7 var; a dropped lo term (2^-11 relative) is 30 times over the bar."""
    from mxfusion_amd import ops
    Xmin, Xmaj, ls = _inputs(R * 1000 + Kn + Q, R, Kn, Q, ard)
    ref = P.gram64(kind, Xmin, Xmaj, ls, [VAR])
    assert ref.min() * 2.0 ** 14 / VAR >= 2.0 ** -14
    planes, _ = _gram_planes(kind, Xmin, Xmaj, ls, ard)
    _structure(planes, R, Kn, kind)
    dense, hi, _ = _dense(planes, R, Kn)
    assert (hi[:, :Kn] >= 2.0 ** -14).all()
    K32 = ops.gram(kind, dev(Xmin)[None], dev(Xmaj)[None], dev(ls)[None], dev([[VAR]]), ard)[0].double().cpu().numpy()
    print('gram planes %s R=%d Kn=%d Q=%d: ratio %.4f (float32 mxf_gram: %.4f)' % (kind, R, Kn, Q, _ratio(dense, ref), _ratio(K32, ref)))
    assert np.allclose(dense, ref, rtol=1e-5, atol=1e-5 * VAR), _ratio(dense, ref)
    # ops.gram_planes is the same call
    got = ops.gram_planes(kind, dev(Xmin), dev(Xmaj), dev(ls), dev([VAR]), ard)
    assert got.dtype == torch.int16 and torch.equal(got.cpu(), torch.from_numpy(planes.copy()))


def test_gram_planes_coincident_points_are_exact_under_rbf():
    """A row of Xmin equal to a row of Xmaj under RBF: the squared distance is a sum of exact zeros, exp2(-0) is exactly 1 on the hardware
    exponential (cov_from<RBF>(0, 16384) = 16384 * v_exp_f32(-0)), so hi = 2^14 and lo = +0, bit for bit -- on both stores, the ragged row
    tail and the ragged k block."""
    R, Kn, Q = 100, 50, 3
    Xmin, Xmaj, ls = _inputs(11, R, Kn, Q, True)
    pairs = [(5, 0), (37, 17), (99, 49), (64, 15), (31, 48)]
    for r, k in pairs:
        Xmin[r] = Xmaj[k]
    planes, _ = _gram_planes('rbf', Xmin, Xmaj, ls, True)
    _structure(planes, R, Kn, 'coincident')
    d = P.decode(planes, R, Kn, 2)
    for r, k in pairs:
        got = (int(d[0][r, k]) & 0xffff, int(d[1][r, k]) & 0xffff)
        assert got == (0x7400, 0), (r, k, hex(got[0]), hex(got[1]))          # 0x7400: 2^14 in f16
    assert (d[0].view(np.float16) == np.float16(2.0 ** 14)).sum() == len(pairs)


@pytest.mark.parametrize('which,index', [('row', 5), ('row', 37), ('row', 99), ('col', 5), ('col', 37), ('col', 49)])
def test_gram_planes_placement_of_one_far_point(which, index):
    """One row of Xmin (R = 100: the first store, the second store, the last row of the ragged tail) or one column of Xmaj (Kn = 50: a full
    k block, another, the ragged one) shifted by 50 while everything else stays on [-2, 2]: exactly that row / column of dense is below
    1e-6 var (the others are >= e^-12.5 var = 3.7e-6 var)."""
    R, Kn, Q = 100, 50, 3
    Xmin, Xmaj, ls = _inputs(12, R, Kn, Q, False)
    (Xmin if which == 'row' else Xmaj)[index] += 50.0
    planes, _ = _gram_planes('rbf', Xmin, Xmaj, ls, False)
    _structure(planes, R, Kn, 'placement')
    dense, _, _ = _dense(planes, R, Kn)
    small = dense < 1e-6 * VAR
    want = np.zeros((R, Kn), bool)
    if which == 'row':
        want[index, :] = True
    else:
        want[:, index] = True
    assert np.array_equal(small, want), (np.argwhere(small != want)[:5])
    ref = P.gram64('rbf', f32(Xmin), f32(Xmaj), ls, [VAR])
    assert np.allclose(dense, ref, rtol=1e-5, atol=1e-5 * VAR)


def test_gram_planes_far_field_underflows_cleanly():
    """ls = 0.05: most RBF covariances underflow (f16 denormals of the scaled value, then zero).  Planes finite and >= 0, absolute error
    <= 1e-5 var."""
    R, Kn, Q = 65, 50, 3
    Xmin, Xmaj, _ = _inputs(13, R, Kn, Q, False)
    Xmin[:8] = Xmaj[:8] + f32(np.random.RandomState(1).uniform(-0.05, 0.05, (8, Q)))       # a few near pairs that do carry covariance
    Xmin = f32(Xmin).astype(np.float64)
    ls = f32([0.05]).astype(np.float64)
    ref = P.gram64('rbf', Xmin, Xmaj, ls, [VAR])
    assert (ref < 1e-30).mean() > 0.5 and ref.max() > 0.1
    planes, _ = _gram_planes('rbf', Xmin, Xmaj, ls, False)
    _structure(planes, R, Kn, 'far field')
    dense, hi, lo = _dense(planes, R, Kn)
    assert (dense >= 0).all() and np.abs(dense - ref).max() <= 1e-5 * VAR, np.abs(dense - ref).max()


@pytest.mark.parametrize('kind', ['rbf', 'matern12', 'matern32', 'matern52'])
def test_gram_planes_do_not_depend_on_where_the_inputs_sit(kind):
    """All inputs shifted by 1e4: the distances are formed difference first (exact in float32 for neighbours at that offset), so the bound
    of the centred case holds.  The reference is the float64 Gram of the CENTRED float32-rounded inputs (X - 1e4 is exact in float64)."""
    R, Kn, Q, off = 70, 45, 5, 1.0e4
    Xmin, Xmaj, ls = _inputs(14, R, Kn, Q, True, shift=off)
    ref = P.gram64(kind, Xmin - off, Xmaj - off, ls, [VAR])
    planes, _ = _gram_planes(kind, Xmin, Xmaj, ls, True)
    _structure(planes, R, Kn, 'offset')
    dense, _, _ = _dense(planes, R, Kn)
    print('gram planes at offset 1e4, %s: ratio %.4f' % (kind, _ratio(dense, ref)))
    assert np.allclose(dense, ref, rtol=1e-5, atol=1e-5 * VAR), _ratio(dense, ref)


def _check_U(U, w, ref, dense, Kn, what):
    """U (Pw, R) against float64 w^T cov (the in-order fmaf chain's recursive-summation bound + the element bound of the covariances) and
    against the kernel's own planes (f32 accumulation + the 2^-22 representation only)"""
    w = f32(w).astype(np.float64)
    absum = np.abs(w).T @ np.abs(ref).T                         # (Pw, R): sum_k |w||cov|
    e1 = np.abs(U - w.T @ ref.T) / absum
    e2 = np.abs(U - w.T @ dense.T) / absum
    print('%s: U vs float64 %.3g of sum|w||cov| (bar %.3g), vs its own planes %.3g (bar %.3g)'
          % (what, e1.max(), Kn * 2.0 ** -24 + 1e-5, e2.max(), (Kn + 4) * 2.0 ** -24))
    assert (e1 <= Kn * 2.0 ** -24 + 1e-5).all(), (what, float(e1.max()))
    assert (e2 <= (Kn + 4) * 2.0 ** -24).all(), (what, float(e2.max()))


@pytest.mark.parametrize('Pw', [1, 3, 8])
@pytest.mark.parametrize('kind,R,Kn,Q', [('rbf', 40, 17, 3), ('matern32', 130, 300, 9), ('matern52', 130, 17, 8), ('matern12', 40, 300, 16)])
def test_gram_planes_fused_row(kind, R, Kn, Q, Pw):
    """U[p][r] = sum_k w[k][p] cov(r, k) from the same pass (PT = 1 for Pw = 1, PT = 8 otherwise; grid.y = 1 instead of the k-block slices),
    and the planes written next to it bit-equal to those written without w."""
    from mxfusion_amd import ops
    Xmin, Xmaj, ls = _inputs(R + Kn + Q + Pw, R, Kn, Q, Q % 2 == 1)
    w = f32(np.random.RandomState(Pw).randn(Kn, Pw))
    ref = P.gram64(kind, Xmin, Xmaj, ls, [VAR])
    plain, _ = _gram_planes(kind, Xmin, Xmaj, ls, Q % 2 == 1)
    planes, U = _gram_planes(kind, Xmin, Xmaj, ls, Q % 2 == 1, w=w)
    assert torch.equal(torch.from_numpy(planes.copy()), torch.from_numpy(plain.copy()))
    _structure(planes, R, Kn, 'fused row')
    dense, _, _ = _dense(planes, R, Kn)
    assert np.allclose(dense, ref, rtol=1e-5, atol=1e-5 * VAR)
    _check_U(U, w, ref, dense, Kn, '%s R=%d Kn=%d Pw=%d' % (kind, R, Kn, Pw))
    p2, U2 = ops.gram_planes(kind, dev(Xmin), dev(Xmaj), dev(ls), dev([VAR]), Q % 2 == 1, w=dev(w))
    assert torch.equal(p2.cpu(), torch.from_numpy(planes.copy())) and U2.shape == (Pw, R) and np.array_equal(U2.double().cpu().numpy(), U)


@pytest.mark.parametrize('mode', ['majs', 'mins', 'both'])
@pytest.mark.parametrize('period', [7, 'Kn', 1])
@pytest.mark.parametrize('kind,R,Kn,Q', [('rbf', 40, 17, 3), ('matern52', 130, 300, 9)])
def test_gram_planes_row_weights(kind, R, Kn, Q, period, mode):
    """majs alone, mins alone and both, weights on [0.2, 1]: the planes of K diag(majs[k % period]), diag(mins[r % period]) K and both, with
    period 7 (divides neither R nor Kn), Kn and 1; U from the weighted covariances.  The bounds of the unweighted tests."""
    period = Kn if period == 'Kn' else period
    rng = np.random.RandomState(period + R)
    Xmin, Xmaj, ls = _inputs(R + Kn + period, R, Kn, Q, True)
    majs = f32(rng.uniform(0.2, 1, period)) if mode in ('majs', 'both') else None
    mins = f32(rng.uniform(0.2, 1, period)) if mode in ('mins', 'both') else None
    w = f32(rng.randn(Kn, 3))
    ref = P.gram64(kind, Xmin, Xmaj, ls, [VAR], majs=majs, mins=mins, period=period)
    plain = P.gram64(kind, Xmin, Xmaj, ls, [VAR])
    if period > 1:
        assert np.abs(ref - plain).max() > 0.05 * VAR            # the weights matter at the bound's scale
    planes, U = _gram_planes(kind, Xmin, Xmaj, ls, True, w=w, majs=majs, mins=mins, period=period)
    noU, _ = _gram_planes(kind, Xmin, Xmaj, ls, True, majs=majs, mins=mins, period=period)
    assert torch.equal(torch.from_numpy(planes.copy()), torch.from_numpy(noU.copy()))
    _structure(planes, R, Kn, 'weights')
    dense, _, _ = _dense(planes, R, Kn)
    assert np.allclose(dense, ref, rtol=1e-5, atol=1e-5 * VAR), _ratio(dense, ref)
    _check_U(U, w, ref, dense, Kn, '%s %s period=%d' % (kind, mode, period))


def test_gram_planes_rejects_bad_arguments():
    """-2 / -3 with a message and nothing written: Q > 16, a non-stationary kind, w with Pw > 8, period < 1, a null pointer."""
    from mxfusion_amd import _lib, ops
    lib, h, st = _ctx()
    R, Kn = 10, 20
    X, Z, ls, var = (torch.rand(R, 17, device='cuda'), torch.rand(Kn, 17, device='cuda'), torch.ones(1, device='cuda'), torch.ones(1, device='cuda'))
    buf = _guarded16(2 * P.plane_elems(R, Kn))
    U = torch.full((9 * R,), SENT32, dtype=torch.float32, device='cuda')
    w = torch.rand(Kn, 9, device='cuda')

    def rc(kind=0, Q=3, Xp=X.data_ptr(), planes=buf.data_ptr(), wp=None, Pw=0, Up=None, period=1, lsp=ls.data_ptr()):
        return lib.load().mxf_gram_planes(h, kind, R, Kn, Q, Xp, Z.data_ptr(), lsp, 0, var.data_ptr(), planes, wp, Pw, Up, R, None, None, period, st)

    assert rc() == 0
    buf.fill_(SENT16)
    assert rc(Q=17) == -3 and b'Q' in lib.load().mxf_last_error(h)
    for kind in (4, 5, 6, 7, -1):                         # linear, bias, white, unknown
        assert rc(kind=kind) == -2, kind
    assert b'stationary' in lib.load().mxf_last_error(h)
    assert rc(wp=w.data_ptr(), Pw=9, Up=U.data_ptr()) == -3 and b'Pw' in lib.load().mxf_last_error(h)
    assert rc(wp=w.data_ptr(), Pw=0, Up=U.data_ptr()) == -3
    assert rc(wp=w.data_ptr(), Pw=3, Up=None) == -2          # w without U
    assert rc(period=0) == -2 and rc(period=-3) == -2
    assert b'period' in lib.load().mxf_last_error(h)
    assert rc(Xp=None) == -2 and rc(planes=None) == -2 and rc(lsp=None) == -2
    assert b'null' in lib.load().mxf_last_error(h)
    assert rc(Q=0) == -2
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENT16).all() and (U.cpu().numpy() == np.float32(SENT32)).all()
    with pytest.raises(_lib.MXFError):
        ops.gram_planes('rbf', X[:, :3], Z[:, :3], ls, var, False, w=w)
    with pytest.raises(_lib.MXFError):
        ops.gram_planes('linear', X[:, :3], Z[:, :3], ls, var, False)
    with pytest.raises(_lib.MXFError):
        ops.gram_planes('rbf', X, Z, ls, var, False)
