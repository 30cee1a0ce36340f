"""mxf_gram_bwd (csrc/gram_bwd.hip) through the C ABI with the test's own buffers, on everything its interface promises: every operand
shared by the samples (stride 0) or sampled, outputs accumulated into, any output pointer null, coincident points, and a workgroup that
walks several column tiles.  Referee: the difference-form closed-form gradient of tests/_gram_ref.py in extended precision (float64 runs)
or float64 (float32 runs; the inputs are rounded to float32 first), which tests/test_gram_ref_host.py checks on the CPU.

The bar is per element and relative to the sum of the absolute values of the element's terms:

    |got - ref| <= C[dtype] * u * abs_sum,        u = 2^-53 (float64), 2^-24 (float32)

No element is excluded.  C (_gram_ref.BAR_C) is 4x the worst ratio measured over this whole file on an MI355X, rounded up to a power of two (the
margin is for the order of the atomic adds and for other inputs).  Measured worst ratios |got - ref| / (u abs_sum):

    float64   2700   (C = 2^14)      both on the same element: test_sample_axes[matern12-64-1-5-ard-XSZ1lSvS], dX
    float32   1690   (C = 2^13)

Why thousands and not tens: with N2 = 1 an element of dX is ONE term, W d_q / l_q, so abs_sum is that term's size and the ratio is the relative
error of d_q itself.  The kernel forms d_q as the difference of two scaled coordinates, (x - c) / l and (z - c) / l, rounded separately (that is
what makes the inner loop one subtraction per coordinate): an absolute error of ~1.5 u (|x - c| + |z - c|) / l, i.e. ~1.5 (|x - c| + |z - c|) /
|x - z| roundoffs of the term -- thousands for the closest of the 64 x 5 x 3 coordinate pairs of that case.  A numpy emulation of exactly this
arithmetic (everything else in the working precision, pairwise sums) gives 2700 and 1690 on the same element, so nothing else hides in the figure.
Away from the single-term shapes (N2 = 1: dX, N = 1: dX2) the worst measured ratios are 71 (float64) and 101 (float32), both on dX2 with one row
band of 63 / 64 rows; dls and dvar stay below 8 everywhere.

Every test prints its worst ratio per output (pytest -s) before it asserts."""
import functools

import numpy as np
import pytest
import torch

import _gram_ref as R
import _strided as st

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
U = {F64: 2.0 ** -53, F32: 2.0 ** -24}
C = {F64: R.BAR_C['f64'], F32: R.BAR_C['f32']}
NAMES = ('dX', 'dX2', 'dls', 'dvar')
S = 3

NS = (1, 63, 64, 65, 130)               # the row tile is 64; 130: more than one row band once the small-grid split has cut the bands to 64 rows
N2S = (1, 255, 256, 257, 600)           # the column tile is 256
QS = (1, 2, 3, 4, 5, 8, 9, 16, 17)      # register-tile buckets 2 / 4 / 8 / 16; 17: the generic kernel, here with S > 1


def _hi(dtype):
    return R.HI if dtype == F64 else np.float64


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype).cuda()


@functools.lru_cache(maxsize=None)
def _reference(kind, seed, N, N2, Q, ard, pattern, f32, special=None):
    """(operands, grad, scale) of one case, computed once and shared by the tests that use the same case; never modified"""
    ops = R.make_case(seed, N, N2, Q, ard, pattern, S=S, f32=f32)
    if special is not None:
        ops = _coincident(ops, f32)
    X, X2, ls, var, dK = ops
    grad, scale = R.gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=np.float64 if f32 else R.HI)
    return ops, grad, scale


def _call(kind, ops, ard, dtype, out=None, need=NAMES):
    X, X2, ls, var, dK = ops
    d = [_dev(a, dtype) for a in (X, X2, ls, var)]
    if out is None:
        out = tuple(None if (p is None or n not in need) else torch.zeros_like(p) for n, p in zip(NAMES, d))
    st.gram_bwd(R.KIND_ID[kind], d[0], d[1], d[2], d[3], ard, _dev(dK, dtype), out=out)
    torch.cuda.synchronize()
    return dict(zip(NAMES, out))


def _check(got, grad, scale, dtype, what, extra=None, factor=1.0):
    """every output present in `got` against factor * grad (+ extra), per element, relative to factor * scale (+ |extra|)"""
    worst = {}
    for n in NAMES:
        if grad[n] is None or got.get(n) is None:
            continue
        ref, sc = grad[n] * factor, scale[n] * factor
        if extra is not None:
            ref, sc = ref + extra[n], sc + np.abs(extra[n])
        worst[n] = R.worst_ratio(got[n].cpu().numpy(), ref, sc, U[dtype])
    print('RATIO %s %s %s' % ('f64' if dtype == F64 else 'f32', what, ' '.join('%s=%.3g' % kv for kv in worst.items())))
    bad = {n: w for n, w in worst.items() if not w <= C[dtype]}
    assert not bad, '%s: |got - ref| / (u abs_sum) = %r > %g' % (what, bad, C[dtype])
    return worst


# ---- the sample-axis matrix -----------------------------------------------------------------------------------------------------------------
def _matrix(ki):
    """24 cases per kind: each of the 16 rectangular and 8 square sample-axis patterns once, walking N, N2, Q and ARD / isotropic so that every
    value of NS, N2S and QS occurs for every kind (the walk is shifted by the kind's index: more (N, N2, Q) combinations over the four kinds)"""
    cases = []
    for i, p in enumerate(R.RECT_PATTERNS):
        cases.append((NS[(i + ki) % 5], N2S[(i + i // 5 + 2 * ki) % 5], QS[(i + 2 * ki) % 9], (i + i // 2) % 2 == 0, p))
    for i, p in enumerate(R.SQUARE_PATTERNS):
        cases.append((NS[(i + 1 + ki) % 5], None, QS[(i + 7 + 3 * ki) % 9], (i + ki) % 2 == 0, p))
    return cases


MATRIX = [(kind,) + c for ki, kind in enumerate(R.KINDS) for c in _matrix(ki)]


def test_matrix_is_complete():
    for kind in R.KINDS:
        mine = [c[1:] for c in MATRIX if c[0] == kind]
        assert {c[4] for c in mine} == set(R.RECT_PATTERNS + R.SQUARE_PATTERNS)
        assert {c[0] for c in mine} == set(NS) and {c[1] for c in mine} == set(N2S) | {None} and {c[2] for c in mine} == set(QS)
        assert {c[3] for c in mine} == {True, False}


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('kind,N,N2,Q,ard,pattern', MATRIX,
                         ids=['%s-%d-%s-%d-%s-%s' % (k, n, n2, q, 'ard' if a else 'iso', R.pattern_id(p)) for k, n, n2, q, a, p in MATRIX])
def test_sample_axes(kind, N, N2, Q, ard, pattern, dtype):
    ops, grad, scale = _reference(kind, 100 + N + Q, N, N2, Q, ard, pattern, dtype == F32)
    got = _call(kind, ops, ard, dtype)
    assert (got['dX2'] is None) == (N2 is None)
    _check(got, grad, scale, dtype, 'axes %s N%d N2%s Q%d %s %s' % (kind, N, N2, Q, 'ard' if ard else 'iso', R.pattern_id(pattern)))


# ---- output subsets and accumulate-into -----------------------------------------------------------------------------------------------------
# rectangular: one row band, two column tiles, X2 sampled -- dX2 is the plain (non-atomic) store of the workgroup that owns the column;
# square: two row bands, X shared -- every output goes through atomics
SHAPES = {'rect': (63, 257, 3, True, (True, True, False, False)), 'square': (65, None, 5, False, (False, None, True, True))}


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('kind', R.KINDS)
def test_output_subsets(kind, shape, dtype):
    """every non-empty subset of the outputs: a present output equals its value from the all-outputs call -- bit for bit where one workgroup
    stores it without atomics (dX2 of the rectangular shape), within the bar elsewhere (the order of the atomic adds varies) -- and the
    reference; a null output is simply absent"""
    N, N2, Q, ard, pattern = SHAPES[shape]
    ops, grad, scale = _reference(kind, 7, N, N2, Q, ard, pattern, dtype == F32)
    present = [n for n in NAMES if grad[n] is not None]
    full = _call(kind, ops, ard, dtype)
    _check(full, grad, scale, dtype, 'subsets %s %s all' % (kind, shape))
    worst = 0.0
    for mask in range(1, 2 ** len(present) - 1):
        need = tuple(n for i, n in enumerate(present) if mask >> i & 1)
        got = _call(kind, ops, ard, dtype, need=need)
        for n in present:
            if n not in need:
                assert got[n] is None
                continue
            if n == 'dX2':
                assert torch.equal(got[n], full[n]), (need, n)
            g, f = got[n].cpu().numpy(), full[n].cpu().numpy()
            worst = max(worst, R.worst_ratio(g, f.astype(grad[n].dtype), scale[n], U[dtype]),
                        R.worst_ratio(g, grad[n], scale[n], U[dtype]))
    print('RATIO %s subsets %s %s worst=%.3g' % ('f64' if dtype == F64 else 'f32', kind, shape, worst))
    assert worst <= C[dtype], worst


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('kind', R.KINDS)
def test_accumulates_into_outputs(kind, shape, dtype):
    """buffers holding C0 come back as C0 + grad, and as C0 + 2 grad after a second call; the scale gains |C0| (one more addend)"""
    N, N2, Q, ard, pattern = SHAPES[shape]
    ops, grad, scale = _reference(kind, 7, N, N2, Q, ard, pattern, dtype == F32)
    rng = np.random.RandomState(5)
    c0 = {n: None if grad[n] is None else rng.randn(*grad[n].shape) * 3 for n in NAMES}
    out = tuple(_dev(c0[n], dtype) for n in NAMES)
    c0 = {n: None if o is None else o.cpu().numpy().astype(_hi(dtype)) for n, o in zip(NAMES, out)}       # (as rounded to dtype)
    for calls in (1, 2):
        got = _call(kind, ops, ard, dtype, out=out)
        _check(got, grad, scale, dtype, 'accumulate %s %s x%d' % (kind, shape, calls), extra=c0, factor=float(calls))


# ---- coincident points ----------------------------------------------------------------------------------------------------------------------
def _coincident(ops, f32):
    """exact duplicates inside X; rectangular: the first 40 rows of X2 are rows of X (Z = X[:M]).  float64 only: a few more rows lie INSIDE the
    Matern clip radius of another row without coinciding with it (offsets <= 3e-9, r2 < 1e-16 << 1e-14) -- the only pairs on which the clipped
    slopes are multiplied by a non-zero distance (Matern52: +5/3 e); in float32 such offsets are below the spacing of the inputs."""
    X, X2, ls, var, dK = ops
    X = X.copy()
    N = X.shape[1]
    rng = np.random.RandomState(9)
    X[:, N - 6:] = X[:, :6]
    if X2 is None:
        if not f32:
            X[:, N - 12:N - 6] = X[:, 10:16] + rng.uniform(-3e-9, 3e-9, X[:, 10:16].shape)
    else:
        assert X2.shape[0] == X.shape[0], 'X2 rows are copies of X rows: same sample extent'
        X2 = X2.copy()
        X2[:, :40] = X[:, :40]
        if not f32:
            X2[:, 40:50] = X[:, 40:50] + rng.uniform(-3e-9, 3e-9, X[:, 40:50].shape)
    return X, X2, ls, var, dK


COINCIDENT = [(70, 300, 1, True, (False, False, True, True)), (70, 300, 3, False, (True, True, False, False)),
              (70, None, 2, True, (True, None, True, False)), (66, 60, 17, True, (False, False, False, True))]


@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('N,N2,Q,ard,pattern', COINCIDENT, ids=['rect-Q1', 'rect-Q3', 'square-Q2', 'rect-Q17'])
@pytest.mark.parametrize('kind', R.KINDS)
def test_coincident_points(kind, N, N2, Q, ard, pattern, dtype):
    """all four gradients are held to the reference where distances are exactly zero (Matern12 sits on its kink there: the clip convention's
    slope, 0, defines the expected value) or inside the clip radius"""
    ops, grad, scale = _reference(kind, 31, N, N2, Q, ard, pattern, dtype == F32, special='coincident')
    X, X2 = ops[0], ops[1]
    assert (X[:, :6] == X[:, N - 6:]).all() and (X2 is None or (X2[:, :40] == X[:, :40]).all())
    got = _call(kind, ops, ard, dtype)
    _check(got, grad, scale, dtype, 'coincident %s N%d N2%s Q%d %s' % (kind, N, N2, Q, R.pattern_id(pattern)))


# ---- several column tiles per workgroup ---------------------------------------------------------------------------------------------------
# gram_bwd_plan (gram_bwd_plan.h) gives a workgroup CT = ceil(tiles * row bands * S / 4096) column tiles of 256: 243 tiles x 1 band x 17 samples = 4131
# -> CT = 2, and 243 is odd: the last workgroup of each sample meets tile0 >= N2 and stops early.  dK is 17 x 64 x 61957 float32 = 270 MB.
CT_S, CT_N, CT_N2, CT_Q = 17, 64, 242 * 256 + 5, 2


@functools.lru_cache(maxsize=None)
def _ct_operands():
    rng = np.random.default_rng(12)
    X = rng.uniform(-2, 2, (1, CT_N, CT_Q)).astype(np.float32)              # shared X: the row-side atomics of 17 samples meet in one dX
    X2 = rng.uniform(-2, 2, (CT_S, CT_N2, CT_Q)).astype(np.float32)        # sampled X2: the plain store, once per column tile of the walk
    ls = rng.uniform(0.8, 1.8, (CT_S, CT_Q)).astype(np.float32)
    var = rng.uniform(0.5, 1.5, (1, 1)).astype(np.float32)
    dK = rng.standard_normal((CT_S, CT_N, CT_N2), dtype=np.float32)
    return (X, X2, ls, var, dK), tuple(torch.from_numpy(a).cuda() for a in (X, X2, ls, var, dK))


def _ct_reference(kind, host):
    """float64, one sample per call of the reference ((N, N2) temporaries of 32 MB), four samples at a time on threads; X and var are shared:
    their gradients and scales are the sums over the samples"""
    from concurrent.futures import ThreadPoolExecutor
    X, X2, ls, var, dK = host
    with ThreadPoolExecutor(4) as pool:
        parts = list(pool.map(lambda s: R.gram_bwd_ref(kind, X, X2[s:s + 1], ls[s:s + 1], var, dK[s:s + 1], dtype=np.float64), range(CT_S)))
    join = lambda i, n: np.concatenate([p[i][n] for p in parts]) if n in ('dX2', 'dls') else sum(p[i][n] for p in parts)
    return {n: join(0, n) for n in NAMES}, {n: join(1, n) for n in NAMES}


@pytest.mark.parametrize('kind', ['rbf', 'matern52'])
def test_several_column_tiles_per_workgroup(kind):
    assert -(-(-(-CT_N2 // 256) * 1 * CT_S) // 4096) == 2 and -(-CT_N2 // 256) % 2 == 1, 'the shape no longer gives CT = 2 with an odd tile count'
    host, dev = _ct_operands()
    grad, scale = _ct_reference(kind, host)
    out = tuple(torch.zeros_like(t) for t in dev[:4])
    st.gram_bwd(R.KIND_ID[kind], dev[0], dev[1], dev[2], dev[3], True, dev[4], out=out)
    torch.cuda.synchronize()
    _check(dict(zip(NAMES, out)), grad, scale, F32, 'CT2 %s' % kind)
