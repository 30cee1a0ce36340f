"""mxf_kmv_wide and mxf_kmv_wide_bwd on the GPU through ops.kernel_matvec / ops.kernel_matvec_bwd_ at Q > 16, in both dtypes:
    out[s, n, j] = sum_n2 k(X[s, n], X2[s, n2]) V[s, n2, j] (+ diag_add[s] V[s, n, j], square)   against _gram_ref.gram_ref(...) @ V,
    dls, dvar of sum_j w_j A[:, j]^T K V[:, j]                                                    against _gram_ref.gram_bwd_ref on the
cotangent dK = sum_j w_j A[:, j] V[:, j]^T written out; both in float64 numpy.

Sizes of csrc/kmv_wide.hip that the shapes are chosen from: a workgroup owns a band of 64 rows and walks tiles of 64 columns, a lane 4 x 4
pairs; a chunk is 16 (float32) / 8 (float64) coordinates, or columns of A and V in the reverse mode; a forward pass serves JB = 4 columns of
V for J <= 4 and 16 (float32) / 8 (float64) above, so J in {1, 5, 8, 9, 16, 17, 33} holds JB, JB + 1 and 2 JB + 1 of either dtype; n2 is
split over min(ceil(512 / (ceil(N / 64) * S)), ceil(N2 / 64)) workgroup rows that add into doubles.  So N in {1, 63, 65, 130} x N2 in
{1, 63, 65, 200} at Q = 17 (N2 <= 64 is written by the lanes themselves, every larger N2 there is split into single tiles), Q in {17, 24, 33,
100} at 65 x 65, the four kinds with and without ARD on the square product with diag_add, S = 2 with all and with some operands per sample,
70 x 5 000 (79 workgroup rows), 20 000 x 3 (313 bands, no split) and 16 400 x 130 (257 bands: two workgroup rows, the first of two tiles).

Operands as tests/test_gpu_kmv.py, but lengthscale in [0.8, 1.8] sqrt(Q / 3) so that r2 keeps the magnitude of its Q = 3 cases.  Bars, that
file's: float64 rtol 1e-9 / atol 1e-11, float32 rtol 1e-4 / atol 1e-5, relative to the sum of the magnitudes of an element's terms; the
reference of a float32 run sees the rounded operands.  Every test prints the worst ratio of an error to its bar."""
import functools

import numpy as np
import pytest
import torch

import _gram_ref as GR

pytestmark = pytest.mark.gpu

BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
ALL, GUARD = frozenset(('X', 'X2', 'ls', 'var', 'V', 'A', 'diag')), 64

#         kind, ard, N, N2 (None: square, with diag_add), Q, J, S, operands that own a sample axis
CASES = [('rbf', True, n, n2, 17, 5, 1, ALL) for n in (1, 63, 65, 130) for n2 in (1, 63, 65, 200)]
CASES += [(k, True, 65, 65, q, 9, 1, ALL) for q, k in ((17, 'matern12'), (24, 'matern32'), (33, 'matern52'), (100, 'rbf'))]
CASES += [('rbf', False, 65, 65, 17, j, 1, ALL) for j in (1, 8, 9, 16, 17, 33)]
CASES += [(k, ard, 65, None, 20, 5, 1, ALL) for k in GR.KINDS for ard in (True, False)]
CASES += [('rbf', True, 65, 70, 17, 9, 2, ALL), ('rbf', True, 65, 70, 17, 9, 2, frozenset(['ls', 'var', 'V', 'A'])),
          ('matern52', True, 65, 70, 18, 17, 2, frozenset(['X2', 'ls'])), ('matern32', False, 65, None, 17, 5, 2, frozenset(['V', 'A', 'diag']))]
CASES += [('rbf', True, 70, 5000, 20, 5, 1, ALL), ('matern32', False, 20000, 3, 17, 1, 1, ALL), ('matern52', True, 16400, 130, 17, 1, 1, ALL)]
IDS = ['%s-%s-N%d-N2%s-Q%d-J%d-S%d-%s' % (k, 'ard' if a else 'iso', n, n2, q, j, s, 'all' if own == ALL else '+'.join(sorted(own)))
       for k, a, n, n2, q, j, s, own in CASES]


def _inputs(case, rounded=False):
    kind, ard, N, N2, Q, J, S, own = case
    rng = np.random.default_rng(N * 1000003 + (N2 or 0) * 1009 + Q * 31 + S * 7 + 2 * len(own) + 13 * J + GR.KIND_ID[kind])
    ax = lambda name: S if name in own else 1
    M = N if N2 is None else N2
    p = dict(X=rng.uniform(-2, 2, (ax('X'), N, Q)), X2=None if N2 is None else rng.uniform(-2, 2, (ax('X2'), N2, Q)),
             ls=rng.uniform(0.8, 1.8, (ax('ls'), Q if ard else 1)) * np.sqrt(Q / 3.0), var=rng.uniform(0.5, 1.5, (ax('var'), 1)),
             V=rng.standard_normal((ax('V'), M, J)), A=rng.standard_normal((ax('A'), N, J)),
             diag=rng.uniform(0.05, 0.5, (ax('diag'), 1)) if N2 is None else None, w=rng.uniform(-1, 1, J))
    if rounded:
        p = {k: v if v is None or k == 'w' else v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    return p


@functools.lru_cache(maxsize=None)
def _reference(case, rounded):
    kind, ard, N, N2, Q, J, S, own = case
    p = _inputs(case, rounded)
    K = GR.gram_ref(kind, p['X'], p['X2'], p['ls'], p['var'], S=S)
    ref, mag = K @ p['V'], np.abs(K) @ np.abs(p['V'])
    if p['diag'] is not None:
        ref, mag = ref + p['diag'][:, :, None] * p['V'], mag + p['diag'][:, :, None] * np.abs(p['V'])
    bc = lambda a: np.broadcast_to(a, (S,) + a.shape[1:])
    dK = np.einsum('snj,smj,j->snm', bc(p['A']), bc(p['V']), p['w'])
    return ref, mag, GR.gram_bwd_ref(kind, p['X'], p['X2'], p['ls'], p['var'], dK)


def _device(p, dtype):
    return {k: None if v is None else torch.as_tensor(v).to(dtype).cuda().contiguous() for k, v in p.items() if k != 'w'}


def _close(got, ref, mag, dtype, what):
    rtol, atol = BARS[dtype]
    got, ref, mag = got.double().cpu(), torch.as_tensor(ref).double(), torch.as_tensor(mag).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    ratio = float((err / (rtol * mag + atol)).max())
    print('ratio', what, str(dtype)[6:], '%.3g' % ratio, 'max error', float(err.max()), 'max magnitude', float(mag.max()))
    assert ratio <= 1.0, (what, float(err.max()), float(mag.max()), ratio)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_and_reverse(case, dtype):
    from mxfusion_amd import ops
    kind, ard = case[:2]
    ref, mag, (g, sc) = _reference(case, dtype == torch.float32)
    p = _inputs(case)
    d = _device(p, dtype)
    got = ops.kernel_matvec(kind, d['X'], d['X2'], d['ls'], d['var'], ard, d['V'], d['diag'])
    _close(got, ref, mag, dtype, 'forward')
    dls, dvar = torch.ones_like(d['ls']), torch.ones_like(d['var'])          # accumulated into: the terms' magnitudes gain that 1
    ops.kernel_matvec_bwd_(kind, d['X'], d['X2'], d['ls'], d['var'], ard, d['A'], d['V'], list(p['w']), dls, dvar)
    _close(dls, g['dls'] + 1.0, sc['dls'] + 1.0, dtype, 'reverse, lengthscale')
    _close(dvar, g['dvar'] + 1.0, sc['dvar'] + 1.0, dtype, 'reverse, variance')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_the_raw_entry_point_writes_out_and_nothing_else(dtype):
    from mxfusion_amd import _lib, ops
    case = ('matern32', True, 130, 200, 17, 9, 1, ALL)          # two bands, a split, a ragged last pass
    ref, mag, _ = _reference(case, dtype == torch.float32)
    d = _device(_inputs(case), dtype)
    S, N, N2, Q, J, args = ops._kmv_operands('test', case[0], d['X'], d['X2'], d['ls'], d['var'], True, d['V'])
    buf = torch.full((S * N * J + 2 * GUARD,), 7.0, dtype=dtype).cuda()
    out = buf[GUARD:GUARD + S * N * J]
    _lib.call('mxf_kmv_wide', ops._h(d['X']), *args, None, 0, ops._p(d['V']), 0, out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    _close(out.reshape(S, N, J), ref, mag, dtype, 'forward into the guarded buffer')
    assert float((buf[:GUARD] - 7.0).abs().max()) == 0.0 and float((buf[-GUARD:] - 7.0).abs().max()) == 0.0, 'the guard band was written'


def test_status_codes_leave_the_buffers_alone():
    """Q = 16 and Q = 16385 are -3; a null V and J = 0 are -2; nothing is written"""
    from mxfusion_amd import _lib, ops
    mk = lambda *s: torch.ones(*s, dtype=torch.float64).cuda()

    def call(Q=17, J=2, null_V=False, bwd=False):
        X, X2, ls, var, V, A = mk(1, 4, Q), mk(1, 5, Q), mk(1, Q), mk(1, 1), mk(1, 5, max(J, 1)), mk(1, 4, max(J, 1))
        out, out2 = torch.full((1, 4, max(J, 1)), 7.0, dtype=torch.float64).cuda(), torch.full((1, Q), 7.0, dtype=torch.float64).cuda()
        head = [_lib.K_RBF, _lib.F64, 1, 4, 5, Q, J, X.data_ptr(), 0, X2.data_ptr(), 0, ls.data_ptr(), 0, 1, var.data_ptr(), 0]
        v = None if null_V else V.data_ptr()
        try:
            if bwd:
                _lib.call('mxf_kmv_wide_bwd', ops._h(X), *head, A.data_ptr(), 0, v, 0, (_lib._c.c_double * max(J, 1))(*[1.0] * max(J, 1)),
                          out2.data_ptr(), None, ops._stream())
            else:
                _lib.call('mxf_kmv_wide', ops._h(X), *head, None, 0, v, 0, out.data_ptr(), ops._stream())
        finally:
            torch.cuda.synchronize()
            assert float((out - 7.0).abs().max()) == 0.0 and float((out2 - 7.0).abs().max()) == 0.0
    for bwd in (False, True):
        for kw, code in ((dict(Q=16), r'\(-3\)'), (dict(Q=16385), r'\(-3\)'), (dict(null_V=True), r'\(-2\)'), (dict(J=0), r'\(-2\)')):
            with pytest.raises(_lib.MXFError, match=code):
                call(bwd=bwd, **kw)
