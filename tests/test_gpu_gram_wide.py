"""GPU tests of the wide-input Gram passes (mxf_gram_wide / mxf_gram_wide_bwd; csrc/gram_wide.hip), called directly through ops.gram_wide and
ops.gram_wide_bwd, against the difference-form reference tests/_gram_ref.py in _gram_ref.HI on the dtype-rounded operands.

Bars, the project's own: |K - ref| <= tol (max var + |ref|), tol = 1e-11 (float64) / 1e-5 (float32) (TOL_K of tests/test_gpu_gram_icm.py);
gradients worst_ratio(got, ref, abs_sum, u) <= _gram_ref.BAR_C (tests/test_gpu_gram_bwd_axes.py).  Shapes sit at the edges of the 64 x 64 tile
and of the coordinate chunk (16 in float32, 8 in float64).  The length-scales of make_case are multiplied by sqrt(Q / 4): without that r^2
grows like Q and a float32 exp underflows where the reference does not."""
import functools

import numpy as np
import pytest
import torch

import _gram_ref as G

pytestmark = pytest.mark.gpu

TOL_K = {torch.float64: 1e-11, torch.float32: 1e-5}
U = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}
BAR = {torch.float64: G.BAR_C['f64'], torch.float32: G.BAR_C['f32']}
SHAPES = [(1, 1, 17, 1), (7, 5, 33, 1), (70, 130, 20, 2), (130, None, 64, 2), (65, 257, 100, 1), (33, 70, 260, 1)]
DTYPES = pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])


@functools.lru_cache(maxsize=None)
def case(N, N2, Q, S, ard, f32):
    """X and var carry the sample axis, X2 and the length-scale are shared"""
    X, X2, ls, var, dK = G.make_case(N + Q, N, N2, Q, ard, (S > 1, None if N2 is None else False, False, S > 1), S=S, f32=f32)
    ls = ls * np.sqrt(Q / 4.0)
    return X, X2, (ls.astype(np.float32).astype(np.float64) if f32 else ls), var, dK


@functools.lru_cache(maxsize=None)
def reference(kind, N, N2, Q, S, ard, f32):
    X, X2, ls, var, dK = case(N, N2, Q, S, ard, f32)
    return (G.gram_ref(kind, X, X2, ls, var, dtype=G.HI, S=S),) + G.gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=G.HI)


def dev(c, dtype):
    return [None if a is None else torch.as_tensor(a).to(dtype).cuda() for a in c]


def check_K(K, ref, var, dtype, what):
    worst = float((np.abs(K.cpu().numpy().astype(G.HI) - ref) / (TOL_K[dtype] * (float(np.max(var)) + np.abs(ref)))).max())
    print('K', what, 'worst ratio', worst)
    assert worst <= 1.0, (what, worst)


def check_grads(got, grad, scale, dtype, what):
    for name, g in zip(('dX', 'dX2', 'dls', 'dvar'), got):
        if grad[name] is None:
            assert g is None, (what, name)
            continue
        worst = G.worst_ratio(g.cpu().numpy().astype(G.HI), grad[name], scale[name], U[dtype])
        print(name, what, 'worst ratio', worst)
        assert worst <= BAR[dtype], (what, name, worst)


@DTYPES
@pytest.mark.parametrize('kind', G.KINDS)
@pytest.mark.parametrize('N,N2,Q,S', SHAPES)
def test_forward_and_reverse_against_the_reference(N, N2, Q, S, kind, dtype):
    from mxfusion_amd import ops
    f32 = dtype == torch.float32
    for ard in (True, False):
        c = case(N, N2, Q, S, ard, f32)
        X, X2, ls, var, dK = dev(c, dtype)
        Kref, grad, scale = reference(kind, N, N2, Q, S, ard, f32)
        what = (kind, N, N2, Q, S, ard)
        check_K(ops.gram_wide(kind, X, X2, ls, var, ard), Kref, c[3], dtype, what)
        check_grads(ops.gram_wide_bwd(kind, X, X2, ls, var, ard, dK), grad, scale, dtype, what)


@DTYPES
def test_diag_add_and_jitter_land_on_the_square_diagonal(dtype):
    from mxfusion_amd import ops
    N, N2, Q, S = SHAPES[3]
    c = case(N, N2, Q, S, True, dtype == torch.float32)
    X, _, ls, var, _ = dev(c, dtype)
    diag = torch.tensor([[0.25], [0.75]], dtype=dtype, device='cuda')
    K0, K1 = ops.gram_wide('matern52', X, None, ls, var, True), ops.gram_wide('matern52', X, None, ls, var, True, diag_add=diag, jitter=0.125)
    off = ~torch.eye(N, dtype=torch.bool, device='cuda')
    assert torch.equal(K0[:, off], K1[:, off])
    ref = reference('matern52', N, N2, Q, S, True, dtype == torch.float32)[0] + (diag.double().cpu().numpy()[:, :, None] + 0.125) * np.eye(N)
    check_K(K1, ref, c[3], dtype, 'diag')
    Kr = ops.gram_wide('rbf', X, None, ls, var, True)
    assert torch.equal(torch.diagonal(Kr, dim1=-2, dim2=-1), var.expand(S, N))          # coincident rows: r2 = 0 exactly


def test_need_skips_outputs_and_given_buffers_are_accumulated_into():
    from mxfusion_amd import ops
    N, N2, Q, S = SHAPES[2]
    X, X2, ls, var, dK = dev(case(N, N2, Q, S, True, False), torch.float64)
    full = ops.gram_wide_bwd('matern32', X, X2, ls, var, True, dK)
    got = ops.gram_wide_bwd('matern32', X, X2, ls, var, True, dK, need=('X', 'var'))
    assert got[1] is None and got[2] is None and torch.allclose(got[0], full[0], rtol=1e-12, atol=1e-13) and torch.allclose(got[3], full[3], rtol=1e-12)
    into = tuple(torch.full_like(p, 3.0) for p in (X, X2, ls, var))
    acc = ops.gram_wide_bwd('matern32', X, X2, ls, var, True, dK, into=into)
    for a, b, f in zip(acc, into, full):
        assert a is b and torch.allclose(a, f + 3.0, rtol=1e-12, atol=1e-12)
    assert ops.gram_wide_bwd('matern32', X, X2, ls, var, True, dK, need=()) == (None,) * 4


def test_refusals_leave_the_output_untouched():
    from mxfusion_amd import _lib, ops
    one = torch.ones(1, 1, dtype=torch.float64, device='cuda')
    out = torch.full((1, 5, 5), float('nan'), dtype=torch.float64, device='cuda')
    for kind, Q, code in (('rbf', 16, 3), ('linear', 20, 3), ('rbf', _lib.GW_MAX_Q + 1, 3)):
        X = torch.ones(1, 5, Q, dtype=torch.float64, device='cuda')
        with pytest.raises(_lib.MXFError, match=r'\(-%d\): mxf_gram_wide: \w' % code):
            ops.gram_wide(kind, X, None, one, one, False, out=out)
        with pytest.raises(_lib.MXFError, match=r'\(-%d\): mxf_gram_wide_bwd: \w' % code):
            ops.gram_wide_bwd(kind, X, None, one, one, False, torch.ones_like(out))
    with pytest.raises(_lib.MXFError, match=r'\(-2\): mxf_gram_wide: null X'):
        _lib.call('mxf_gram_wide', ops._h(out), 0, 1, 1, 5, 5, 20, None, 0, None, 0, one.data_ptr(), 0, 0, one.data_ptr(), 0, None, 0, 0.0, 0, out.data_ptr(), 5, 25, None)
    assert bool(torch.isnan(out).all())
