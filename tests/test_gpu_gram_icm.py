"""GPU tests of the fused coregionalisation Gram pass and its reverse mode (mxf_gram_icm / mxf_gram_icm_bwd; csrc/gram_icm.hip) against
the float64 restatement tests/_coreg_ref.py on the dtype-rounded operands.

Bars: the project's own for the passes this one extends, scaled by max|B|.
    K         rtol = tol, atol = tol var max|B|,        tol = 1e-11 (float64) / 1e-5 (float32)      (test_gram_shapes_vs_oracle)
    gradients rtol = tol, atol = tol max(1, max|ref|),  tol = 1e-9 / 2e-4                           (test_gram_bwd_vs_autograd)
Shapes sit at the tile edges (csrc/gram_icm_plan.h: 256 columns per workgroup, 64 rows per band): one pair, fewer rows and columns than a
tile, more than one column tile and band, Q at the coordinate tiles' ends (1, 3, 5, 8, 16) and T in {1, 3, 32}."""
import functools

import numpy as np
import pytest
import torch

import _coreg_ref as R

pytestmark = pytest.mark.gpu

TOL_K = {torch.float64: 1e-11, torch.float32: 1e-5}
TOL_G = {torch.float64: 1e-9, torch.float32: 2e-4}
SHAPES = [(1, 1, 1, 1), (7, 5, 3, 1), (70, 300, 8, 2), (130, None, 5, 2), (64, 257, 16, 1), (33, 700, 1, 1)]
NAMES = ('X', 'X2', 'ls', 'var', 'B')


def dev(t, dtype):
    return None if t is None else (torch.as_tensor(t).cuda() if dtype is None else t.to(dtype).cuda())


def dev_case(c, dtype):
    return dict(X=dev(c['X'], dtype), X2=dev(c['X2'], dtype), idx=dev(c['idx'], None), idx2=dev(c['idx2'], None), ls=dev(c['ls'], dtype),
                var=dev(c['var'], dtype), B=dev(c['B'], dtype), dK=dev(c['dK'], dtype))


@functools.lru_cache(maxsize=None)
def case(N, N2, Q, S, T, ard, f32):
    return R.make_case(N + Q + T, N, N2, Q, S, T, ard, f32=f32)


@functools.lru_cache(maxsize=None)
def reference(kind, N, N2, Q, S, T, ard, f32):
    c = case(N, N2, Q, S, T, ard, f32)
    return R.icm_grads(kind, c['X'], c['X2'], c['idx'], c['idx2'], c['ls'], c['var'], c['B'], c['dK'])


def check_K(K, ref, c, dtype, what):
    tol = TOL_K[dtype]
    atol = tol * float(c['var'].max()) * float(c['B'].abs().max())
    err = (K.double().cpu() - ref).abs()
    worst = float((err / (atol + tol * ref.abs())).max())
    print('K', what, 'worst ratio', worst)
    assert worst <= 1.0, (what, worst)


def check_grads(got, ref, dtype, what):
    tol = TOL_G[dtype]
    for name, g in zip(NAMES, got):
        if name not in ref:
            assert g is None, (what, name)
            continue
        r = ref[name]
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        err = (g.double().cpu() - r).abs()
        worst = float((err / (tol * max(1.0, float(r.abs().max())) + tol * r.abs())).max())
        print('d' + name, what, 'worst ratio', worst)
        assert worst <= 1.0, (what, name, worst)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('T', [1, 3, 32])
@pytest.mark.parametrize('N,N2,Q,S', SHAPES)
def test_forward_and_reverse_against_the_restatement(N, N2, Q, S, T, dtype):
    from mxfusion_amd import ops
    f32 = dtype == torch.float32
    for kind in R.KINDS:
        for ard in (True, False):
            c = case(N, N2, Q, S, T, ard, f32)
            d = dev_case(c, dtype)
            Kref, gref = reference(kind, N, N2, Q, S, T, ard, f32)
            what = (kind, N, N2, Q, S, T, ard)
            K = ops.gram_icm(kind, d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], ard, d['B'])
            check_K(K, Kref, c, dtype, what)
            got = ops.gram_icm_bwd(kind, d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], ard, d['B'], d['dK'])
            check_grads(got, gref, dtype, what)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_an_output_without_rows_and_all_rows_on_one_output(dtype):
    """T = 4 with no row or column on output 2: row 2 and column 2 of dB are exactly zero.  All rows on output 1 of T = 3 (the columns on
    any): only row 1 of dB is non-zero."""
    from mxfusion_amd import ops
    f32 = dtype == torch.float32
    for T, fix in ((4, 'skip2'), (3, 'one')):
        c = dict(R.make_case(11, 70, 300, 3, 1, T, True, f32=f32))
        if fix == 'skip2':
            c['idx'] = np.where(c['idx'] == 2, 3, c['idx']).astype(np.int32)
            c['idx2'] = np.where(c['idx2'] == 2, 0, c['idx2']).astype(np.int32)
        else:
            c['idx'] = np.full_like(c['idx'], 1)
        d = dev_case(c, dtype)
        Kref, gref = R.icm_grads('matern32', c['X'], c['X2'], c['idx'], c['idx2'], c['ls'], c['var'], c['B'], c['dK'])
        check_K(ops.gram_icm('matern32', d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], True, d['B']), Kref, c, dtype, fix)
        got = ops.gram_icm_bwd('matern32', d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], True, d['B'], d['dK'])
        check_grads(got, gref, dtype, fix)
        dB = got[4].cpu()
        if fix == 'skip2':
            assert float(dB[:, 2, :].abs().max()) == 0.0 and float(dB[:, :, 2].abs().max()) == 0.0
        else:
            assert float(dB[:, [0, 2], :].abs().max()) == 0.0 and float(dB[:, 1, :].abs().min()) > 0.0


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('N2', [300, None])
def test_b_shared_over_the_samples_against_b_per_sample(N2, dtype):
    """S = 2: with the same B for both samples, once passed as (1, T, T) and once as (2, T, T), the shared dB is the sum of the per-sample
    ones (and each agrees with the restatement); every other output is the same."""
    from mxfusion_amd import ops
    f32 = dtype == torch.float32
    c = dict(R.make_case(5, 70, N2, 8, 2, 3, True, f32=f32))
    c['B'] = c['B'][:1].clone()
    d = dev_case(c, dtype)
    args = lambda B: ('rbf', d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], True, B)
    shared = ops.gram_icm_bwd(*args(d['B']), d['dK'])
    per = ops.gram_icm_bwd(*args(d['B'].expand(2, -1, -1).contiguous()), d['dK'])
    assert torch.equal(ops.gram_icm(*args(d['B'])), ops.gram_icm(*args(d['B'].expand(2, -1, -1).contiguous())))
    _, gref = R.icm_grads('rbf', c['X'], c['X2'], c['idx'], c['idx2'], c['ls'], c['var'], c['B'], c['dK'])
    check_grads(shared, gref, dtype, 'shared')
    assert shared[4].shape == (1, 3, 3) and per[4].shape == (2, 3, 3)
    ref = gref['B']
    tol = TOL_G[dtype]
    assert torch.allclose(per[4].double().sum(0, keepdim=True).cpu(), ref, rtol=tol, atol=tol * max(1.0, float(ref.abs().max())))
    assert torch.allclose(shared[4].double(), per[4].double().sum(0, keepdim=True), rtol=tol, atol=tol * max(1.0, float(ref.abs().max())))


def test_every_need_subset_returns_what_the_full_call_returns():
    from mxfusion_amd import ops
    import itertools
    c = R.make_case(3, 70, 300, 3, 2, 3, True)
    d = dev_case(c, torch.float64)
    args = ('matern52', d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], True, d['B'], d['dK'])
    full = ops.gram_icm_bwd(*args)
    tol = TOL_G[torch.float64]
    for k in range(len(NAMES) + 1):
        for need in itertools.combinations(NAMES, k):
            got = ops.gram_icm_bwd(*args, need=need)
            for name, g, f in zip(NAMES, got, full):
                if name not in need:
                    assert g is None, (need, name)
                else:      # the sums arrive in another order: the bar, not bit equality
                    assert torch.allclose(g, f, rtol=tol, atol=tol * max(1.0, float(f.abs().max()))), (need, name)
    sq = ('matern52', d['X'], None, d['idx'], None, d['ls'], d['var'], True, d['B'], d['dK'][:, :, :70].contiguous())
    assert ops.gram_icm_bwd(*sq)[1] is None and ops.gram_icm_bwd(*sq, need=('X2',)) == (None,) * 5


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_row_strides_above_n2_and_poisoned_padding(dtype):
    """dK read with a row stride above N2 gives what the packed dK gives; K_out written into a wider buffer leaves the columns beyond N2
    bit-unchanged (they are poisoned with NaN beforehand)."""
    from mxfusion_amd import ops
    c = R.make_case(9, 70, 300, 8, 2, 3, True, f32=dtype == torch.float32)
    d = dev_case(c, dtype)
    args = ('rbf', d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], True, d['B'])
    K = ops.gram_icm(*args)
    wide = torch.full((2, 70, 333), float('nan'), dtype=dtype, device='cuda')
    poison = wide.clone()
    out = ops.gram_icm(*args, out=wide[:, :, :300])
    assert out.data_ptr() == wide.data_ptr() and torch.equal(wide[:, :, :300], K)
    assert torch.equal(wide[:, :, 300:].view(torch.int32 if dtype == torch.float32 else torch.int64),
                       poison[:, :, 300:].view(torch.int32 if dtype == torch.float32 else torch.int64))
    dKw = torch.full((2, 70, 333), float('nan'), dtype=dtype, device='cuda')
    dKw[:, :, :300] = d['dK']
    packed = ops.gram_icm_bwd(*args, d['dK'])
    strided = ops.gram_icm_bwd(*args, dKw[:, :, :300])
    tol = TOL_G[dtype]
    for name, a, b in zip(NAMES, strided, packed):
        assert bool(torch.isfinite(a).all()) and torch.allclose(a, b, rtol=tol, atol=tol * max(1.0, float(b.abs().max()))), name


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_diag_add_and_jitter_land_on_the_square_diagonal_only(dtype):
    from mxfusion_amd import ops
    c = R.make_case(4, 130, None, 5, 2, 3, False, f32=dtype == torch.float32)
    d = dev_case(c, dtype)
    args = ('matern32', d['X'], None, d['idx'], None, d['ls'], d['var'], False, d['B'])
    diag = torch.tensor([[0.25], [0.75]], dtype=dtype, device='cuda')
    K0, K1 = ops.gram_icm(*args), ops.gram_icm(*args, diag_add=diag, jitter=0.125)
    off = ~torch.eye(130, dtype=torch.bool, device='cuda')
    assert torch.equal(K0[:, off], K1[:, off])
    want = torch.diagonal(K0, dim1=-2, dim2=-1) + (diag + 0.125)
    assert torch.allclose(torch.diagonal(K1, dim1=-2, dim2=-1), want, rtol=4 * torch.finfo(dtype).eps, atol=0)
    ref = R.icm('matern32', c['X'], None, c['idx'], None, c['ls'], c['var'], c['B'], diag_add=diag.double().cpu(), jitter=0.125)
    check_K(K1, ref, c, dtype, 'diag')
    # a rectangular Gram takes neither
    X2 = d['X'][:, :40].contiguous()
    r = ('matern32', d['X'], X2, d['idx'], d['idx'][:40].contiguous(), d['ls'], d['var'], False, d['B'])
    assert torch.equal(ops.gram_icm(*r), ops.gram_icm(*r, diag_add=diag, jitter=0.125))


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('kind', R.KINDS)
def test_b_all_ones_is_the_plain_gram(kind, dtype):
    from mxfusion_amd import ops
    c = R.make_case(6, 70, 300, 8, 2, 3, True, f32=dtype == torch.float32)
    d = dev_case(c, dtype)
    ones = torch.ones(1, 3, 3, dtype=dtype, device='cuda')
    K = ops.gram_icm(kind, d['X'], d['X2'], d['idx'], d['idx2'], d['ls'], d['var'], True, ones)
    G = ops.gram(kind, d['X'], d['X2'], d['ls'], d['var'], True)
    tol = TOL_K[dtype]
    assert torch.allclose(K, G, rtol=tol, atol=tol * float(c['var'].max()))


def test_refusals_and_a_clamped_index():
    """T = 33 is refused with -3 before anything is launched.  An index of T handed straight to the entry point on a 5 x 5 problem is
    clamped to T - 1: finite values, those of the clamped index, and no access outside B (an argument check on valid memory)."""
    from mxfusion_amd import _lib, ops
    c = R.make_case(8, 5, None, 2, 1, 3, True)
    d = dev_case(c, torch.float64)
    B33 = torch.eye(33, dtype=torch.float64, device='cuda')[None]
    with pytest.raises(_lib.MXFError, match=r'\(-3\).*T above the limit of 32 outputs'):
        ops.gram_icm('rbf', d['X'], None, d['idx'], None, d['ls'], d['var'], True, B33)
    with pytest.raises(_lib.MXFError, match=r'\(-3\).*T above the limit of 32 outputs'):
        ops.gram_icm_bwd('rbf', d['X'], None, d['idx'], None, d['ls'], d['var'], True, B33, d['dK'])
    bad = torch.tensor([0, 3, 1, -1, 2], dtype=torch.int32, device='cuda')
    clamped = torch.tensor([0, 2, 1, 0, 2], dtype=torch.int32, device='cuda')
    K = ops.gram_icm('rbf', d['X'], None, bad, None, d['ls'], d['var'], True, d['B'])
    assert bool(torch.isfinite(K).all()) and torch.equal(K, ops.gram_icm('rbf', d['X'], None, clamped, None, d['ls'], d['var'], True, d['B']))
    g = ops.gram_icm_bwd('rbf', d['X'], None, bad, None, d['ls'], d['var'], True, d['B'], d['dK'])
    gc = ops.gram_icm_bwd('rbf', d['X'], None, clamped, None, d['ls'], d['var'], True, d['B'], d['dK'])
    for a, b in zip(g, gc):
        assert (a is None and b is None) or (bool(torch.isfinite(a).all()) and torch.allclose(a, b, rtol=1e-12, atol=1e-12))
