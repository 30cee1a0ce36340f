"""mxf_robustmax_expect and mxf_robustmax_probs on the GPU against tests/_robustmax_ref.py (float64 torch on the CPU, gradients by autograd),
both dtypes; a float32 run is held to the reference at the float32-rounded inputs.

Shapes, from the kernel's plan (csrc/robustmax.hip): a workgroup is 256 rows, one per thread -- n in {1, 255, 257}; the row is compiled for
C padded to 4, 8, 16, 32 -- C in {2, 3, 4, 5, 9, 17, 32}; a sample has at most 512 chunks of 256 rows, so from n = 512 * 256 + 1 a thread
loops over a second row, and the grid is capped at 65 536 workgroups, so from S = 65 537 a workgroup loops over a second (sample, chunk)
pair -- both at C = 2; S in {1, 2} with each operand shared or owning its sample axis; 1, 20 and 64 nodes.

Inputs: m uniform in [-3, 3]; v uniform in [0.05, 4] with every fifth cycling through 1e-8, 0.3, 25, 1e-3; the labels cover every class.
Bars (those of tests/test_gpu_psi.py): float64 rtol 1e-9 / atol 1e-11, float32 rtol 1e-4 / atol 1e-5; out[s], a sum, relative to the sum of the
magnitudes of its terms.  Every output is finite."""
import numpy as np
import pytest
import torch

import _robustmax_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
EPS = 1e-3
FILL = 0.5


def _inputs(Sy, Sm, Sv, n, C, dtype, seed=0):
    """CPU tensors of the call's dtype: y (Sy, n, 1), m (Sm, n, C), v (Sv, n)"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-3.0, 3.0, (Sm, n, C))
    v = rng.uniform(0.05, 4.0, (Sv, n))
    special = np.array([1e-8, 0.3, 25.0, 1e-3])
    idx = np.arange(0, n, 5)
    v[:, idx] = special[(idx // 5) % 4]
    y = np.stack([rng.permutation(n) % C for _ in range(Sy)])[..., None].astype(np.float64)
    return [torch.as_tensor(a).to(dtype) for a in (y, m, v)]


def _reference(y, m, v, scale, cot, nq, eps=EPS):
    """out (S,), the sum of the magnitudes of its terms (S,), dm (S, n, C), dv (S, n) with the sample axis on every gradient, and probs"""
    S = max(t.shape[0] for t in (y, m, v))
    C = m.shape[-1]
    yl = R.labels(y.double(), C).expand(S, -1)
    md = m.double().expand(S, -1, -1).clone().requires_grad_(True)
    vd = v.double().expand(S, -1).clone().requires_grad_(True)
    e = R.expect_elem(yl, md, vd, eps, nq)
    out = scale * e.sum(-1)
    w = torch.ones(S, dtype=torch.float64) if cot is None else cot.double()
    dm, dv = torch.autograd.grad((out * w).sum(), [md, vd])
    with torch.no_grad():
        pr = R.probs(md.detach(), vd.detach(), nq)
    return out.detach(), abs(scale) * e.detach().abs().sum(-1), dm, dv, pr


def _close(got, ref, dtype, scale=None):
    rtol, atol = BARS[dtype]
    got, ref = got.double().cpu(), ref.double()
    assert bool(torch.isfinite(got).all())
    bound = rtol * (ref.abs() if scale is None else scale) + atol
    err = (got - ref).abs()
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))


def _run_and_check(y, m, v, dtype, nq=20, scale=0.7, with_cot=True, check_probs=True):
    from mxfusion_amd import ops
    S = max(t.shape[0] for t in (y, m, v))
    n, C = m.shape[1], m.shape[2]
    cot = torch.linspace(0.6, 1.7, S).to(dtype) if with_cot else None
    ref_out, ref_mag, ref_dm, ref_dv, ref_pr = _reference(y, m, v, scale, cot, nq)
    out = torch.full((S,), FILL, dtype=dtype, device='cuda')
    dm = torch.full((S, n, C), FILL, dtype=dtype, device='cuda')
    dv = torch.full((S, n), FILL, dtype=dtype, device='cuda')
    ops.robustmax_expect_(y.cuda(), m.cuda(), v.cuda(), EPS, scale, out, dm_acc=dm, dv_acc=dv, cot=None if cot is None else cot.cuda(),
                          num_nodes=nq)
    _close(out - FILL, ref_out, dtype, scale=ref_mag + FILL)
    _close(dm, ref_dm + FILL, dtype)
    _close(dv, ref_dv + FILL, dtype)
    if check_probs:
        pr = ops.robustmax_probs(m.cuda(), v.cuda(), num_nodes=nq)
        assert pr.shape == (max(m.shape[0], v.shape[0]), n, C)
        ref = ref_pr if pr.shape[0] == S else ref_pr[:1]
        _close(pr, ref, dtype)
        # not renormalised: the sum is 1 within the rule's own error, which the reference shows, plus the bar on C values
        rtol, atol = BARS[dtype]
        dev = (pr.double().cpu().sum(-1) - 1.0).abs()
        assert bool((dev <= (ref.sum(-1) - 1.0).abs() + C * (rtol + atol)).all()), float(dev.max())
    return out, dm, dv


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('C', [2, 3, 4, 5, 9, 17, 32])
def test_every_padded_size(C, dtype):
    """either side of every padded size; S = 2 with shared labels and variances under sampled means, per-sample weights"""
    y, m, v = _inputs(1, 2, 1, 257, C, dtype, seed=C)
    _run_and_check(y, m, v, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('nq', [1, 20, 64])
@pytest.mark.parametrize('n', [1, 255, 257])
def test_rows_and_nodes(n, nq, dtype):
    y, m, v = _inputs(1, 1, 1, n, 3, dtype, seed=n + nq)
    _run_and_check(y, m, v, dtype, nq=nq, with_cot=False)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_sample_axes(dtype):
    """S = 2: every combination of y, m, v shared or owning its sample axis"""
    for k in range(1, 8):
        Sy, Sm, Sv = 1 + (k & 1), 1 + (k >> 1 & 1), 1 + (k >> 2 & 1)
        y, m, v = _inputs(Sy, Sm, Sv, 40, 5, dtype, seed=k)
        _run_and_check(y, m, v, dtype, with_cot=bool(k & 1))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_loops_over_rows_and_pairs(dtype):
    """n = 512 * 256 + 1: the first thread of the first chunk takes a second row; S = 65 537 at n = 1: the first workgroup a second pair"""
    y, m, v = _inputs(1, 1, 1, 512 * 256 + 1, 2, dtype, seed=1)
    _run_and_check(y, m, v, dtype, check_probs=False)
    y, m, v = _inputs(1, 65537, 1, 1, 2, dtype, seed=2)
    _run_and_check(y, m, v, dtype, with_cot=False, check_probs=False)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_zero_and_negative_variance_count_as_the_floor(dtype):
    from mxfusion_amd import ops
    y, m, v = _inputs(1, 1, 1, 64, 3, dtype, seed=5)
    v[0, 0], v[0, 1], v[0, 2] = 0.0, -1.0, 1e-12
    m[0, 2] = m[0, 0]
    y[0, 2] = y[0, 0]
    out, dm, dv = _run_and_check(y, m, v, dtype)
    assert float(dv[0, 0]) == FILL and float(dv[0, 1]) == FILL          # below the floor: no gradient in v
    assert bool((dm[0, 0] == dm[0, 2]).all())                           # v = 0 is the row at the floor
    pr = ops.robustmax_probs(m.cuda(), v.cuda())
    assert bool((pr[0, 0] == pr[0, 2]).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_null_gradients_and_out_of_range_labels(dtype):
    """dm or dv absent: the others unchanged; labels -1, C and 2.5 read as 0, C - 1 and 2 -- an ordinary run with a defined result"""
    from mxfusion_amd import ops
    C, n = 4, 33
    y, m, v = _inputs(1, 1, 1, n, C, dtype, seed=7)
    yd, md, vd = y.cuda(), m.cuda(), v.cuda()
    full = [torch.zeros(s, dtype=dtype, device='cuda') for s in ((1,), (1, n, C), (1, n))]
    ops.robustmax_expect_(yd, md, vd, EPS, 1.3, full[0], dm_acc=full[1], dv_acc=full[2])
    for skip in ('dm', 'dv', 'both'):
        out = torch.zeros(1, dtype=dtype, device='cuda')
        dm = None if skip in ('dm', 'both') else torch.zeros(1, n, C, dtype=dtype, device='cuda')
        dv = None if skip in ('dv', 'both') else torch.zeros(1, n, dtype=dtype, device='cuda')
        ops.robustmax_expect_(yd, md, vd, EPS, 1.3, out, dm_acc=dm, dv_acc=dv)
        _close(out, full[0].cpu(), dtype)
        assert dm is None or bool((dm == full[1]).all())
        assert dv is None or bool((dv == full[2]).all())
    bad, read_as = y.clone(), y.clone()
    for i, (b, r) in enumerate(((-1.0, 0.0), (float(C), C - 1.0), (2.5, 2.0), (1e9, C - 1.0), (-1e9, 0.0))):
        bad[0, i, 0], read_as[0, i, 0] = b, r
    got = [torch.zeros(s, dtype=dtype, device='cuda') for s in ((1,), (1, n, C), (1, n))]
    want = [torch.zeros(s, dtype=dtype, device='cuda') for s in ((1,), (1, n, C), (1, n))]
    ops.robustmax_expect_(bad.cuda(), md, vd, EPS, 1.0, got[0], dm_acc=got[1], dv_acc=got[2])
    ops.robustmax_expect_(read_as.cuda(), md, vd, EPS, 1.0, want[0], dm_acc=want[1], dv_acc=want[2])
    torch.cuda.synchronize()
    assert all(bool((a == b).all()) and bool(torch.isfinite(a).all()) for a, b in zip(got, want))
    ref = _reference(read_as, m, v, 1.0, None, 20)
    _close(got[0], ref[0], dtype, scale=ref[1])


def test_refused_calls():
    """C = 33 and C = 1 are status -3; eps outside (0, 1), a null out and a null probs are status -2; nothing is written"""
    from mxfusion_amd import _lib, ops
    n = 8
    for C, code in ((33, -3), (1, -3)):
        y, m, v = [torch.zeros(s, dtype=torch.float64, device='cuda') for s in ((1, n, 1), (1, n, C), (1, n))]
        out = torch.full((1,), FILL, dtype=torch.float64, device='cuda')
        pr = torch.full((1, n, C), FILL, dtype=torch.float64, device='cuda')
        nodes = ops.lik_nodes(20)
        with pytest.raises(_lib.MXFError, match=r'\(%d\).*32' % code):
            _lib.call('mxf_robustmax_expect', ops._h(m), _lib.F64, 1, n, C, y.data_ptr(), 0, m.data_ptr(), 0, v.data_ptr(), 0, *nodes, 1e-3, None, 1.0,
                      out.data_ptr(), None, None, ops._stream())
        with pytest.raises(_lib.MXFError, match=r'\(%d\).*32' % code):
            _lib.call('mxf_robustmax_probs', ops._h(m), _lib.F64, 1, n, C, m.data_ptr(), 0, v.data_ptr(), 0, *nodes, pr.data_ptr(), ops._stream())
        with pytest.raises(ValueError):
            ops.robustmax_probs(m, v)
        assert float(out) == FILL and bool((pr == FILL).all())
    C = 3
    y, m, v = [torch.zeros(s, dtype=torch.float64, device='cuda') for s in ((1, n, 1), (1, n, C), (1, n))]
    out = torch.full((1,), FILL, dtype=torch.float64, device='cuda')
    for eps in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(_lib.MXFError, match=r'\(-2\).*eps'):
            _lib.call('mxf_robustmax_expect', ops._h(m), _lib.F64, 1, n, C, y.data_ptr(), 0, m.data_ptr(), 0, v.data_ptr(), 0, *nodes, eps, None, 1.0,
                      out.data_ptr(), None, None, ops._stream())
        with pytest.raises(ValueError):
            ops.robustmax_expect_(y, m, v, eps, 1.0, out)
    with pytest.raises(_lib.MXFError, match=r'\(-2\).*null out'):
        _lib.call('mxf_robustmax_expect', ops._h(m), _lib.F64, 1, n, C, y.data_ptr(), 0, m.data_ptr(), 0, v.data_ptr(), 0, *nodes, 1e-3, None, 1.0,
                  None, None, None, ops._stream())
    with pytest.raises(_lib.MXFError, match=r'\(-2\).*null probs'):
        _lib.call('mxf_robustmax_probs', ops._h(m), _lib.F64, 1, n, C, m.data_ptr(), 0, v.data_ptr(), 0, *nodes, None, ops._stream())
    with pytest.raises(_lib.MXFError, match=r'\(-2\).*stride'):
        _lib.call('mxf_robustmax_probs', ops._h(m), _lib.F64, 1, n, C, m.data_ptr(), 5, v.data_ptr(), 0, *nodes, out.data_ptr(), ops._stream())
    assert float(out) == FILL
    with pytest.raises(ValueError):
        ops.robustmax_expect_(y, m, v, 1e-3, 1.0, torch.zeros(2, dtype=torch.float64, device='cuda'))
