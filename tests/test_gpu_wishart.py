"""Wishart on the MI355X: the fused small-matrix kernels (mxf_wishart_*, wishart.hip) up to order 32, the blocked dense path above it, the
class through the API, its draws.  Expected values and gradients are torch.distributions.Wishart(df, covariance_matrix=V).log_prob(X) in
float64 on the CPU with autograd -- never the code under test.

X and V are Q diag(e) Q^T with e log-uniform in [0.1, 10]; nu = n - 1 + uniform(0.5, 6) per sample; the cotangent is uniform(0.5, 1.5);
everything is rounded to the dtype under test before either side sees it.  Errors are normwise per tensor, |got - want|_F / |want|_F,
matrix gradients symmetrised.  float64: 1e-9.  float32: four times the worst normwise error that torch's own float32
CPU log_prob and autograd show against the float64 reference on the same inputs (worst over the case's four tensors: value, dnu, dV, dX),
computed in the test."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 3, 8, 16, 17, 31, 32, 33, 48)          # 33, 48: the blocked dense path
BATCHES = ((1, 1), (3, 5), (2, 257))                   # 257 rows: a ragged last workgroup for any power-of-two rows per workgroup
LAYOUTS = ('per_row', 'V_shared', 'V_per_sample', 'nu_shared', 'nu_per_row', 'X_shared')
NAMES = ('value', 'dnu', 'dV', 'dX')
F64_BAR = 1e-9


def _tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def _round(a, dtype):
    """inputs exactly representable in the dtype under test, as float64: kernel and reference see the same numbers"""
    return np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64)


def _sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def spd(r, shape, n, dtype='float64'):
    """shape + (n, n) matrices Q diag(e) Q^T, e log-uniform in [0.1, 10], rounded to dtype and symmetric"""
    Q = np.linalg.qr(r.randn(*(shape + (n, n))))[0]
    e = np.exp(r.uniform(np.log(0.1), np.log(10.0), shape + (n,)))
    return _sym(_round(_sym((Q * e[..., None, :]) @ np.swapaxes(Q, -1, -2)), dtype))


def reference(X, nu, V, cot, dtype):
    """log p (S, B) and the gradients of sum(cot * log p) w.r.t. nu, V, X, shaped like them: torch.distributions on the CPU in `dtype`.
    nu (S|1,) is one value per sample; (S|1, B) one per row."""
    lX, lnu, lV = [torch.as_tensor(t, dtype=dtype).requires_grad_(True) for t in (X, nu, V)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                          # "low df": n - 1 < nu < n is inside the support
        lp = torch.distributions.Wishart(lnu.reshape(-1, 1) if lnu.dim() == 1 else lnu, covariance_matrix=lV, validate_args=False).log_prob(lX)
    g = torch.autograd.grad((lp * torch.as_tensor(cot, dtype=dtype)).sum(), [lnu, lV, lX])
    out = [lp.detach().double().numpy()] + [t.double().numpy() for t in g]
    return out[:2] + [_sym(out[2]), _sym(out[3])]


def nerr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


@functools.lru_cache(maxsize=None)
def case(dtype, n, S, B, layout):
    """(X, nu, V, cot) in float64 numpy, the reference value and gradients, the bar -- computed once per case and shared"""
    r = np.random.RandomState(1000 * n + 10 * S + B + len(layout))
    sx = (1, B) if layout == 'X_shared' else (S, B)
    sv = {'V_shared': (1, 1), 'V_per_sample': (S, 1)}.get(layout, (S, B))
    sn = {'nu_shared': (1,), 'nu_per_row': (S, B)}.get(layout, (S,))
    X, V = spd(r, sx, n, dtype), spd(r, sv, n, dtype)
    nu, cot = _round(n - 1 + r.uniform(0.5, 6.0, sn), dtype), _round(r.uniform(0.5, 1.5, (S, B)), dtype)
    want = reference(X, nu, V, cot, torch.float64)
    bar = F64_BAR
    if dtype == 'float32':
        bar = 4 * max(nerr(g, w) for g, w in zip(reference(X, nu, V, cot, torch.float32), want))
    return (X, nu, V, cot), want, bar


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=_tdt(dtype)).cuda()


def _factor(dtype, rv_shape, **kw):
    from mxfusion_amd.components.distributions import Wishart
    return Wishart.define_variable(shape=rv_shape, dtype=dtype, **kw).factor


def _variables(f, X, nu, V):
    return {f.random_variable.uuid: X, f.inputs[0][1].uuid: nu, f.inputs[1][1].uuid: V}


def run_api(dtype, ops_in, scaling=1):
    """log_pdf through the class and its reverse mode under the cotangent: [value, dnu, dV, dX] as float64 numpy"""
    X, nu, V, cot = ops_in
    f = _factor(dtype, tuple(X.shape[1:]))
    f.log_pdf_scaling = scaling
    lX, lnu, lV = [_dev(t, dtype).requires_grad_(True) for t in (X, nu, V)]
    lp = f.log_pdf(F=None, variables=_variables(f, lX, lnu, lV))
    assert lp.dtype == _tdt(dtype) and tuple(lp.shape) == tuple(cot.shape)
    g = torch.autograd.grad((lp * _dev(cot, dtype)).sum(), [lnu, lV, lX])
    torch.cuda.synchronize()
    assert int(f._last_info.abs().max()) == 0
    out = [lp.detach().double().cpu().numpy()] + [t.double().cpu().numpy() for t in g]
    return out[:2] + [_sym(out[2]), _sym(out[3])]


WORST = {}          # dtype -> (worst error, widest bar): printed for the record of a run


def check(dtype, n, S, B, layout, scaling=1):
    ops_in, want, bar = case(dtype, n, S, B, layout)
    got = run_api(dtype, ops_in, scaling)
    errs = [nerr(g, scaling * w) for g, w in zip(got, want)]
    worst = WORST.get(dtype, (0.0, 0.0))
    WORST[dtype] = (max(worst[0], max(errs)), max(worst[1], bar))
    print('%s n=%d (S, B)=(%d, %d) %s: errors value %.3g dnu %.3g dV %.3g dX %.3g, bar %.3g; worst so far %.3g, widest bar %.3g'
          % ((dtype, n, S, B, layout) + tuple(errs) + (bar,) + WORST[dtype]))
    for name, g, w, e in zip(NAMES, got, want, errs):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert e <= bar, (name, e, bar)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('n', ORDERS)
def test_orders(n, dtype):
    """1, the non-powers of two and the limit itself on the fused path; 33 and 48 on the dense one"""
    check(dtype, n, 3, 5, 'per_row')
    check(dtype, n, 3, 5, 'V_shared')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('S, B', BATCHES)
@pytest.mark.parametrize('n', [3, 32])
def test_batches(n, S, B, dtype):
    check(dtype, n, S, B, 'per_row')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('n, S, B', [(5, 3, 5), (17, 2, 257), (33, 3, 5)])
def test_broadcast_layouts(n, S, B, layout, dtype):
    """where the reverse mode's summation goes wrong: every operand shared over one or both leading axes, value and all three gradients"""
    check(dtype, n, S, B, layout)


@pytest.mark.parametrize('n', [5, 33])
def test_log_pdf_scaling_follows_the_reference(n):
    """wishart.py:96 multiplies by log_pdf_scaling: value and gradients are 8 times the unscaled ones"""
    check('float64', n, 3, 5, 'V_per_sample', scaling=8)


def test_expanded_operands_are_passed_as_broadcasts():
    """an expanded (stride-0) scale and nu reach the kernel as shared operands: same value, gradient summed into the one copy"""
    n, S, B = 5, 3, 5
    r = np.random.RandomState(7)
    X, V, nu, cot = spd(r, (S, B), n), spd(r, (1, 1), n), n - 1 + r.uniform(0.5, 6.0, (1, 1)), r.uniform(0.5, 1.5, (S, B))
    want = reference(X, nu, V, cot, torch.float64)
    f = _factor('float64', (B, n, n))
    lV, lnu = _dev(V, 'float64').requires_grad_(True), _dev(nu, 'float64').requires_grad_(True)
    lp = f.log_pdf(F=None, variables=_variables(f, _dev(X, 'float64'), lnu.expand(S, B), lV.expand(S, B, n, n)))
    gnu, gV = torch.autograd.grad((lp * _dev(cot, 'float64')).sum(), [lnu, lV])
    assert nerr(lp.detach().cpu().numpy(), want[0]) <= F64_BAR
    assert nerr(gnu.cpu().numpy(), want[1]) <= F64_BAR and nerr(_sym(gV.cpu().numpy()), want[2]) <= F64_BAR


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_integer_degrees_of_freedom(dtype):
    """wishart.py:82: an integer nu is cast to the distribution's dtype, which the result has"""
    n, S, B = 3, 2, 4
    r = np.random.RandomState(5)
    X, V = spd(r, (S, B), n, dtype), spd(r, (S, B), n, dtype)
    f = _factor(dtype, (B, n, n))
    lp = f.log_pdf(F=None, variables=_variables(f, _dev(X, dtype), torch.tensor([4], dtype=torch.int32).cuda(), _dev(V, dtype)))
    assert lp.dtype == _tdt(dtype) and tuple(lp.shape) == (S, B)
    want = reference(X, np.array([4.0]), V, np.ones((S, B)), torch.float64)[0]
    bar = F64_BAR if dtype == 'float64' else 4 * nerr(reference(X, np.array([4.0]), V, np.ones((S, B)), torch.float32)[0], want)
    assert nerr(lp.double().cpu().numpy(), want) <= bar


def test_the_reference_test_case():
    """testing/components/distributions/wishart_test.py:46-101: n = 2, nu = 2 (int32), 6 samples of 3 matrices, the variable equal to the
    scale, float32, against scipy.stats.wishart.logpdf under np.allclose's defaults"""
    from scipy.stats import wishart
    S, B, n = 6, 3, 2
    A = spd(np.random.RandomState(0), (S, B), n, 'float32')
    f = _factor('float32', (B, n, n), rand_gen=None)
    lp = f.log_pdf(F=None, variables=_variables(f, _dev(A, 'float32'), torch.tensor([2], dtype=torch.int32).cuda(), _dev(A, 'float32')))
    want = np.array([[wishart.logpdf(A[s, b], df=2, scale=A[s, b]) for b in range(B)] for s in range(S)])
    assert lp.dtype == torch.float32 and np.allclose(want, lp.cpu().numpy())


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_failures_are_flagged_row_by_row(dtype):
    """In a (2, 3) batch of order 5 one X is indefinite, in another row V is, in a third nu = n - 1: info is n + j, j and 2 n + 1 with j
    the first leading minor that is not positive definite, those rows are NaN in the value and in their gradients, the other rows meet
    the bars, and the call returns normally."""
    n, S, B = 5, 2, 3
    r = np.random.RandomState(3)
    X, V, nu, cot = spd(r, (S, B), n, dtype), spd(r, (S, B), n, dtype), _round(n - 1 + r.uniform(0.5, 6.0, (S, B)), dtype), np.ones((S, B))
    Q = np.linalg.qr(r.randn(n, n))[0]
    X[0, 1] = _sym(_round(_sym((Q * np.array([1.0, 2.0, 3.0, -1.0, 1.5])) @ Q.T), dtype))
    V[1, 0] = _sym(_round(_sym((Q * np.array([2.0, -0.5, 1.0, 1.0, 3.0])) @ Q.T), dtype))
    nu[1, 2] = n - 1
    minor = lambda A: next(k for k in range(1, n + 1) if np.linalg.eigvalsh(A[:k, :k]).min() <= 0)
    f = _factor(dtype, (B, n, n))
    lX, lnu, lV = [_dev(t, dtype).requires_grad_(True) for t in (X, nu, V)]
    lp = f.log_pdf(F=None, variables=_variables(f, lX, lnu, lV))
    g = torch.autograd.grad((lp * _dev(cot, dtype)).sum(), [lnu, lV, lX])
    torch.cuda.synchronize()
    assert f._last_info.cpu().tolist() == [[0, n + minor(X[0, 1]), 0], [minor(V[1, 0]), 0, 2 * n + 1]]
    got = [lp.detach().double().cpu().numpy()] + [t.double().cpu().numpy() for t in g]
    good = np.array([[True, False, True], [False, True, False]])
    for t in got:
        assert np.isnan(t[~good]).all() and np.isfinite(t[good]).all()
    want = reference(X[good][None], nu[good][None], V[good][None], cot[good][None], torch.float64)
    bar = F64_BAR
    if dtype == 'float32':
        bar = 4 * max(nerr(a, b) for a, b in zip(reference(X[good][None], nu[good][None], V[good][None], cot[good][None], torch.float32), want))
    for name, t, w in zip(NAMES, got, want):
        t = t[good][None]
        assert nerr(_sym(t) if t.ndim == 4 else t, w) <= bar, name


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_abi_statuses_and_an_empty_call():
    """n = 0 and n = 33 are status -3, a bad dtype and a null X are -2, S = 0 returns 0; none of them writes anything"""
    from mxfusion_amd import _lib
    raw, h, stream = _lib.load(), _lib.handle(torch.cuda.current_device()), torch.cuda.current_stream().cuda_stream
    S, B, n, fill = 2, 3, 4, 123.0
    z = lambda *s: torch.full(s, 1.0, dtype=torch.float64, device='cuda')
    X = torch.eye(33, dtype=torch.float64, device='cuda').expand(S, B, 33, 33).contiguous()
    nu, cot = z(S, B) * 40, z(S, B)
    outs = {k: torch.full(s, fill, dtype=torch.float64, device='cuda') for k, s in
            (('out', (S, B)), ('dX', (S, B, 33, 33)), ('dnu', (S, B)), ('dV', (S, B, 33, 33)))}
    info = torch.full((S * B,), 77, dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    i64 = ctypes.c_int64

    def both(dt, S_, n_, Xp):
        ld, sm = i64(max(n_, 1)), i64(max(n_, 1) ** 2)
        ops_ = (dt, S_, i64(B), n_, Xp, ld, i64(B * sm.value), p(nu), i64(B), i64(1), p(X), ld, i64(B * sm.value), sm, S_, i64(B))
        return (raw.mxf_wishart_logpdf(h, *ops_, 1.0, p(outs['out']), p(info), stream),
                raw.mxf_wishart_logpdf_bwd(h, *ops_, p(cot), 1.0, p(outs['dX']), p(outs['dnu']), p(outs['dV']), stream))

    assert both(_lib.F64, S, 0, p(X)) == (-3, -3)
    assert both(_lib.F64, S, 33, p(X)) == (-3, -3) and b'33' in raw.mxf_last_error(h)
    assert both(7, S, n, p(X)) == (-2, -2)
    assert both(_lib.F64, S, n, ctypes.c_void_p(None)) == (-2, -2)
    assert both(_lib.F64, 0, n, p(X)) == (0, 0)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == fill).all()), k
    assert info.cpu().tolist() == [77] * (S * B)
    from mxfusion_amd import ops
    with pytest.raises(_lib.MXFError):
        ops.wishart_logpdf(X, nu, X)


def test_direct_call_accumulates_and_skips_a_missing_buffer():
    """wishart_logpdf_bwd_ into buffers pre-filled with ones gives ones plus the gradient; a None buffer is skipped"""
    from mxfusion_amd import ops
    (X, nu, V, cot), want, _ = case('float64', 5, 3, 5, 'V_per_sample')
    Xd, nud, Vd, cotd = _dev(X, 'float64'), _dev(nu, 'float64').reshape(3, 1), _dev(V, 'float64'), _dev(cot, 'float64')
    out, info = ops.wishart_logpdf(Xd, nud, Vd)
    assert nerr(out.cpu().numpy(), want[0]) <= F64_BAR and int(info.abs().max()) == 0
    ones = lambda t: torch.ones_like(t)
    dX, dnu, dV = ones(Xd), ones(nud), ones(Vd)
    ops.wishart_logpdf_bwd_(Xd, nud, Vd, cotd, 1.0, dX, dnu, dV)
    dnu2, dV2 = ones(nud), ones(Vd)
    ops.wishart_logpdf_bwd_(Xd, nud, Vd, cotd, 1.0, None, dnu2, dV2)
    dX3 = ones(Xd)
    ops.wishart_logpdf_bwd_(Xd, nud, Vd, cotd, 1.0, dX3, None, None)
    torch.cuda.synchronize()
    for got, w in ((dnu.reshape(3), want[1]), (dnu2.reshape(3), want[1]), (dV, want[2]), (dV2, want[2]), (dX, want[3]), (dX3, want[3])):
        got = got.cpu().numpy() - 1.0
        assert nerr(_sym(got) if got.ndim == 4 else got, w) <= F64_BAR


def test_operands_that_do_not_fit_the_layout_are_copied_and_the_copies_outlive_the_launch():
    """X and V as views whose last stride is 2: the wrappers copy them, and the copies have to stay alive until the kernel has read them
    (the output and info buffers are allocated after the copies): bit for bit the results of the contiguous operands"""
    from mxfusion_amd import ops
    (X, nu, V, cot), _, _ = case('float64', 5, 3, 5, 'nu_per_row')          # nothing is shared: no sum in arrival order
    Xd, nud, Vd, cotd = _dev(X, 'float64'), _dev(nu, 'float64'), _dev(V, 'float64'), _dev(cot, 'float64')

    def wide(t):
        buf = torch.full(tuple(t.shape[:-1]) + (2 * t.shape[-1],), float('nan'), dtype=t.dtype, device=t.device)
        buf[..., ::2] = t
        return buf[..., ::2]
    Xw, Vw = wide(Xd), wide(Vd)
    assert Xw.stride(-1) == 2 and Vw.stride(-1) == 2
    want, want_info = ops.wishart_logpdf(Xd, nud, Vd)
    grads = [torch.zeros_like(t) for t in (Xd, nud, Vd)]
    ops.wishart_logpdf_bwd_(Xd, nud, Vd, cotd, 1.0, *grads)
    for _ in range(3):                                   # (the allocator hands a freed block to the next request of its size)
        got, info = ops.wishart_logpdf(Xw, nud, Vw)
        g2 = [torch.zeros_like(t) for t in (Xd, nud, Vd)]
        ops.wishart_logpdf_bwd_(Xw, nud, Vw, cotd, 1.0, *g2)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(info, want_info) and int(info.abs().max()) == 0
        for a, b in zip(g2, grads):
            assert torch.equal(a, b)


# ---- draws -------------------------------------------------------------------------------------------------------------------------------

def _bartlett(V, buf, S, lead, n, dt):
    """the documented construction in NumPy in the precision dt: the normal draw first, (S,) + lead + (n, n), its strict lower triangle A's
    off-diagonal entries; then the chi-squared draw, (S,) + lead + (n,), its square root A's diagonal; X = (L A)(L A)^T"""
    buf = buf.astype(dt)
    k = S * int(np.prod(lead)) * n * n
    eps, c = buf[:k].reshape((S,) + lead + (n, n)), buf[k:k + k // n].reshape((S,) + lead + (n,))
    A = np.tril(eps, -1) + np.sqrt(c)[..., None] * np.eye(n, dtype=dt)
    LA = np.linalg.cholesky(V.astype(dt)) @ A
    return LA @ np.swapaxes(LA, -1, -2)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('per_row', [False, True])
def test_draws_with_injected_noise(per_row, dtype):
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    S, lead, n = 4, (5,), 3
    r = np.random.RandomState(11)
    V = spd(r, (S,) + lead if per_row else (1,), n, dtype)
    buf = _round(np.concatenate([r.randn(S * 5 * n * n), r.uniform(0.5, 4.0, S * 5 * n)]), dtype)
    f = _factor(dtype, lead + (n, n), rand_gen=MockRandomGenerator(_dev(buf, dtype)))
    got = f.draw_samples(F=None, variables=_variables(f, None, _dev([5.5], dtype), _dev(V, dtype)), num_samples=S)
    assert got.dtype == _tdt(dtype) and tuple(got.shape) == (S,) + lead + (n, n)
    Vb = V if per_row else V[:, None]
    want = _bartlett(Vb, buf, S, lead, n, np.float64)
    bar = 1e-12 if dtype == 'float64' else 4 * nerr(_bartlett(Vb, buf, S, lead, n, np.float32), want)
    err = nerr(got.double().cpu().numpy(), want)
    print('draw %s per_row=%s: error %.3g, bar %.3g' % (dtype, per_row, err, bar))
    assert err <= bar


@pytest.mark.parametrize('n', [1, 3])
def test_draws_from_the_device_generator_have_the_wishart_mean(n):
    """E X = nu V and Var X_ij = nu (V_ij^2 + V_ii V_jj): 20 000 draws, every entry of the sample mean within five standard errors"""
    torch.manual_seed(1234)
    N, nu = 20000, 3.0 if n == 1 else 5.5
    V = np.ones((1, 1, 1)) if n == 1 else np.array([[[2.0, 0.6, -0.3], [0.6, 1.0, 0.2], [-0.3, 0.2, 0.5]]])
    f = _factor('float64', (n, n))
    X = f.draw_samples(F=None, variables=_variables(f, None, _dev([nu], 'float64'), _dev(V, 'float64')), num_samples=N)
    assert tuple(X.shape) == (N, n, n)
    mean = X.mean(0).cpu().numpy()
    d = np.diag(V[0])
    se = np.sqrt(nu * (V[0] ** 2 + np.outer(d, d)) / N)
    assert (np.abs(mean - nu * V[0]) <= 5 * se).all(), (mean, nu * V[0], se)


def test_draws_are_differentiable_in_the_scale():
    """d sum(draw) / dV through the Cholesky factor against the same construction under torch autograd on the CPU, float64, 1e-9"""
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    S, B, n = 4, 5, 3
    r = np.random.RandomState(12)
    V = spd(r, (1,), n)
    buf = np.concatenate([r.randn(S * B * n * n), r.uniform(0.5, 4.0, S * B * n)])
    f = _factor('float64', (B, n, n), rand_gen=MockRandomGenerator(_dev(buf, 'float64')))
    Vd = _dev(V, 'float64').requires_grad_(True)
    got = f.draw_samples(F=None, variables=_variables(f, None, _dev([5.5], 'float64'), Vd), num_samples=S)
    g, = torch.autograd.grad(got.sum(), Vd)
    Vc = torch.as_tensor(V).requires_grad_(True)
    k = S * B * n * n
    eps, c = torch.as_tensor(buf[:k]).reshape(S, B, n, n), torch.as_tensor(buf[k:]).reshape(S, B, n)
    LA = torch.linalg.cholesky(Vc) @ (torch.tril(eps, -1) + torch.diag_embed(torch.sqrt(c)))
    gw, = torch.autograd.grad((LA @ LA.transpose(-1, -2)).sum(), Vc)
    assert nerr(_sym(g.cpu().numpy()), _sym(gw.numpy())) <= 1e-9
