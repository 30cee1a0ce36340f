"""MultivariateNormal and MultivariateNormalMeanPrecision on the MI355X: the fused small-matrix kernels (mxf_mvn_*, mvn.hip) up to order
32, the blocked dense path above it, the classes through the API.  Expected values and gradients are torch.distributions.MultivariateNormal
in float64 on the CPU (covariance_matrix or precision_matrix, autograd) -- never the code under test.

Matrices are Q diag(e) Q^T with e log-uniform in [0.1, 10] (cond <= 100).  Errors are normwise per tensor, |got - want|_F / |want|_F.
float64: 1e-9.  float32: four times the worst normwise error that torch's own float32 CPU log_prob and autograd show
against the float64 reference on the same inputs (worst over the case's four tensors: value, dx, dmean, dA), computed in the test."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _strided as st

pytestmark = pytest.mark.gpu

FORMS = ('covariance', 'precision')
ORDERS = (1, 2, 3, 8, 16, 17, 31, 32, 33, 48)          # 33, 48: the blocked dense path
BATCHES = ((1, 1), (3, 5), (2, 257))                   # 257 rows of 8 per workgroup: a ragged last one
LAYOUTS = ('per_row', 'A_shared', 'A_per_sample', 'mean_shared', 'x_single')
F64_BAR = 1e-9


def _tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def _round(a, dtype):
    """inputs exactly representable in the dtype under test, as float64: kernel and reference see the same numbers"""
    return np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64)


def spd(r, shape, n):
    """shape + (n, n) matrices Q diag(e) Q^T, e log-uniform in [0.1, 10]"""
    Q = np.linalg.qr(r.randn(*(shape + (n, n))))[0]
    e = np.exp(r.uniform(np.log(0.1), np.log(10.0), shape + (n,)))
    A = (Q * e[..., None, :]) @ np.swapaxes(Q, -1, -2)
    return 0.5 * (A + np.swapaxes(A, -1, -2))


@functools.lru_cache(maxsize=None)
def case(form, dtype, n, S, B, layout):
    """(x, mean, A, cot) in float64 numpy, (reference value and gradients), float32 bar -- computed once per case and shared"""
    r = np.random.RandomState(1000 * n + 10 * S + B + len(layout))
    sx = (1, B) if layout == 'x_single' else (S, B)
    sm = (1, 1) if layout == 'mean_shared' else (S, B)
    sa = {'A_shared': (1, 1), 'A_per_sample': (S, 1)}.get(layout, (S, B))
    A = spd(r, sa, n)
    A = _round(A, dtype)
    A = 0.5 * (A + np.swapaxes(A, -1, -2))
    x, mean, cot = _round(r.randn(*(sx + (n,))) * 2, dtype), _round(r.randn(*(sm + (n,))), dtype), _round(r.uniform(0.5, 1.5, (S, B)), dtype)
    want = reference(form, x, mean, A, cot, torch.float64)
    bar = F64_BAR
    if dtype == 'float32':
        t32 = reference(form, x, mean, A, cot, torch.float32)
        bar = 4 * max(nerr(g, w) for g, w in zip(t32, want))
    return (x, mean, A, cot), want, bar


def reference(form, x, mean, A, cot, dtype):
    """log p (S, B) and the gradients of sum(cot * log p) w.r.t. x, mean, A, shaped like them: torch.distributions on the CPU in `dtype`"""
    leaves = [torch.as_tensor(t, dtype=dtype).requires_grad_(True) for t in (x, mean, A)]
    kw = {'covariance_matrix' if form == 'covariance' else 'precision_matrix': leaves[2]}
    lp = torch.distributions.MultivariateNormal(leaves[1], validate_args=False, **kw).log_prob(leaves[0])
    g = torch.autograd.grad((lp * torch.as_tensor(cot, dtype=dtype)).sum(), leaves)
    return [lp.detach().double().numpy()] + [t.double().numpy() for t in g]


def nerr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=_tdt(dtype)).cuda()


def _factor(form, dtype, rv_shape, **kw):
    from mxfusion_amd.components.distributions import MultivariateNormal, MultivariateNormalMeanPrecision
    cls = MultivariateNormal if form == 'covariance' else MultivariateNormalMeanPrecision
    return cls.define_variable(shape=rv_shape, dtype=dtype, **kw).factor


def run_api(form, dtype, ops_in, scaling=1):
    """log_pdf through the class and its reverse mode under the cotangent: [value, dx, dmean, dA] as float64 numpy"""
    x, mean, A, cot = ops_in
    f = _factor(form, dtype, tuple(x.shape[1:]))
    f.log_pdf_scaling = scaling
    leaves = [_dev(t, dtype).requires_grad_(True) for t in (x, mean, A)]
    variables = {f.random_variable.uuid: leaves[0], f.inputs[0][1].uuid: leaves[1], f.inputs[1][1].uuid: leaves[2]}
    lp = f.log_pdf(F=None, variables=variables)
    assert lp.dtype == _tdt(dtype) and tuple(lp.shape) == tuple(cot.shape)
    g = torch.autograd.grad((lp * _dev(cot, dtype)).sum(), leaves)
    torch.cuda.synchronize()
    return [lp.detach().double().cpu().numpy()] + [t.double().cpu().numpy() for t in g]


def check(form, dtype, n, S, B, layout, scaling=1):
    ops_in, want, bar = case(form, dtype, n, S, B, layout)
    got = run_api(form, dtype, ops_in, scaling)
    errs = [nerr(g, scaling * w) for g, w in zip(got, want)]
    print('%s %s n=%d (S, B)=(%d, %d) %s: errors value %.3g dx %.3g dmean %.3g dA %.3g, bar %.3g' % ((form, dtype, n, S, B, layout) + tuple(errs) + (bar,)))
    for name, g, w, e in zip(('value', 'dx', 'dmean', 'dA'), got, want, errs):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert e <= bar, (name, e, bar)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n', ORDERS)
def test_orders(n, form, dtype):
    """1, the non-powers of two and the limit itself on the fused path; 33 and 48 on the dense one"""
    check(form, dtype, n, 3, 5, 'per_row')
    check(form, dtype, n, 3, 5, 'A_shared')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('S, B', BATCHES)
@pytest.mark.parametrize('n', [3, 32])
def test_batches(n, S, B, form, dtype):
    check(form, dtype, n, S, B, 'per_row')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('n, S, B', [(5, 3, 5), (17, 2, 257), (33, 3, 5)])
def test_broadcast_layouts(n, S, B, layout, form, dtype):
    """where the reverse mode's summation goes wrong: every operand shared over one or both leading axes, value and all three gradients"""
    check(form, dtype, n, S, B, layout)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n', [5, 33])
def test_log_pdf_scaling_follows_the_reference(n, form):
    """normal.py:178 and normal.py:394 both multiply by log_pdf_scaling: value and gradients are 8 times the unscaled ones"""
    check(form, 'float64', n, 3, 5, 'A_per_sample', scaling=8)


def test_expanded_operands_are_passed_as_broadcasts():
    """an expanded (stride-0) matrix and mean reach the kernel as shared operands: same value, gradient summed into the one copy"""
    (x, mean, A, cot), want, _ = case('covariance', 'float64', 5, 3, 5, 'A_shared')
    f = _factor('covariance', 'float64', (5, 5))
    Al, ml = _dev(A, 'float64').requires_grad_(True), _dev(mean[:1, :1], 'float64').requires_grad_(True)
    variables = {f.random_variable.uuid: _dev(x, 'float64'), f.inputs[0][1].uuid: ml.expand(3, 5, 5), f.inputs[1][1].uuid: Al.expand(3, 5, 5, 5)}
    ref = reference('covariance', x, np.broadcast_to(mean[:1, :1], x.shape).copy(), A, cot, torch.float64)
    lp = f.log_pdf(F=None, variables=variables)
    gm, gA = torch.autograd.grad((lp * _dev(cot, 'float64')).sum(), [ml, Al])
    assert nerr(lp.detach().cpu().numpy(), ref[0]) <= F64_BAR
    assert nerr(gA.cpu().numpy(), ref[3]) <= F64_BAR and nerr(gm.cpu().numpy(), ref[2].sum((0, 1), keepdims=True)) <= F64_BAR


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def _abi(t):
    from mxfusion_amd import _lib
    dt = {torch.float32: _lib.F32, torch.float64: _lib.F64}[t.dtype]
    return _lib, _lib.handle(torch.cuda.current_device()), dt, torch.cuda.current_stream().cuda_stream


def abi_factor(A, form, call=None):
    """mxf_mvn_factor on a view A (M, n, n): one matrix per sample, the view's own row and sample strides"""
    lib, h, dt, stream = _abi(A)
    M, n = A.shape[0], A.shape[-1]
    F = torch.empty((M, 1, n, n), dtype=A.dtype, device=A.device)
    logdet = torch.empty((M, 1), dtype=A.dtype, device=A.device)
    info = torch.zeros(M, dtype=torch.int32, device=A.device)
    lib.call('mxf_mvn_factor', h, dt, form, M, 1, n, A.data_ptr(), A.stride(-2), A.stride(0), 0, F.data_ptr(), logdet.data_ptr(), info.data_ptr(), stream)
    return F, logdet, info


def abi_logpdf(x, mean, F, logdet, form, cot=None):
    """mxf_mvn_logpdf (and, given a cotangent, mxf_mvn_logpdf_bwd) on a view x (S, B, n) with its own sample stride; mean (S, B, n) dense"""
    lib, h, dt, stream = _abi(x)
    S, B, n = x.shape
    out = torch.empty((S, B), dtype=x.dtype, device=x.device)
    lib.call('mxf_mvn_logpdf', h, dt, form, S, B, n, x.data_ptr(), x.stride(0), mean.data_ptr(), B * n, n, F.data_ptr(), logdet.data_ptr(),
             F.shape[0], F.shape[1], 1.0, out.data_ptr(), stream)
    if cot is None:
        return out
    grads = [torch.zeros(s, dtype=x.dtype, device=x.device) for s in ((S, B, n), (S, B, n), tuple(F.shape))]
    lib.call('mxf_mvn_logpdf_bwd', h, dt, form, S, B, n, x.data_ptr(), x.stride(0), mean.data_ptr(), B * n, n, F.data_ptr(), F.shape[0], F.shape[1],
             cot.data_ptr(), 1.0, grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), stream)
    return [out] + grads


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('form', [0, 1])
def test_not_positive_definite(form, dtype):
    """One matrix of four (n = 5) has a negative eigenvalue: the call returns 0, info names that matrix's first failing pivot, its log-pdf
    is NaN, the other three rows meet the bars."""
    r = np.random.RandomState(3)
    n, bad = 5, 2
    A = spd(r, (4,), n)
    Q = np.linalg.qr(r.randn(n, n))[0]
    A[bad] = (Q * np.array([1.0, 2.0, 3.0, -1.0, 1.5])) @ Q.T
    A = _round(A, dtype)
    A = 0.5 * (A + np.swapaxes(A, -1, -2))
    pivot = next(k for k in range(1, n + 1) if np.linalg.eigvalsh(A[bad][:k, :k]).min() <= 0)      # first leading minor that is not positive definite
    x, mean = _round(r.randn(1, 4, n), dtype), _round(r.randn(1, 4, n), dtype)
    F, logdet, info = abi_factor(_dev(A, dtype), form)                                             # (lib.call raises on a non-zero status)
    out = abi_logpdf(_dev(x, dtype), _dev(mean, dtype), F.reshape(1, 4, n, n), logdet.reshape(1, 4), form)
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [0, 0, pivot, 0]
    got = out.double().cpu().numpy()[0]
    assert np.isnan(got[bad]) and np.isnan(float(logdet[bad, 0]))
    good = [i for i in range(4) if i != bad]
    ref = lambda dt: reference(FORMS[form], x[0, good], mean[0, good], A[good], np.ones(3), dt)[0]
    want = ref(torch.float64)
    bar = F64_BAR if dtype == 'float64' else 4 * nerr(ref(torch.float32), want)
    print('not positive definite, form %d %s: error %.3g, bar %.3g' % (form, dtype, nerr(got[good], want), bar))
    assert nerr(got[good], want) <= bar


def test_order_33_is_refused_and_touches_nothing():
    lib, h, dt, stream = _abi(torch.zeros(1, dtype=torch.float64, device='cuda'))
    raw = lib.load()
    n, S, B = 33, 2, 3
    z = lambda *s: torch.full(s, 1.0, dtype=torch.float64, device='cuda')
    A, x, mean, cot = torch.eye(n, dtype=torch.float64, device='cuda').expand(S, B, n, n).contiguous(), z(S, B, n), z(S, B, n), z(S, B)
    outs = {k: torch.full(s, st.SENTINEL, dtype=torch.float64, device='cuda') for k, s in
            (('F', (S, B, n, n)), ('logdet', (S, B)), ('out', (S, B)), ('dx', (S, B, n)), ('dmean', (S, B, n)), ('dA', (S, B, n, n)))}
    info = torch.full((S * B,), 77, dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    i64 = ctypes.c_int64
    for form in (0, 1):
        rcs = [raw.mxf_mvn_factor(h, dt, form, S, i64(B), n, p(A), i64(n), i64(B * n * n), i64(n * n), p(outs['F']), p(outs['logdet']), p(info), stream),
               raw.mxf_mvn_logpdf(h, dt, form, S, i64(B), n, p(x), i64(B * n), p(mean), i64(B * n), i64(n), p(outs['F']), p(outs['logdet']), S, i64(B),
                                  1.0, p(outs['out']), stream),
               raw.mxf_mvn_logpdf_bwd(h, dt, form, S, i64(B), n, p(x), i64(B * n), p(mean), i64(B * n), i64(n), p(outs['F']), S, i64(B), p(cot), 1.0,
                                      p(outs['dx']), p(outs['dmean']), p(outs['dA']), stream)]
        for rc in rcs:
            assert rc < 0
            assert len(raw.mxf_last_error(h)) > 0 and b'33' in raw.mxf_last_error(h)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert torch.equal(t.view(torch.int64), torch.full_like(t, st.SENTINEL).view(torch.int64)), k
    assert info.cpu().tolist() == [77] * (S * B)
    from mxfusion_amd import ops, _lib
    with pytest.raises(_lib.MXFError):
        ops.mvn_factor(A)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('form', [0, 1])
@pytest.mark.parametrize('n', [5, 32])
def test_strided_operands(n, form, dtype):
    """A as padded, offset, gapped views (row stride > n, base off by one element, a gap between the matrices) and x at an offset base with
    a gap between its samples: bit for bit the results of the dense operands, and not one byte of either allocation written."""
    r = np.random.RandomState(n)
    S, B = 2, 3
    A, x = spd(r, (S * B,), n), r.randn(S, B, n)
    mean, cot = _dev(r.randn(S, B, n), dtype), _dev(r.uniform(0.5, 1.5, (S, B)), dtype)
    F0, ld0, info0 = abi_factor(_dev(A, dtype), form)
    base = abi_logpdf(_dev(x, dtype), mean, F0.reshape(S, B, n, n), ld0.reshape(S, B), form, cot)
    for variant in ('ld+3', 'lead1+ld8', 'gap5+ld8'):
        Av = st.carve_as(A, variant, dtype=_tdt(dtype))
        snap = st.snapshot(Av)
        F, ld, info = abi_factor(Av, form)
        torch.cuda.synchronize()
        st.assert_unchanged(Av, snap, 'A ' + variant)
        assert torch.equal(F, F0) and torch.equal(ld, ld0) and torch.equal(info, info0), variant
    for variant in ('lead1', 'gap5'):
        xv = st.carve_as(x, variant, dtype=_tdt(dtype))
        snap = st.snapshot(xv)
        got = abi_logpdf(xv, mean, F0.reshape(S, B, n, n), ld0.reshape(S, B), form, cot)
        torch.cuda.synchronize()
        st.assert_unchanged(xv, snap, 'x ' + variant)
        for g, b in zip(got, base):
            assert torch.equal(g, b), variant


# ---- draws -------------------------------------------------------------------------------------------------------------------------------

def _draw_reference(form, mean, A, eps):
    """mean + chol(K) eps (covariance), mean + L^-T eps with P = L L^T (precision): float64 CPU torch, differentiable in A"""
    L = torch.linalg.cholesky(A)
    e = eps[..., None]
    y = L @ e if form == 'covariance' else torch.linalg.solve_triangular(L.transpose(-1, -2), e, upper=True)
    return mean + y[..., 0]


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('n, sa', [(3, (1, 1)), (8, (1, 4)), (8, (1, 1)), (40, (1, 4))])
def test_draw_samples_with_injected_noise_and_their_gradient(n, sa, form):
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    r = np.random.RandomState(11 + n)
    S, B = 5, 4
    A, mean, eps = spd(r, sa, n), r.randn(1, B, n), r.randn(S, B, n)
    f = _factor(form, 'float64', (B, n), rand_gen=MockRandomGenerator(_dev(eps.reshape(-1), 'float64')))
    Ad = _dev(A.reshape(sa[1:] + (n, n))[None] if sa[1] > 1 else A.reshape(1, n, n), 'float64').requires_grad_(True)
    got = f.draw_samples(F=None, variables={f.inputs[0][1].uuid: _dev(mean, 'float64'), f.inputs[1][1].uuid: Ad}, num_samples=S)
    Ac = torch.as_tensor(A.reshape(sa[1:] + (n, n)) if sa[1] > 1 else A.reshape(n, n)).requires_grad_(True)
    want = _draw_reference(form, torch.as_tensor(mean), Ac, torch.as_tensor(eps))
    assert tuple(got.shape) == (S, B, n)
    assert nerr(got.detach().cpu().numpy(), want.detach().numpy()) <= F64_BAR
    g, = torch.autograd.grad((got ** 2).sum(), Ad)
    gw, = torch.autograd.grad((want ** 2).sum(), Ac)
    assert nerr(g.cpu().numpy().reshape(gw.shape), gw.numpy()) <= 1e-8


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

def _lower(theta):
    """(..., 6) -> (..., 3, 3) lower factor with a positive (softplus) diagonal"""
    rows, cols = torch.tril_indices(3, 3)
    L = torch.zeros(tuple(theta.shape[:-1]) + (3, 3), dtype=theta.dtype, device=theta.device)
    L[..., rows, cols] = theta
    d = torch.diagonal(L, dim1=-2, dim2=-1)
    return L - torch.diag_embed(d) + torch.diag_embed(torch.nn.functional.softplus(d))


def _mvn_model(learn_sigma):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import MultivariateNormal
    from mxfusion_amd.components.functions.function_evaluation import MXFusionFunction
    from mxfusion_amd.inference import GradBasedInference, MAP
    r = np.random.RandomState(0)
    P0, Sigma = spd(r, (), 3), spd(r, (), 3)
    theta0 = r.randn(6) * 0.5
    if learn_sigma:
        Lt = _lower(torch.as_tensor(theta0))
        Sigma = (Lt @ Lt.T).numpy()
    Y = r.multivariate_normal(np.array([1.0, -2.0, 0.5]), Sigma, size=200)
    m0 = np.array([0.3, -0.2, 0.1])
    dev = lambda t: torch.as_tensor(np.asarray(t), dtype=torch.float64).cuda()
    m = Model()
    m.m = MultivariateNormal.define_variable(shape=(3,), mean=dev(np.zeros(3)), covariance=dev(P0), dtype='float64')
    if learn_sigma:
        m.theta = Variable(shape=(6,), initial_value=dev(theta0))
        m.Sigma = MXFusionFunction(lambda th: (lambda L: L @ L.transpose(-1, -2))(_lower(th)))(m.theta)
        cov = m.Sigma
    else:
        cov = dev(Sigma)
    m.Y = MultivariateNormal.define_variable(shape=(200, 3), mean=m.m, covariance=cov, dtype='float64')
    alg = MAP(model=m, observed=[m.Y], locations={m.m: Variable(shape=(3,), initial_value=dev(m0))})
    infr = GradBasedInference(inference_algorithm=alg, dtype='float64')
    infr.initialize(Y=dev(Y))
    return m, alg, infr, dev(Y), (P0, Sigma, Y, m0, theta0)


def _closed_form(mv, Sigma, P0, Y):
    """sum_i log N(y_i | m, Sigma) + log N(m | 0, P0) on the CPU"""
    D = torch.distributions.MultivariateNormal
    return D(mv, covariance_matrix=Sigma).log_prob(torch.as_tensor(Y)).sum() + D(torch.zeros(3, dtype=torch.float64), covariance_matrix=torch.as_tensor(P0)).log_prob(mv)


def test_map_of_a_gaussian_mean_end_to_end():
    """m ~ N(0, P0), y_i ~ N(m, Sigma), 200 rows, MAP: loss and gradient at the start equal the closed form to 1e-9; the run lowers the loss
    and moves m towards the closed-form posterior mean."""
    m, alg, infr, Yd, (P0, Sigma, Y, m0, _) = _mvn_model(False)
    loc = alg.posterior[m.m].factor.location
    mv = torch.as_tensor(m0).requires_grad_(True)
    want = -_closed_form(mv, torch.as_tensor(Sigma), P0, Y)
    gw, = torch.autograd.grad(want, mv)
    loss, loss_for_gradient = infr.create_executor()(Yd)
    assert abs(float(loss) - float(want)) <= 1e-9 * abs(float(want)), (float(loss), float(want))
    loss_for_gradient.backward()
    assert nerr(infr.params.grad(loc).cpu().numpy().reshape(-1), gw.numpy()) <= 1e-9
    infr.params.zero_grad()
    post = np.linalg.solve(np.linalg.inv(P0) + 200 * np.linalg.inv(Sigma), np.linalg.inv(Sigma) @ Y.sum(0))
    infr.run(Y=Yd, max_iter=30, learning_rate=0.1)
    after = infr.params[loc].detach().cpu().numpy().reshape(-1)
    end, _ = infr.create_executor()(Yd)
    assert float(end) < float(loss)
    assert np.linalg.norm(after - post) < np.linalg.norm(m0 - post)


def test_map_gradient_with_respect_to_cholesky_parameters():
    """Sigma = L L^T with L's six entries under inference (softplus diagonal): d loss / d theta at the start matches CPU autograd to 1e-8"""
    m, alg, infr, Yd, (P0, _, Y, m0, theta0) = _mvn_model(True)
    th = torch.as_tensor(theta0).requires_grad_(True)
    L = _lower(th)
    want = -_closed_form(torch.as_tensor(m0), L @ L.T, P0, Y)
    gw, = torch.autograd.grad(want, th)
    loss, loss_for_gradient = infr.create_executor()(Yd)
    assert abs(float(loss) - float(want)) <= 1e-9 * abs(float(want))
    loss_for_gradient.backward()
    assert nerr(infr.params.grad(m.theta).cpu().numpy().reshape(-1), gw.numpy()) <= 1e-8
