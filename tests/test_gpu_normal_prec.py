"""NormalMeanPrecision on the MI355X: kind 'normal_prec' of the univariate kernels (mxf_univariate_logpdf*, all five entry points) and the
draw by mean and precision (mxf_normal_reparam_prec*) through the tensor wrappers, the class through the API on the reference's cases
(testing/components/distributions/normal_mean_precision_test.py), and the Gamma-prior-on-precision regression under MAP.

Expected values are scipy.stats.norm.logpdf(x, a, b ** -0.5) in float64, expected gradients float64 CPU autograd of the formula
(_transform_ref.py).  Tolerances.  float64: 1e-9 relative to the sum of the magnitudes of the addends of the formula a result comes from
(a reduced value or gradient: summed over what it is reduced over).  float32: rtol 1e-4, atol 1e-5, the bar of
tests/test_gpu_normal.py; every float32 case first asserts that the same formula in float32 on the CPU meets that bar on its inputs.

Inputs: precisions log-uniform over 1e-3 .. 1e3; x = a + z / sqrt(b) with |z| in [0.2, 0.8] and one sign per element, 4 in 5 positive, so that
neither 1/b - d^2 nor a sum over samples or elements cancels (the float32 bar is relative to the result)."""
import numpy as np
import pytest
import torch
from scipy import stats

import _transform_ref as R
from _transform_ref import check, dev, rounded, tdt

pytestmark = pytest.mark.gpu

BIG = 512 * 256 + 3            # the reduced launch is capped at 512 workgroups of 256: the grid-stride loop takes a second trip
PREFILL = 0.75
WORST = {}                     # the largest error of the module as a fraction of its bound, per dtype


@pytest.fixture(scope='module', autouse=True)
def _report_worst_errors():
    """after the module: the largest error its checks saw, per dtype, as a fraction of the bound (shown with -s)"""
    yield
    for dtype, (frac, err, what) in sorted(WORST.items()):
        print('normal_prec worst %s: %.3e absolute, %.3f of its bound (%s)' % (dtype, err, frac, what))


def make_inputs(n, S, la, lb, dtype, seed=0):
    """x (S, n); a, b in the layouts la, lb: 'one' (1,), 'elem' (n,), 'samp' (S, n); float64 holding values of `dtype`"""
    r = np.random.RandomState(seed + 17 * n + S)
    shape = {'one': (1,), 'elem': (n,), 'samp': (S, n)}
    a = rounded(r.randn(*shape[la]), dtype)
    b = rounded(10.0 ** r.uniform(-3, 3, shape[lb]), dtype)
    b.reshape(-1)[0], b.reshape(-1)[-1] = (1e-3, 1e3) if b.size > 1 else (b.reshape(-1)[0],) * 2
    b = rounded(b, dtype)
    z = r.uniform(0.2, 0.8, (S, n)) * np.where(r.rand(n) < 0.8, 1.0, -1.0)
    x = rounded(np.broadcast_to(a, (S, n)) + z / np.sqrt(np.broadcast_to(b, (S, n))), dtype)
    return x, a, b


def reduce_to(g, layout):
    """per-(s, i) terms -> what a parameter of that layout receives"""
    return g.sum().reshape(1) if layout == 'one' else (g.sum(0) if layout == 'elem' else g)


def expected(x, a, b, la, lb, w, dtype):
    """log p (S, n) from scipy and {dx, da, db}: (value, magnitude) in the parameters' layouts, for the weights w; float32: the inputs are
    first shown to be fair"""
    S, n = x.shape
    A, B = np.broadcast_to(a, (S, n)), np.broadcast_to(b, (S, n))
    lp = stats.norm.logpdf(x, A, B ** -0.5)
    lp_t, g = R.normal_prec_reference(x, A, B, w)
    assert np.allclose(lp_t, lp, rtol=1e-12, atol=1e-12)                    # the restated formula is scipy's
    mag = R.normal_prec_magnitudes(x, A, B, w)
    out = {'lp': (lp, mag[0]), 'dx': (g[0], mag[1]), 'da': (reduce_to(g[1], la), reduce_to(mag[2], la)),
           'db': (reduce_to(g[2], lb), reduce_to(mag[3], lb))}
    if dtype == 'float32':
        lp32, g32 = R.normal_prec_reference(x, A, B, w, dtype=torch.float32)
        assert np.allclose(lp32, lp, rtol=R.F32_RTOL, atol=R.F32_ATOL), 'the float32 inputs cancel in log p'
        for t32, key, lay in ((g32[0], 'dx', 'samp'), (g32[1], 'da', la), (g32[2], 'db', lb)):
            assert np.allclose(reduce_to(t32.astype(np.float32), lay), out[key][0], rtol=R.F32_RTOL, atol=R.F32_ATOL), \
                'the float32 inputs cancel in ' + key
    return out


def fair_sum(vals, want, dtype):
    """float32: the sum in float32 on the CPU meets the bar"""
    if dtype == 'float32':
        got = torch.as_tensor(vals, dtype=torch.float32).sum(-1).double().numpy()
        assert np.allclose(got, want, rtol=R.F32_RTOL, atol=R.F32_ATOL), 'the float32 inputs cancel in the sum'


ONE_OR_ELEM = [('one', 'one'), ('one', 'elem'), ('elem', 'one'), ('elem', 'elem')]


@pytest.mark.parametrize('n, lay', [(1, ('one', 'one'))] + [(n, c) for n in (3, 257, BIG) for c in ONE_OR_ELEM], ids=str)
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_reduced_kernel_value_gradients_and_accumulation(dtype, S, n, lay):
    """mxf_univariate_logpdf: out, dx, da, db come back as prefill + expected; accumulators behind NULL pointers are not touched and do not
    change the others (NULL in each position up to n = 257; at the large n all pointers, and out alone)."""
    from mxfusion_amd import ops
    la, lb = lay
    x, a, b = make_inputs(n, S, la, lb, dtype)
    scale = 0.5 / S
    want = expected(x, a, b, la, lb, scale, dtype)
    total = (scale * want['lp'][0].sum(), abs(scale) * want['lp'][1].sum())
    fair_sum(scale * want['lp'][0].reshape(-1), total[0], dtype)
    masks = [(True,) * 4] + ([(True, False, False, False)] if n == BIG else [tuple(j != i for j in range(4)) for i in range(4)])
    for mask in masks:
        bufs = [torch.full(s, PREFILL, dtype=tdt(dtype)).cuda() for s in ((1,), x.shape, a.shape, b.shape)]
        ops.univariate_logpdf_('normal_prec', dev(x, dtype), dev(a, dtype), dev(b, dtype), scale, *[t if m else None for t, m in zip(bufs, mask)])
        torch.cuda.synchronize()
        for t, m, key in zip(bufs, mask, ('out', 'dx', 'da', 'db')):
            if not m:
                assert bool((t == PREFILL).all()), '%s was not handed over and changed' % key
                continue
            val, mag = total if key == 'out' else want[key]
            check(t - PREFILL, val, mag + PREFILL, dtype, 'reduced %s %s' % (key, mask), WORST)


LAYOUTS = ('one', 'elem', 'samp')
ELEM_CASES = [(1, ('one', 'one')), (1, ('samp', 'samp'))] + [(n, (p, q)) for n in (3, 257) for p in LAYOUTS for q in LAYOUTS] + \
    [(BIG, ('elem', 'samp')), (BIG, ('samp', 'one'))]


@pytest.mark.parametrize('n, lay', ELEM_CASES, ids=str)
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_elementwise_and_per_sample_kernels_with_their_reverse_modes(dtype, S, n, lay):
    """mxf_univariate_logpdf_elem / _bwd (a cotangent per sample and element) and mxf_univariate_logpdf_ps / _ps_bwd (the per-sample sums
    and their weighted reverse mode): each parameter a single element, per element, or per sample and element; prefilled accumulators."""
    from mxfusion_amd import ops
    la, lb = lay
    scale = 1.5
    x, a, b = make_inputs(n, S, la, lb, dtype, seed=3)
    r = np.random.RandomState(5)
    xd, ad, bd = dev(x, dtype), dev(a, dtype), dev(b, dtype)
    cot, w = rounded(r.uniform(0.5, 1.5, (S, n)), dtype), rounded(r.uniform(0.5, 1.5, (S,)), dtype)

    want = expected(x, a, b, la, lb, scale * cot, dtype)
    got = ops.univariate_logpdf_elem('normal_prec', xd, ad, bd, scale)
    assert got.shape == xd.shape and got.dtype == tdt(dtype)
    check(got, scale * want['lp'][0], scale * want['lp'][1], dtype, 'elem log p', WORST)
    bufs = [torch.full(t.shape, PREFILL, dtype=tdt(dtype)).cuda() for t in (x, a, b)]
    ops.univariate_logpdf_bwd_('normal_prec', xd, ad, bd, dev(cot, dtype), scale, *bufs)
    torch.cuda.synchronize()
    for t, key in zip(bufs, ('dx', 'da', 'db')):
        check(t - PREFILL, want[key][0], want[key][1] + PREFILL, dtype, 'elem reverse ' + key, WORST)
    only_b = torch.full(b.shape, PREFILL, dtype=tdt(dtype)).cuda()             # null dx and da
    ops.univariate_logpdf_bwd_('normal_prec', xd, ad, bd, dev(cot, dtype), scale, None, None, only_b)
    check(only_b - PREFILL, want['db'][0], want['db'][1] + PREFILL, dtype, 'elem reverse db alone', WORST)

    want = expected(x, a, b, la, lb, scale * w[:, None], dtype)
    sums = (scale * want['lp'][0].sum(1), scale * want['lp'][1].sum(1))
    fair_sum(scale * want['lp'][0], sums[0], dtype)
    out = torch.full((S,), PREFILL, dtype=tdt(dtype)).cuda()
    ops.logpdf_per_sample_('normal_prec', xd, ad, bd, scale, out)
    check(out - PREFILL, sums[0], sums[1] + PREFILL, dtype, 'per-sample sums', WORST)
    bufs = [torch.full(t.shape, PREFILL, dtype=tdt(dtype)).cuda() for t in (x, a, b)]
    ops.logpdf_per_sample_bwd_('normal_prec', xd, ad, bd, dev(w, dtype), scale, *bufs)
    torch.cuda.synchronize()
    for t, key in zip(bufs, ('dx', 'da', 'db')):
        check(t - PREFILL, want[key][0], want[key][1] + PREFILL, dtype, 'per-sample reverse ' + key, WORST)
    only_a = torch.full(a.shape, PREFILL, dtype=tdt(dtype)).cuda()             # null dx and db
    ops.logpdf_per_sample_bwd_('normal_prec', xd, ad, bd, dev(w, dtype), scale, None, only_a, None)
    check(only_a - PREFILL, want['da'][0], want['da'][1] + PREFILL, dtype, 'per-sample reverse da alone', WORST)


def test_kind_out_of_range_is_status_minus_two():
    from mxfusion_amd import _lib
    x = torch.ones(2, 5, dtype=torch.float64).cuda()
    out = torch.zeros(1, dtype=torch.float64).cuda()
    h, lib = _lib.handle(torch.cuda.current_device()), _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    args = (_lib.F64, 2, 5, x.data_ptr(), x.data_ptr(), 1, x.data_ptr(), 1, 1.0, out.data_ptr(), None, None, None, st)
    assert lib.mxf_univariate_logpdf(h, 7, *args) == -2 and lib.mxf_univariate_logpdf(h, -1, *args) == -2
    assert lib.mxf_univariate_logpdf(h, _lib.D_NORMAL_PREC, *args) == 0
    torch.cuda.synchronize()
    assert abs(float(out[0]) - 10 * (-0.5 * R.LOG2PI)) < 1e-12


# ---- the draw ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 257, 2048 * 256 + 3], ids=str)
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_reparam_kernels(dtype, S, n):
    """mxf_normal_reparam_prec / _bwd against numpy: x = mean + eps / sqrt(precision); dmean += sum_s dx, dprecision += -1/2 sum_s dx eps
    precision^(-3/2), added into prefilled buffers, either of which may be null.  dx and eps are positive: the sums do not cancel."""
    from mxfusion_amd import ops
    r = np.random.RandomState(n + S)
    mean, prec = rounded(r.randn(n), dtype), rounded(10.0 ** r.uniform(-3, 3, n), dtype)
    eps, dx = rounded(r.uniform(0.2, 2.0, (S, n)), dtype), rounded(r.uniform(0.5, 1.5, (S, n)), dtype)
    got = ops.normal_reparam_prec(dev(mean, dtype), dev(prec, dtype), dev(eps, dtype))
    assert got.shape == (S, n) and got.dtype == tdt(dtype)
    check(got, mean + eps * prec ** -0.5, np.abs(mean) + eps * prec ** -0.5, dtype, 'draw', WORST)
    want_m, want_p = dx.sum(0), -0.5 * (dx * eps).sum(0) * prec ** -1.5
    dm, dp = [torch.full((n,), PREFILL, dtype=tdt(dtype)).cuda() for _ in range(2)]
    ops.normal_reparam_prec_bwd_(dev(prec, dtype), dev(eps, dtype), dev(dx, dtype), dm, dp)
    check(dm - PREFILL, want_m, want_m + PREFILL, dtype, 'draw dmean', WORST)
    check(dp - PREFILL, want_p, np.abs(want_p) + PREFILL, dtype, 'draw dprecision', WORST)
    for null in (0, 1):
        bufs = [torch.full((n,), PREFILL, dtype=tdt(dtype)).cuda() for _ in range(2)]
        ops.normal_reparam_prec_bwd_(dev(prec, dtype), dev(eps, dtype), dev(dx, dtype), *[None if i == null else t for i, t in enumerate(bufs)])
        torch.cuda.synchronize()
        assert bool((bufs[null] == PREFILL).all())
        check(bufs[1 - null] - PREFILL, (want_p, want_m)[null], np.abs((want_p, want_m)[null]) + PREFILL, dtype, 'draw reverse, one null', WORST)
    with pytest.raises(ValueError):
        ops.normal_reparam_prec(dev(mean, dtype)[:0], dev(prec, dtype), dev(eps, dtype))


# ---- the class, on the reference's cases -------------------------------------------------------------------------------------------------

def _factor(dtype, **kw):
    from mxfusion_amd.components.distributions import NormalMeanPrecision
    return NormalMeanPrecision.define_variable(shape=(3, 2), dtype=dtype, **kw).factor


def _axis(t, sampled, dtype):
    t = dev(t, dtype)
    return t if sampled else t[None]


@pytest.mark.parametrize('dtype, mean_s, prec_s, rv_s', [('float64', True, False, True), ('float64', False, True, True),
                                                         ('float64', False, False, True), ('float64', False, False, False),
                                                         ('float32', True, False, True)])
def test_log_pdf(dtype, mean_s, prec_s, rv_s):
    """normal_mean_precision_test.py:30-69, with the reverse mode added"""
    r = np.random.RandomState(0)
    sh = lambda s: ((5,) if s else ()) + (3, 2)
    mean, prec, rv = rounded(r.rand(*sh(mean_s)), dtype), rounded(r.rand(*sh(prec_s)) + 0.1, dtype), rounded(r.rand(*sh(rv_s)), dtype)
    f = _factor(dtype)
    variables = {f.mean.uuid: _axis(mean, mean_s, dtype), f.precision.uuid: _axis(prec, prec_s, dtype),
                 f.random_variable.uuid: _axis(rv, rv_s, dtype)}
    leaves = [t.requires_grad_(True) for t in variables.values()]
    got = f.log_pdf(F=None, variables=variables)
    any_s = mean_s or prec_s or rv_s
    assert got.dtype == tdt(dtype) and got.shape == ((5 if any_s else 1), 3, 2)
    full = lambda t, s: np.broadcast_to(t if s else t[None], got.shape).reshape(got.shape[0], -1)
    A, B, X = full(mean, mean_s), full(prec, prec_s), full(rv, rv_s)
    want = stats.norm.logpdf(X, A, B ** -0.5)
    rtol, atol = (1e-7, 1e-10) if dtype == 'float64' else (1e-4, 1e-5)          # the reference's own tolerances
    assert np.allclose(got.detach().double().cpu().numpy().reshape(want.shape), want, rtol=rtol, atol=atol)
    cot = np.random.RandomState(6).uniform(0.5, 1.5, want.shape)
    mag = R.normal_prec_magnitudes(X, A, B, cot)
    check(got, want, mag[0], dtype, 'class log p', WORST)
    g = R.normal_prec_reference(X, A, B, cot)[1]
    (got * dev(cot, dtype).reshape(got.shape)).sum().backward()
    for leaf, gp, mg, s, key in zip(leaves, (g[1], g[2], g[0]), (mag[2], mag[3], mag[1]), (mean_s, prec_s, rv_s), ('dmean', 'dprecision', 'dx')):
        keep = s or not any_s                       # a leaf without the sample axis receives the sum over the samples
        if dtype == 'float32':
            g32 = R.normal_prec_reference(X, A, B, cot, dtype=torch.float32)[1][{'dmean': 1, 'dprecision': 2, 'dx': 0}[key]]
            assert np.allclose(g32 if keep else g32.astype(np.float32).sum(0, keepdims=True), gp if keep else gp.sum(0, keepdims=True),
                               rtol=R.F32_RTOL, atol=R.F32_ATOL), 'the float32 inputs cancel in ' + key
        check(leaf.grad.reshape(-1), (gp if keep else gp.sum(0, keepdims=True)).reshape(-1),
              (mg if keep else mg.sum(0, keepdims=True)).reshape(-1), dtype, 'class ' + key, WORST)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_log_pdf_broadcasts_single_element_parameters_and_applies_the_scaling(dtype):
    """mean and precision of one element against a (5, 3, 2) variable, through log_pdf, log_pdf_sum and log_pdf_per_sample;
    normal.py:283 multiplies by log_pdf_scaling"""
    r = np.random.RandomState(1)
    rv = rounded(r.rand(5, 3, 2), dtype)
    f = _factor(dtype)
    want = stats.norm.logpdf(rv, 0.25, 2.0 ** -0.5)
    bar = dict(rtol=1e-9, atol=1e-12) if dtype == 'float64' else dict(rtol=R.F32_RTOL, atol=R.F32_ATOL)
    for scaling in (1.0, 3.0):
        f.log_pdf_scaling = scaling
        variables = {f.mean.uuid: dev([[[0.25]]], dtype), f.precision.uuid: dev([[[2.0]]], dtype), f.random_variable.uuid: dev(rv, dtype)}
        assert np.allclose(f.log_pdf(F=None, variables=variables).double().cpu().numpy(), scaling * want, **bar)
        assert np.allclose(float(f.log_pdf_sum(None, variables)), scaling * want.mean(0).sum(), **bar)
        assert np.allclose(f.log_pdf_per_sample(None, variables).double().cpu().numpy(), scaling * want.reshape(5, -1).sum(1), **bar)
    full = {f.mean.uuid: dev(np.full((1, 3, 2), 0.25), dtype), f.precision.uuid: dev(np.full((1, 3, 2), 2.0), dtype),
            f.random_variable.uuid: dev(rv, dtype)}
    assert np.allclose(float(f.log_pdf_sum(None, full)), 3.0 * want.mean(0).sum(), **bar)


@pytest.mark.parametrize('dtype, mean_s, prec_s', [('float64', True, False), ('float64', False, True), ('float64', False, False),
                                                   ('float64', True, True), ('float32', True, False), ('float32', False, False)])
def test_draw_samples(dtype, mean_s, prec_s, monkeypatch):
    """normal_mean_precision_test.py:71-110 with MockRandomGenerator noise, and the gradients in both parameters; the kernel draws where
    neither parameter carries samples, the torch expression otherwise"""
    from mxfusion_amd import ops
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    calls = []
    real = ops.normal_reparam_prec
    monkeypatch.setattr(ops, 'normal_reparam_prec', lambda *a: (calls.append(1), real(*a))[1])
    r = np.random.RandomState(2)
    sh = lambda s: ((5,) if s else ()) + (3, 2)
    mean, prec = rounded(r.rand(*sh(mean_s)), dtype), rounded(r.rand(*sh(prec_s)) + 0.1, dtype)
    rand = rounded(r.uniform(0.2, 2.0, (5, 3, 2)), dtype)
    f = _factor(dtype, rand_gen=MockRandomGenerator(dev(rand.reshape(-1), dtype)))
    variables = {f.mean.uuid: _axis(mean, mean_s, dtype), f.precision.uuid: _axis(prec, prec_s, dtype)}
    leaves = [t.requires_grad_(True) for t in variables.values()]
    got = f.draw_samples(F=None, variables=variables, num_samples=5)
    assert got.dtype == tdt(dtype) and got.shape == (5, 3, 2)
    assert len(calls) == (0 if mean_s or prec_s else 1)
    M, P = (mean if mean_s else mean[None]), (prec if prec_s else prec[None])
    want = M + rand * P ** -0.5
    rtol, atol = (1e-7, 1e-10) if dtype == 'float64' else (1e-4, 1e-5)
    assert np.allclose(got.detach().double().cpu().numpy(), want, rtol=rtol, atol=atol)
    check(got, want, np.abs(M) + rand * P ** -0.5, dtype, 'class draw', WORST)
    cot = rounded(np.random.RandomState(3).uniform(0.5, 1.5, (5, 3, 2)), dtype)
    (got * dev(cot, dtype)).sum().backward()
    gm, gp = cot + 0 * M, -0.5 * cot * rand * P ** -1.5
    for leaf, g, s, key in ((leaves[0], gm, mean_s, 'dmean'), (leaves[1], gp, prec_s, 'dprecision')):
        g = g if s else g.sum(0, keepdims=True)
        check(leaf.grad, g, np.abs(g), dtype, 'class draw ' + key, WORST)


# ---- the conjugate model under MAP -------------------------------------------------------------------------------------------------------

N, D = 20, 3


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_gamma_prior_on_the_precision_under_map(dtype):
    """tau ~ Gamma(2, 1), y ~ NormalMeanPrecision(dot(x, w), broadcast_to(tau, (N, 1))), N = 20, a softplus-constrained location for tau:
    the initial loss and every gradient against the float64 CPU restatement (float64 at the float64 bar, float32 at the float32 bar, the
    restatement in float32 first held to it), then 5 Adam steps against the oracle's Adam rule."""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Gamma, NormalMeanPrecision
    from mxfusion_amd.components.functions.operators import broadcast_to, dot
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.inference import GradBasedInference, MAP
    from oracle import gp_oracle as O
    r = np.random.RandomState(0)
    x = rounded(r.randn(N, D), dtype)
    w_true = np.array([[0.7], [-1.2], [0.4]])
    y = rounded(x @ w_true + 0.5 * r.randn(N, 1), dtype)
    w0, tau0 = rounded([[0.1], [-0.2], [0.3]], dtype), 1.5
    m = Model()
    m.N = Variable()
    m.x = Variable(shape=(m.N, D))
    m.w = Variable(shape=(D, 1), initial_value=dev(w0, dtype))
    m.tau = Gamma.define_variable(alpha=2., beta=1., shape=(1,), dtype=dtype)
    m.y = NormalMeanPrecision.define_variable(mean=dot(m.x, m.w), precision=broadcast_to(m.tau, (m.N, 1)), shape=(m.N, 1), dtype=dtype)
    loc = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=dev([tau0], dtype))
    alg = MAP(model=m, observed=[m.x, m.y], locations={m.tau: loc})
    infr = GradBasedInference(inference_algorithm=alg, dtype=dtype)
    infr.initialize(x=dev(x, dtype), y=dev(y, dtype))

    def cpu_loss(raw, dt=torch.float64):
        tau = torch.nn.functional.softplus(raw['tau'].to(dt))
        mean = torch.as_tensor(x, dtype=dt) @ raw['w'].to(dt)
        lik = R.normal_prec_logpdf(torch.as_tensor(y, dtype=dt), mean, tau.reshape(1, 1).expand(N, 1)).sum()
        return -(lik + R.gamma_logpdf(tau, 2.0, 1.0).sum())

    raw = {'w': torch.as_tensor(w0), 'tau': infr.params.raw(loc).detach().double().cpu().reshape(1)}
    assert abs(float(torch.nn.functional.softplus(raw['tau'])) - tau0) < (1e-12 if dtype == 'float64' else 1e-6)
    lv = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    want = cpu_loss(lv)
    want.backward()
    # the magnitude the float64 bar is relative to: the likelihood's and the prior's addends
    tau_v = float(torch.nn.functional.softplus(raw['tau']))
    resid = y - x @ w0
    mloss = N * (0.5 * abs(np.log(tau_v)) + 0.5 * R.LOG2PI) + 0.5 * tau_v * float((resid ** 2).sum()) + abs(np.log(tau_v)) + tau_v
    if dtype == 'float32':
        l32 = {k: v.float().clone().requires_grad_(True) for k, v in raw.items()}
        loss32 = cpu_loss(l32, torch.float32)
        loss32.backward()
        assert np.allclose(float(loss32.detach()), float(want.detach()), rtol=R.F32_RTOL, atol=R.F32_ATOL)
        for k in raw:
            assert np.allclose(l32[k].grad.double().numpy(), lv[k].grad.numpy(), rtol=R.F32_RTOL, atol=R.F32_ATOL), k
    loss, loss_for_gradient = infr.create_executor()(dev(x, dtype), dev(y, dtype))
    check(loss.reshape(1), [float(want.detach())], mloss, dtype, 'MAP loss', WORST)
    loss_for_gradient.backward()
    chain = float(torch.sigmoid(raw['tau']))                         # d tau / d raw: the gradient under test is the raw location's
    gmag = {'w': tau_v * (np.abs(x)[:, :, None] * np.abs(resid)[:, None, :]).sum(0),
            'tau': chain * np.array([N * 0.5 / tau_v + 0.5 * float((resid ** 2).sum()) + 1 / tau_v + 1.0])}
    for k, v in (('w', m.w), ('tau', loc)):
        check(infr.params.grad(v).reshape(-1), lv[k].grad.numpy().reshape(-1), gmag[k].reshape(-1), dtype, 'MAP gradient ' + k, WORST)
    infr.params.zero_grad()

    infr.run(x=dev(x, dtype), y=dev(y, dtype), max_iter=5, learning_rate=0.05)
    opt = O.MXNetAdam(0.05)
    for _ in range(5):
        lv = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
        cpu_loss(lv).backward()
        raw = opt.step({k: v.detach() for k, v in lv.items()}, {k: v.grad for k, v in lv.items()}, batch_size=1)
    end = {'w': raw['w'].numpy(), 'tau': torch.nn.functional.softplus(raw['tau']).numpy()}
    for k, v in (('w', m.w), ('tau', loc)):
        got = infr.params[v].double().cpu().numpy().reshape(end[k].shape)
        if dtype == 'float64':
            assert np.allclose(got, end[k], rtol=1e-9, atol=0), (k, got, end[k])
        else:
            assert np.allclose(got, end[k], rtol=R.F32_RTOL, atol=R.F32_ATOL), (k, got, end[k])
    assert abs(float(end['tau'][0]) - tau0) > 1e-3                      # the steps moved the parameters
