"""Logistic and the segmented transformation kernel (mxf_transform_fwd / _bwd, transform.hip) on the MI355X: the reference's
test_logistic cases (testing/components/variables/var_trans_test.py:57-68), the kernel against float64 numpy (_transform_ref.py), one
batched call for the Logistic and offset-softplus members of transform_many, and a bounded parameter through MAP and a checkpoint.

Tolerances.  float64: 1e-9 relative to the sum of the magnitudes of the addends (|lower| + (upper - lower) sigmoid for a value, the slope
itself for a derivative: DESIGN.md section 2).  float32: rtol 1e-4, atol 1e-5, the bar of tests/test_gpu_normal.py; every float32 case first
asserts that the same formula in float32 on the CPU meets that bar on its inputs."""
import numpy as np
import pytest
import torch

import _transform_ref as R
from _transform_ref import check, dev, rounded, tdt

pytestmark = pytest.mark.gpu

BOUNDS = [(0., 1.), (-2., 3.), (1e-6, 1e-2), (1., 200000.)]
WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst_errors():
    """after the module: the largest error its checks saw, per dtype, as a fraction of the bound (shown with -s)"""
    yield
    for dtype, (frac, err, what) in sorted(WORST.items()):
        print('logistic worst %s: %.3e absolute, %.3f of its bound (%s)' % (dtype, err, frac, what))


def _count(monkeypatch, *names):
    """call counters on the named ops wrappers"""
    from mxfusion_amd import ops
    calls = {n: 0 for n in names}
    for n in names:
        def counted(*a, _real=getattr(ops, n), _n=n, **kw):
            calls[_n] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, n, counted)
    return calls


@pytest.mark.parametrize('x, lower, upper, dtype, rtol, atol', [(10., 2, 20, 'float64', 1e-7, 1e-10), (1e-3, 1e-6, 1e-2, 'float64', 1e-7, 1e-10),
                                                                 (1., 1, 200000, 'float32', 1e-4, 1e-5), (5., 2, 10000, 'float32', 1e-4, 1e-5)])
def test_logistic_round_trip_reference_cases(x, lower, upper, dtype, rtol, atol):
    from mxfusion_amd.components.variables import Logistic
    t = Logistic(lower, upper)
    xt = dev([x], dtype)
    y = t.transform(xt)
    inv = t.inverseTransform(y)
    assert y.dtype == tdt(dtype) and inv.dtype == xt.dtype and inv.is_cuda
    assert lower <= float(y) <= upper
    assert np.isclose(float(xt), float(inv), rtol=rtol, atol=atol)


def _grid(dtype):
    return rounded(np.concatenate([np.linspace(-40., 40., 321), [-800., 800.] if dtype == 'float64' else [-100., 100.]]), dtype)


@pytest.mark.parametrize('lower, upper', BOUNDS, ids=str)
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_kernel_value_and_derivative_against_numpy(dtype, lower, upper):
    from mxfusion_amd.components.variables import Logistic
    x = _grid(dtype)
    want, slope = R.logistic(x, lower, upper), R.logistic_slope(x, lower, upper)
    cot = rounded(np.random.RandomState(0).uniform(0.5, 1.5, x.shape), dtype)
    if dtype == 'float32':
        x32, lo32, hi32 = x.astype(np.float32), np.float32(lower), np.float32(upper)
        assert np.allclose(R.logistic(x32, lo32, hi32), want, rtol=R.F32_RTOL, atol=R.F32_ATOL), 'the float32 inputs cancel in the value'
        assert np.allclose(cot.astype(np.float32) * R.logistic_slope(x32, lo32, hi32), cot * slope, rtol=R.F32_RTOL, atol=R.F32_ATOL), \
            'the float32 inputs cancel in the derivative'
    xd = dev(x, dtype).requires_grad_(True)
    y = Logistic(lower, upper).transform(xd)
    assert y.dtype == tdt(dtype) and y.shape == xd.shape
    (y * dev(cot, dtype)).sum().backward()
    torch.cuda.synchronize()
    yv, gv = y.detach().double().cpu().numpy(), xd.grad.double().cpu().numpy()
    assert np.isfinite(yv).all() and np.isfinite(gv).all()
    assert (yv >= lower).all() and (yv <= upper).all(), (yv.min() - lower, yv.max() - upper)
    check(y, want, abs(lower) + (upper - lower) * R.sigmoid(x), dtype, 'logistic value %s' % ((lower, upper),), WORST)
    check(xd.grad, cot * slope, cot * slope, dtype, 'logistic derivative %s' % ((lower, upper),), WORST)
    assert gv[-2] == 0.0 and gv[-1] == 0.0, gv[-2:]                     # the extreme x: exactly 0, not NaN
    lo_t, hi_t = lower, upper                                           # the bounds rounded inwards to the working dtype
    if dtype == 'float32':
        lo_t, hi_t = np.float32(lower), np.float32(upper)
        lo_t = np.nextafter(lo_t, np.float32(np.inf)) if float(lo_t) < lower else lo_t
        hi_t = np.nextafter(hi_t, np.float32(-np.inf)) if float(hi_t) > upper else hi_t
    assert yv[-2] == float(lo_t) and yv[-1] == float(hi_t), (yv[-2:], lo_t, hi_t)      # saturated: the bound itself
    assert (np.diff(yv[:-2]) >= 0).all()                                # monotone over the grid


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_raw_entry_points_accumulate_and_refuse_bad_tables(dtype):
    """ops.transform / transform_bwd_ on a two-segment buffer with a prefilled accumulator and an empty segment in the middle; a bad kind, a
    negative size, an empty interval and sizes that do not add up are refused before anything is launched"""
    from mxfusion_amd import _lib, ops
    x = rounded(np.linspace(-5., 5., 300), dtype)
    segs = [('softplus', 43, 0.5, 0.), ('logistic', 0, 0., 1.), ('logistic', 257, -2., 5.)]
    want = np.concatenate([R.softplus(x[:43], 0.5), R.logistic(x[43:], -2., 3.)])
    slope = np.concatenate([R.sigmoid(x[:43]), R.logistic_slope(x[43:], -2., 3.)])
    xd = dev(x, dtype)
    mag = np.concatenate([R.softplus(x[:43]) + 0.5, 2. + 5. * R.sigmoid(x[43:])])
    check(ops.transform(segs, xd), want, mag, dtype, 'two segments', WORST)
    dy = rounded(np.random.RandomState(1).uniform(0.5, 1.5, x.shape), dtype)
    acc = torch.full(x.shape, 0.75, dtype=tdt(dtype)).cuda()
    ops.transform_bwd_(segs, xd, dev(dy, dtype), acc)
    check(acc - 0.75, dy * slope, dy * slope + 0.75, dtype, 'two segments, reverse', WORST)
    y = torch.full(x.shape, 7.0, dtype=tdt(dtype)).cuda()
    lib, h, st = _lib.load(), _lib.handle(torch.cuda.current_device()), torch.cuda.current_stream().cuda_stream
    arr = lambda ct, v: (ct * len(v))(*v)
    import ctypes as C
    for kinds, sizes, p0, p1 in (([0, 2], [43, 257], [0., 0.], [0., 1.]), ([0, 1], [43, -1], [0., 0.], [0., 1.]),
                                 ([0, 1], [43, 257], [0., 0.], [0., 0.]), ([0, 1], [43, 257], [0., 0.], [0., float('nan')]),
                                 ([0, 1], [43, 257], [float('inf'), 0.], [0., 1.])):
        rc = lib.mxf_transform_fwd(h, _lib.F32 if dtype == 'float32' else _lib.F64, 2, arr(C.c_int, kinds), arr(C.c_int64, sizes),
                                   arr(C.c_double, p0), arr(C.c_double, p1), xd.data_ptr(), y.data_ptr(), st)
        assert rc == -2 and b'mxf_transform_fwd' in lib.mxf_last_error(h)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                       # nothing was written
    with pytest.raises(ValueError):
        ops.transform(segs[:2], xd)
    with pytest.raises(ValueError):
        ops.transform([('logistic', 300, 0., 1.)], xd.reshape(30, 10).t())


def _alone(t, x, cot):
    leaf = x.clone().requires_grad_(True)
    y = t.transform(leaf)
    if cot is not None:
        (y * cot).sum().backward()
    return y.detach(), leaf.grad


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_transform_many_batches_the_mixed_list_into_one_call_each_way(dtype, monkeypatch):
    """plain softplus, Softplus(0.5), Logistic(0, 1), Logistic(-2, 3), each at the sizes 1, 255, 256, 257 and 1000 (segment ends inside and
    on workgroup boundaries): every result and gradient equals the one of that tensor transformed alone; one member's output is left
    unused; the 15 members that are not plain softplus take one forward and one backward call."""
    from mxfusion_amd.components.variables import Logistic, PositiveTransformation, Softplus
    from mxfusion_amd.components.variables.var_trans import transform_many
    r = np.random.RandomState(4)
    members = [(t, n) for n in (1, 255, 256, 257, 1000) for t in (PositiveTransformation(), Softplus(0.5), Logistic(0., 1.), Logistic(-2., 3.))]
    shape = lambda n: (n,) if n != 1000 else (10, 100)
    xs = [dev(rounded(r.uniform(-6., 6., shape(n)), dtype), dtype) for _, n in members]
    cots = [dev(rounded(r.uniform(0.5, 1.5, shape(n)), dtype), dtype) for _, n in members]
    unused = 10                                                          # Logistic(0, 1) at 256
    assert type(members[unused][0]).__name__ == 'Logistic'
    alone = [_alone(t, x, None if i == unused else c) for i, ((t, _), x, c) in enumerate(zip(members, xs, cots))]
    calls = _count(monkeypatch, 'transform', 'transform_bwd_', 'softplus', 'softplus_bwd_')
    leaves = [x.clone().requires_grad_(True) for x in xs]
    ys = transform_many([t for t, _ in members], leaves)
    assert calls == {'transform': 1, 'transform_bwd_': 0, 'softplus': 1, 'softplus_bwd_': 0}, calls
    sum((y * c).sum() for i, (y, c) in enumerate(zip(ys, cots)) if i != unused).backward()
    torch.cuda.synchronize()
    assert calls == {'transform': 1, 'transform_bwd_': 1, 'softplus': 1, 'softplus_bwd_': 1}, calls
    for i, ((t, n), y, leaf, (y1, g1)) in enumerate(zip(members, ys, leaves, alone)):
        what = '%s at %d' % (type(t).__name__, n)
        assert y.shape == xs[i].shape and y.dtype == tdt(dtype)
        exact = type(t).__name__ != 'Softplus'          # the same kernel arithmetic alone and batched; Softplus(0.5) alone adds its offset in torch
        if exact:
            assert torch.equal(y.detach(), y1), what
        check(y, y1.double().cpu().numpy(), np.abs(y1.double().cpu().numpy()) + 0.5, dtype, what, WORST)
        if i == unused:
            assert g1 is None and (leaf.grad is None or not bool(leaf.grad.any())), what
            continue
        if exact:
            assert torch.equal(leaf.grad, g1), what
        check(leaf.grad, g1.double().cpu().numpy(), np.abs(g1.double().cpu().numpy()), dtype, what + ', gradient', WORST)
    # and against numpy, so that "alone" is not the only witness
    for (t, n), x, y in zip(members, xs, ys):
        xv = x.double().cpu().numpy()
        if type(t).__name__ == 'Logistic':
            want, mag = R.logistic(xv, t._lower, t._upper), abs(t._lower) + (t._upper - t._lower) * R.sigmoid(xv)
        else:
            want, mag = R.softplus(xv, t._offset), R.softplus(xv) + abs(t._offset)
        check(y, want, mag, dtype, 'numpy, %s at %d' % (type(t).__name__, n), WORST)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_more_segments_than_one_launch_holds(dtype, monkeypatch):
    """33 Logistic tensors in one transform_many (MXF_TR_MAX_SEG = 32: the entry point launches twice): values and gradients of all"""
    from mxfusion_amd import _lib
    from mxfusion_amd.components.variables import Logistic
    from mxfusion_amd.components.variables.var_trans import transform_many
    assert _lib.TR_MAX_SEG == 32
    r = np.random.RandomState(7)
    bounds = [(0.25 * i - 4.0, 0.25 * i - 4.0 + 1.0 + i) for i in range(33)]
    sizes = [1 + (i * 7) % 11 for i in range(32)] + [300]
    xs = [rounded(r.uniform(-6., 6., n), dtype) for n in sizes]
    leaves = [dev(x, dtype).requires_grad_(True) for x in xs]
    calls = _count(monkeypatch, 'transform', 'transform_bwd_')
    ys = transform_many([Logistic(*b) for b in bounds], leaves)
    sum(y.sum() for y in ys).backward()
    torch.cuda.synchronize()
    assert calls == {'transform': 1, 'transform_bwd_': 1}, calls
    for i, ((lo, hi), x, y, leaf) in enumerate(zip(bounds, xs, ys, leaves)):
        want, slope = R.logistic(x, lo, hi), R.logistic_slope(x, lo, hi)
        if dtype == 'float32':
            x32 = x.astype(np.float32)
            assert np.allclose(R.logistic(x32, np.float32(lo), np.float32(hi)), want, rtol=R.F32_RTOL, atol=R.F32_ATOL)
            assert np.allclose(R.logistic_slope(x32, np.float32(lo), np.float32(hi)), slope, rtol=R.F32_RTOL, atol=R.F32_ATOL)
        check(y, want, abs(lo) + (hi - lo) * R.sigmoid(x), dtype, 'segment %d' % i, WORST)
        check(leaf.grad, slope, slope, dtype, 'segment %d, gradient' % i, WORST)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_a_long_segment_next_to_a_short_one(dtype):
    """2048 * 256 + 3 elements under Logistic(-2, 3) between two 1-element segments: the long segment sets the grid for all three and its
    grid-stride loop takes a second trip, each way"""
    from mxfusion_amd import ops
    n = 2048 * 256 + 3
    x = rounded(np.random.RandomState(9).uniform(-8., 8., n + 2), dtype)
    dy = rounded(np.random.RandomState(10).uniform(0.5, 1.5, n + 2), dtype)
    segs = [('softplus', 1, 0.5, 0.), ('logistic', n, -2., 5.), ('logistic', 1, 0., 1.)]
    want = np.concatenate([R.softplus(x[:1], 0.5), R.logistic(x[1:-1], -2., 3.), R.logistic(x[-1:], 0., 1.)])
    mag = np.concatenate([R.softplus(x[:1]) + 0.5, 2. + 5. * R.sigmoid(x[1:-1]), R.sigmoid(x[-1:])])
    slope = np.concatenate([R.sigmoid(x[:1]), R.logistic_slope(x[1:-1], -2., 3.), R.logistic_slope(x[-1:], 0., 1.)])
    if dtype == 'float32':
        x32 = x.astype(np.float32)
        assert np.allclose(R.logistic(x32[1:-1], np.float32(-2.), np.float32(3.)), want[1:-1], rtol=R.F32_RTOL, atol=R.F32_ATOL)
        assert np.allclose(dy[1:-1].astype(np.float32) * R.logistic_slope(x32[1:-1], np.float32(-2.), np.float32(3.)), (dy * slope)[1:-1],
                           rtol=R.F32_RTOL, atol=R.F32_ATOL)
    xd = dev(x, dtype)
    check(ops.transform(segs, xd), want, mag, dtype, 'long segment', WORST)
    acc = torch.full(x.shape, 0.75, dtype=tdt(dtype)).cuda()
    ops.transform_bwd_(segs, xd, dev(dy, dtype), acc)
    check(acc - 0.75, dy * slope, dy * slope + 0.75, dtype, 'long segment, reverse', WORST)


def test_plain_softplus_lists_make_the_calls_they_made_before(monkeypatch):
    """three plain softplus members: one batched softplus call each way and no transform call; one plain and one offset softplus (nothing
    to batch on either side): a softplus call each, as before"""
    from mxfusion_amd.components.variables import PositiveTransformation, Softplus
    from mxfusion_amd.components.variables.var_trans import transform_many
    calls = _count(monkeypatch, 'transform', 'transform_bwd_', 'softplus', 'softplus_bwd_')
    leaves = [dev(np.linspace(-2., 2., n), 'float64').requires_grad_(True) for n in (1, 5, 300)]
    ys = transform_many([PositiveTransformation(), Softplus(0.), PositiveTransformation()], leaves)
    sum(y.sum() for y in ys).backward()
    assert calls == {'transform': 0, 'transform_bwd_': 0, 'softplus': 1, 'softplus_bwd_': 1}, calls
    for leaf, y in zip(leaves, ys):
        xv = leaf.detach().cpu().numpy()
        check(y, R.softplus(xv), R.softplus(xv) + 2, 'float64', 'plain softplus')
        check(leaf.grad, R.sigmoid(xv), R.sigmoid(xv), 'float64', 'plain softplus, gradient')
    for k in calls:
        calls[k] = 0
    leaves = [dev(np.linspace(-2., 2., n), 'float64').requires_grad_(True) for n in (4, 5)]
    ys = transform_many([PositiveTransformation(), Softplus(0.5)], leaves)
    sum(y.sum() for y in ys).backward()
    assert calls == {'transform': 0, 'transform_bwd_': 0, 'softplus': 2, 'softplus_bwd_': 2}, calls
    check(ys[1], R.softplus(leaves[1].detach().cpu().numpy(), 0.5), 3.0, 'float64', 'offset softplus alone')


def _beta_model(dtype):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Bernoulli, Beta
    from mxfusion_amd.components.variables import Logistic
    from mxfusion_amd.inference import GradBasedInference, MAP
    m = Model()
    m.z = Beta.define_variable(alpha=2., beta=3., shape=(3,), dtype=dtype)
    m.y = Bernoulli.define_variable(prob_true=m.z, shape=(3,), dtype=dtype)
    loc = Variable(shape=(3,), transformation=Logistic(0., 1.), initial_value=[0.2, 0.5, 0.9])
    alg = MAP(model=m, observed=[m.y], locations={m.z: loc})
    return m, loc, GradBasedInference(inference_algorithm=alg, dtype=dtype)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_beta_latent_with_a_logistic_location_under_map(dtype):
    """z ~ Beta(2, 3) of shape (3,), y ~ Bernoulli(z), MAP with the location constrained by Logistic(0, 1): the initial loss and the gradient
    with respect to the raw location against float64 CPU autograd; after 20 Adam steps at learning rate 0.5 the location is strictly
    inside (0, 1)."""
    y = np.array([1., 0., 1.])
    m, loc, infr = _beta_model(dtype)
    infr.initialize(y=dev(y, dtype))
    raw0 = infr.params.raw(loc).detach().double().cpu().reshape(3)
    z0 = np.array([0.2, 0.5, 0.9])
    assert np.allclose(torch.sigmoid(raw0).numpy(), z0, rtol=0, atol=1e-12 if dtype == 'float64' else 1e-6)
    assert np.allclose(infr.params[loc].double().cpu().numpy(), z0, rtol=0, atol=1e-12 if dtype == 'float64' else 1e-6)

    def cpu_loss(raw, dt=torch.float64):
        z = R.logistic_t(raw.to(dt), 0., 1.)
        yt = torch.as_tensor(y, dtype=dt)
        prior = torch.distributions.Beta(torch.tensor(2., dtype=dt), torch.tensor(3., dtype=dt)).log_prob(z)
        return -(prior + yt * torch.log(z) + (1 - yt) * torch.log1p(-z)).sum()
    leaf = raw0.clone().requires_grad_(True)
    want = cpu_loss(leaf)
    want.backward()
    if dtype == 'float32':
        l32 = raw0.float().clone().requires_grad_(True)
        w32 = cpu_loss(l32, torch.float32)
        w32.backward()
        assert np.allclose(float(w32.detach()), float(want.detach()), rtol=R.F32_RTOL, atol=R.F32_ATOL)
        assert np.allclose(l32.grad.double().numpy(), leaf.grad.numpy(), rtol=R.F32_RTOL, atol=R.F32_ATOL)
    zt = torch.sigmoid(raw0).numpy()
    lbeta = float(torch.lgamma(torch.tensor(5.)) - torch.lgamma(torch.tensor(2.)) - torch.lgamma(torch.tensor(3.)))
    mloss = float((np.abs(np.log(zt)) * (1 + y) + np.abs(np.log1p(-zt)) * (2 + 1 - y) + abs(lbeta)).sum())
    mgrad = ((1 + y) / zt + (2 + 1 - y) / (1 - zt)) * zt * (1 - zt)
    loss, loss_for_gradient = infr.create_executor()(dev(y, dtype))
    check(loss.reshape(1), [float(want.detach())], mloss, dtype, 'MAP loss, Beta latent', WORST)
    loss_for_gradient.backward()
    check(infr.params.grad(loc).reshape(3), leaf.grad.numpy(), mgrad, dtype, 'MAP gradient, raw location', WORST)
    infr.params.zero_grad()
    infr.run(y=dev(y, dtype), max_iter=20, learning_rate=0.5)
    end = infr.params[loc].double().cpu().numpy()
    assert np.isfinite(end).all() and (end > 0).all() and (end < 1).all(), end
    assert np.abs(end - z0).max() > 1e-2                                 # the steps moved it


def test_logistic_parameter_survives_a_checkpoint(tmp_path):
    """a Logistic(-1, 4) parameter: stored unconstrained, as positive parameters are, and the same constrained value after a fresh
    script's load"""
    import io
    import zipfile
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Normal
    from mxfusion_amd.components.variables import Logistic
    from mxfusion_amd.inference import Inference, MAP

    def script(mu0):
        m = Model()
        m.mu = Variable(shape=(2,), transformation=Logistic(-1., 4.), initial_value=dev(mu0, 'float64'))
        m.y = Normal.define_variable(mean=m.mu, variance=dev([1.0], 'float64'), shape=(2,), dtype='float64')
        infr = Inference(MAP(model=m, observed=[m.y]), dtype='float64')
        infr.initialize(y=(2,))
        return m, infr
    m, infr = script([0.5, 3.5])
    infr.params[m.mu] = dev([-0.75, 3.9], 'float64')
    z = str(tmp_path / 'inference.zip')
    infr.save(z)
    with zipfile.ZipFile(z) as zf:
        stored = np.load(io.BytesIO(zf.read('mxnet_parameters.npz')))[m.mu.uuid]
    want = np.array([-0.75, 3.9])
    assert np.allclose(stored.reshape(-1), np.log((want + 1.) / (4. - want)), rtol=1e-12)        # unconstrained
    m2, infr2 = script([1.0, 1.0])
    infr2.load(z)
    assert torch.equal(infr.params.raw(m.mu), infr2.params.raw(m2.mu))
    got = infr2.params[m2.mu].cpu().numpy()
    assert np.allclose(got, want, rtol=1e-12) and np.array_equal(got, infr.params[m.mu].cpu().numpy())
