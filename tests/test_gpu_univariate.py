"""Gamma, GammaMeanVariance, Beta, Laplace and Uniform on the MI355X: the fused log-pdf kernels (mxf_univariate_logpdf*, univariate.hip)
through the tensor wrappers, and the classes through the API.  Expected values are scipy.stats in float64, expected gradients float64 CPU
autograd through torch.distributions -- neither shares code with the kernels.

Tolerances.  float64: 1e-9, relative to the sum of the magnitudes of the addends of the formula a result comes from
(`magnitudes`; a reduced value or gradient: summed over what it is reduced over).  float32: rtol 1e-4, atol 1e-5, the bar of
tests/test_gpu_normal.py; every float32 case first asserts that the same formula in float32 on the CPU meets that bar on its inputs."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import stats

pytestmark = pytest.mark.gpu

KINDS = ('gamma', 'gamma_mv', 'beta', 'laplace', 'uniform')
SHAPE_PARAMS = [0.05, 0.5, 1.0, 1.4616, 2.0, 5.9, 6.0, 6.1, 50.0]       # across the digamma recurrence threshold (6) and digamma's zero
BIG = 512 * 256 + 3            # the launch is capped at 512 workgroups of 256: the grid-stride loop takes a second trip


def _tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def _round(a, dtype):
    """inputs exactly representable in the dtype under test, as float64: kernel and reference see the same numbers"""
    return np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64)


def make_inputs(kind, n, S, n_a, n_b, dtype, seed=0, a0=None, b0=None):
    """x (S, n), a (n_a), b (n_b) in float64.  Per-element shape parameters cycle through SHAPE_PARAMS (float64: and 1e4); single-element
    ones default to values at which the sum over the elements does not cancel (a0, b0 override them)."""
    r = np.random.RandomState(seed + 17 * n + S)
    shapes = np.array(SHAPE_PARAMS + ([1e4] if dtype == 'float64' else []))
    u = r.uniform(0.3, 0.9, (S, n))
    if kind == 'gamma' or (kind == 'gamma_mv' and n_a == n_b):
        a = shapes[np.arange(n) % len(shapes)] if n_a == n and n > 1 else np.array([2.0 if a0 is None else a0])
        b = r.uniform(0.5, 2.0, n) if n_b == n and n > 1 else np.array([1.5 if b0 is None else b0])
        if kind == 'gamma_mv':               # the same distributions, handed over as mean a/b and variance a/b^2
            a, b = a / b, a / b ** 2
        a, b = _round(a, dtype), _round(b, dtype)
        x = _round((a if kind == 'gamma_mv' else a / b) * u, dtype)          # x below the mean
    elif kind == 'gamma_mv':                 # one of mean and variance single: alpha = m^2/v in [0.28, 10], beta = m/v in [0.5, 3.4]
        a = _round(r.uniform(0.5, 3.0, n) if n_a == n else [4.0 / 3.0], dtype)
        b = _round(a / r.uniform(0.5, 2.0, n) if n_b == n else [0.9], dtype)
        x = _round(a * u, dtype)
    elif kind == 'beta':
        a = shapes[np.arange(n) % len(shapes)] if n_a == n and n > 1 else np.array([2.0 if a0 is None else a0])
        b = shapes[(np.arange(n) + 4) % len(shapes)] if n_b == n and n > 1 else np.array([5.9 if b0 is None else b0])
        a, b, x = _round(a, dtype), _round(b, dtype), _round(r.uniform(0.05, 0.95, (S, n)), dtype)
    elif kind == 'laplace':
        a = _round(r.randn(n) if n_a == n and n > 1 else [0.3], dtype)
        b = _round(r.uniform(0.5, 2.0, n) if n_b == n and n > 1 else [1.5], dtype)
        x = _round(a + b * (2 * r.randn(S, n) + 1), dtype)
        x[0, 0] = a[0]                                        # x == location: sign(0) = 0
    else:
        a = _round(r.uniform(-1.0, -0.5, n) if n_a == n and n > 1 else [-0.5], dtype)
        b = _round(r.uniform(0.5, 2.0, n) if n_b == n and n > 1 else [1.25], dtype)
        x = _round(r.uniform(-0.45, 0.45, (S, n)), dtype)                   # inside every element's interval
        x[0, 0] = np.broadcast_to(a, (n,))[0]                 # x == low: inside
        if n > 1:
            x[-1, 1] = np.broadcast_to(b, (n,))[1]            # x == high: outside
        if n > 2:
            x[0, 2] = np.broadcast_to(a, (n,))[2] - 0.25      # x < low: outside
    x = settle_float32(kind, x, np.broadcast_to(a, (n,)), np.broadcast_to(b, (n,)), dtype)
    return x, a, b


def settle_float32(kind, x, A, B, dtype):
    """float32 inputs without catastrophic cancellation: where log p(x | A, B) is so close to zero that a few float32 roundings of its
    largest addends (lgamma(50) = 144) exceed the float32 bar, x moves down until it is not.  A, B: broadcastable against x."""
    if dtype != 'float32' or kind not in ('gamma', 'gamma_mv', 'beta'):
        return x
    for _ in range(8):
        bad = 8 * 2.0 ** -24 * magnitudes(kind, x, A, B, 1.0)[0] > 1e-4 * np.abs(scipy_logpdf(kind, x, A, B)) + 1e-5
        if not bad.any():
            break
        x = _round(np.where(bad, 0.8 * x, x), dtype)
    return x


def scipy_logpdf(kind, x, a, b):
    if kind == 'gamma':
        return stats.gamma.logpdf(x, a, scale=1.0 / b)
    if kind == 'gamma_mv':
        return stats.gamma.logpdf(x, a * a / b, scale=b / a)
    if kind == 'beta':
        return stats.beta.logpdf(x, a, b)
    if kind == 'laplace':
        return stats.laplace.logpdf(x, loc=a, scale=b)
    lp = stats.uniform.logpdf(x, loc=a, scale=b - a)
    return np.where(x == b, -np.inf, lp)          # scipy's support is closed at the top, the reference's (uniform.py:55-57) half-open


def torch_logpdf(kind, x, a, b):
    """the reference's formula through torch.distributions (any dtype, CPU), (S, n)"""
    D = torch.distributions
    if kind == 'gamma':
        return D.Gamma(a, b, validate_args=False).log_prob(x)
    if kind == 'gamma_mv':
        return D.Gamma(a * a / b, a / b, validate_args=False).log_prob(x)
    if kind == 'beta':
        return D.Beta(a, b, validate_args=False).log_prob(x)
    if kind == 'laplace':
        return D.Laplace(a, b, validate_args=False).log_prob(x)
    inside = (a <= x) & (x < b)
    lp = -torch.log(b - a) + torch.zeros_like(x)
    return torch.where(inside, lp, torch.full_like(lp, -float('inf')))


def reference(kind, x, a, b, w, dtype=torch.float64):
    """log p (S, n) and the per-(s, i) gradients of sum(w * log p) w.r.t. x, a, b, each (S, n): CPU autograd in `dtype`.  Elements outside the
    Uniform's support carry no gradient."""
    S, n = x.shape
    leaves = [torch.as_tensor(np.broadcast_to(t, (S, n)).copy(), dtype=dtype).requires_grad_(True) for t in (x, a, b)]
    lp = torch_logpdf(kind, *leaves)
    finite = torch.isfinite(lp)
    tot = (torch.where(finite, lp, torch.zeros_like(lp)) * torch.as_tensor(w, dtype=dtype)).sum()
    g = torch.autograd.grad(tot, leaves, allow_unused=True)
    g = [torch.zeros_like(lp) if t is None else torch.where(finite, t, torch.zeros_like(t)) for t in g]
    return lp.detach().double().numpy(), [t.double().numpy() for t in g]


def magnitudes(kind, x, a, b, w):
    """sum of the magnitudes of the addends of log p and of its three weighted partial derivatives, each (S, n): what a float64 error is
    measured against (the rounding error of a sum is relative to its terms, not to what is left after they cancel)"""
    from scipy.special import gammaln, digamma
    w = np.abs(w) + np.zeros_like(x)
    if kind in ('gamma', 'gamma_mv'):
        A, B = (a, b) if kind == 'gamma' else (a * a / b, a / b)
        lx = np.abs(np.log(x))
        lp = np.abs(A - 1) * lx + B * x + np.abs(gammaln(A)) + np.abs(A * np.log(B))
        gA, gB = lx + np.abs(np.log(B)) + np.abs(digamma(A)), A / B + x
        if kind == 'gamma_mv':
            gA, gB = 2 * B * gA + gB / b, B * B * gA + B / b * gB
        return lp, w * (np.abs(A - 1) / x + B), w * gA, w * gB
    if kind == 'beta':
        lx, l1x, ps = np.abs(np.log(x)), np.abs(np.log1p(-x)), np.abs(digamma(a + b))
        lp = np.abs(a - 1) * lx + np.abs(b - 1) * l1x + np.abs(gammaln(a)) + np.abs(gammaln(b)) + np.abs(gammaln(a + b))
        return lp, w * (np.abs(a - 1) / x + np.abs(b - 1) / (1 - x)), w * (lx + ps + np.abs(digamma(a))), w * (l1x + ps + np.abs(digamma(b)))
    if kind == 'laplace':
        d = np.abs(x - a)
        return np.abs(np.log(2 * b)) + d / b, w / b, w / b, w * (1 / b + d / b ** 2)
    inside = (a <= x) & (x < b)
    g = np.where(inside, w / (b - a), 0.0)
    return np.abs(np.log(b - a)) + np.zeros_like(x), np.zeros_like(x), g, g


def _reduce(g, n_p):
    """per-(s, i) terms -> what a parameter of n_p elements without a sample axis receives"""
    return g.sum().reshape(1) if n_p == 1 else g.sum(0)


def check(got, want, mag, dtype, what):
    got = got.detach().double().cpu().numpy().reshape(np.shape(want))
    if dtype == 'float64':
        err = np.abs(got - want)
        ok = err <= 1e-9 * mag
        assert ok.all(), '%s: worst error %.3e against bound %.3e' % (what, err[~ok].max(), (1e-9 * np.broadcast_to(mag, err.shape))[~ok].min())
    else:
        assert np.allclose(got, want, rtol=1e-4, atol=1e-5), '%s: worst error %.3e' % (what, np.abs(got - want).max())


def expected(kind, x, a, b, scale, dtype, cot=None):
    """(sum log p, dx (S,n), da, db) scaled as the kernel scales them, each with the magnitude its float64 tolerance is relative to; float32:
    the inputs are first shown to be fair -- the same formula in float32 on the CPU meets the float32 bar against float64."""
    S, n = x.shape
    w = scale if cot is None else scale * cot
    lp_t, g = reference(kind, x, a, b, w)
    lp = scipy_logpdf(kind, x, np.broadcast_to(a, (n,)), np.broadcast_to(b, (n,)))
    fin = np.isfinite(lp)
    assert (np.isfinite(lp_t) == fin).all()
    assert np.allclose(lp_t[fin], lp[fin], rtol=1e-10, atol=1e-10)          # scipy.stats and torch.distributions agree with each other
    mag = magnitudes(kind, x, np.broadcast_to(a, (n,)), np.broadcast_to(b, (n,)), w)
    out = {'out': (scale * lp.sum(), abs(scale) * mag[0].sum()), 'lp': lp, 'dx': (g[0], mag[1]),
           'da': (_reduce(g[1], a.size), _reduce(mag[2], a.size)), 'db': (_reduce(g[2], b.size), _reduce(mag[3], b.size))}
    if dtype == 'float32':
        lp32, g32 = reference(kind, x, a, b, w, dtype=torch.float32)
        assert np.allclose(lp32, lp, rtol=1e-4, atol=1e-5), 'the float32 inputs cancel in log p'
        assert np.allclose(scale * torch.as_tensor(lp32[fin]).float().sum().item(), scale * lp[fin].sum(), rtol=1e-4, atol=1e-5)
        for t32, key, n_p in ((g32[0], 'dx', None), (g32[1], 'da', a.size), (g32[2], 'db', b.size)):
            red = t32 if n_p is None else _reduce(t32.astype(np.float32), n_p)
            assert np.allclose(red, out[key][0], rtol=1e-4, atol=1e-5), 'the float32 inputs cancel in ' + key
    return out


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=_tdt(dtype)).cuda()


PREFILL = 0.75


def run_reduced(kind, x, a, b, scale, dtype, mask=(True, True, True, True)):
    """ops.univariate_logpdf_ on prefilled accumulators; mask: which of (out, dx, da, db) are handed over (the others are NULL)"""
    from mxfusion_amd import ops
    bufs = [torch.full(s, PREFILL, dtype=_tdt(dtype)).cuda() for s in ((1,), x.shape, a.shape, b.shape)]
    ops.univariate_logpdf_(kind, _dev(x, dtype), _dev(a, dtype), _dev(b, dtype), scale, *[t if m else None for t, m in zip(bufs, mask)])
    torch.cuda.synchronize()
    return bufs


# n = 1: single-element and per-element parameters are the same case
@pytest.mark.parametrize('n, combo', [(1, (0, 0))] + [(n, c) for n in (257, BIG) for c in ((0, 0), (0, 1), (1, 0), (1, 1))],
                         ids=lambda v: str(v) if isinstance(v, int) else 'a%s_b%s' % tuple('1n'[i] for i in v))
@pytest.mark.parametrize('S', [1, 5])
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', KINDS)
def test_reduced_kernel_value_gradients_and_accumulation(kind, dtype, n, S, combo):
    """out, dx, da, db come back as prefill + expected; accumulators behind NULL pointers are not touched and do not change the others.
    NULL in each position runs at n = 1 and n = 257; at the large n, where only the trip count differs, all pointers and out alone.
    (gamma_mv with one of mean and variance single draws the other from a range: every SHAPE_PARAMS value is covered by
    test_every_shape_parameter_value_as_single_element and by the cases where both are per element.)"""
    n_a, n_b = (n if combo[0] else 1), (n if combo[1] else 1)
    x, a, b = make_inputs(kind, n, S, n_a, n_b, dtype)
    scale = 0.5 / S
    want = expected(kind, x, a, b, scale, dtype)
    masks = [(True, True, True, True)]
    masks += [(True, False, False, False)] if n == BIG else [tuple(j != i for j in range(4)) for i in range(4)]
    for mask in masks:
        bufs = run_reduced(kind, x, a, b, scale, dtype, mask)
        for t, m, key in zip(bufs, mask, ('out', 'dx', 'da', 'db')):
            if not m:
                assert bool((t == PREFILL).all()), '%s was not handed over and changed' % key
                continue
            val, mag = want[key]
            if key == 'out' and not np.isfinite(val):
                assert float(t[0]) == -np.inf, 'a sum with an element outside the support is -inf, got %r' % float(t[0])
                continue
            check(t - PREFILL, val, mag, dtype, '%s %s' % (key, mask))
        if kind == 'uniform' and mask[1]:
            assert bool((bufs[1] == PREFILL).all())             # d/dx of a Uniform log-density is zero everywhere


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', ['gamma', 'gamma_mv', 'beta'])
def test_every_shape_parameter_value_as_single_element(kind, dtype):
    """n = 1, everything single-element, once per shape-parameter value (float64: and 1e4): lgamma and digamma on either side of the recurrence
    threshold and of digamma's zero."""
    vals = SHAPE_PARAMS + ([1e4] if dtype == 'float64' else [])
    for i, v in enumerate(vals):
        x, a, b = make_inputs(kind, 1, 5, 1, 1, dtype, seed=i, a0=v, b0=vals[(i + 4) % len(vals)] if kind == 'beta' else None)
        want = expected(kind, x, a, b, 1.0, dtype)
        bufs = run_reduced(kind, x, a, b, 1.0, dtype)
        for t, key in zip(bufs, ('out', 'dx', 'da', 'db')):
            check(t - PREFILL, want[key][0], want[key][1], dtype, '%s at shape parameter %g' % (key, v))


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_uniform_support_edges_and_laplace_at_location(dtype):
    from mxfusion_amd import ops
    x, a, b = make_inputs('uniform', 257, 5, 257, 257, dtype)
    lp = ops.univariate_logpdf_elem('uniform', _dev(x, dtype), _dev(a, dtype), _dev(b, dtype)).cpu().numpy()
    check(torch.as_tensor(lp[0, 0]), -np.log(b[0] - a[0]), abs(np.log(b[0] - a[0])), dtype, 'log p at x == low')       # inside
    assert lp[-1, 1] == -np.inf and lp[0, 2] == -np.inf                                                     # x == high, x < low: outside
    assert np.isfinite(np.delete(lp.reshape(-1), [1 + 4 * 257, 2])).all()
    bufs = run_reduced('uniform', x, a, b, 1.0, dtype)
    assert float(bufs[0][0]) == -np.inf                                    # -inf, not NaN
    g = reference('uniform', x, a, b, 1.0)[1]
    for t, want in ((bufs[2], g[1].sum(0)), (bufs[3], g[2].sum(0))):
        check(t - PREFILL, want, np.abs(g[1]).sum(0), dtype, 'uniform gradient')
    only_outside = np.array([[b[1]], [a[1] - 1.0]])                         # both samples of one element outside: its gradients are exactly zero
    bufs = run_reduced('uniform', only_outside, a[1:2], b[1:2], 1.0, dtype)
    assert all(bool((t == PREFILL).all()) for t in bufs[1:]) and float(bufs[0][0]) == -np.inf
    x, a, b = make_inputs('laplace', 257, 5, 257, 257, dtype)
    assert x[0, 0] == a[0]
    bufs = run_reduced('laplace', x, a, b, 1.0, dtype)
    assert float(bufs[1][0, 0]) == PREFILL                                  # d/dx at x == location: sign(0) = 0


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('sampled', [(False, False), (True, False), (False, True), (True, True)], ids=['a_b', 'As_b', 'a_Bs', 'As_Bs'])
def test_elementwise_kernel_and_its_cotangent_reverse_mode(kind, dtype, sampled):
    """out[s,i] = scale log p and, with a cotangent, the gradients; parameters with a sample axis of their own get (S, n) gradients."""
    from mxfusion_amd import ops
    S, n, scale = 5, 257, 1.5
    r = np.random.RandomState(3)
    x, a, b = make_inputs(kind, n, S, n, n, dtype)
    full = []
    for p, s in ((a, sampled[0]), (b, sampled[1])):
        if s and kind == 'uniform':
            p = p[None] + (-1 if p is a else 1) * r.uniform(0.0, 0.2, (S, n))      # the interval only widens: x stays where it was
        elif s and (kind == 'beta' or (kind == 'laplace' and p is a)):
            p = np.stack([np.roll(p, k) for k in range(S)])                          # another element's parameter in each sample
        elif s:
            p = p[None] * r.uniform(0.9, 1.1, (S, n))
        full.append(_round(p, dtype))
    A, B = full
    cot = _round(r.uniform(0.5, 1.5, (S, n)), dtype)
    lpA, lpB = np.broadcast_to(A, (S, n)), np.broadcast_to(B, (S, n))
    x = settle_float32(kind, x, lpA, lpB, dtype)          # (the pairs of x and per-sample parameters are new ones)
    lp = scipy_logpdf(kind, x, lpA, lpB)
    _, g = reference(kind, x, lpA, lpB, scale * cot)
    if dtype == 'float32':
        lp32, g32 = reference(kind, x, lpA, lpB, scale * cot, dtype=torch.float32)
        assert np.allclose(lp32, lp, rtol=1e-4, atol=1e-5) and all(np.allclose(u, v, rtol=1e-4, atol=1e-5) for u, v in zip(g32, g))
    xd, ad, bd, cd = _dev(x, dtype), _dev(A, dtype), _dev(B, dtype), _dev(cot, dtype)
    got = ops.univariate_logpdf_elem(kind, xd, ad, bd, scale)
    fin = np.isfinite(lp)
    assert (np.isfinite(got.cpu().numpy()) == fin).all()
    mag = magnitudes(kind, x, lpA, lpB, scale * cot)
    check(torch.where(torch.isfinite(got), got, torch.zeros_like(got)), np.where(fin, scale * lp, 0.0), scale * mag[0], dtype, 'log p')
    bufs = [torch.full(t.shape, PREFILL, dtype=_tdt(dtype)).cuda() for t in (x, A, B)]
    ops.univariate_logpdf_bwd_(kind, xd, ad, bd, cd, scale, *bufs)
    torch.cuda.synchronize()
    check(bufs[0] - PREFILL, g[0], mag[1], dtype, 'dx')
    for t, gp, mg, s, key in ((bufs[1], g[1], mag[2], sampled[0], 'da'), (bufs[2], g[2], mag[3], sampled[1], 'db')):
        check(t - PREFILL, gp if s else gp.sum(0), mg if s else mg.sum(0), dtype, key)


def test_bad_parameter_length_is_status_minus_two():
    from mxfusion_amd import _lib, ops
    x, a = torch.ones(2, 5, dtype=torch.float64).cuda(), torch.ones(2, dtype=torch.float64).cuda()
    out = torch.zeros(1, dtype=torch.float64).cuda()
    h, lib = _lib.handle(torch.cuda.current_device()), _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for n_a, n_b in ((2, 1), (1, 2)):
        rc = lib.mxf_univariate_logpdf(h, _lib.D_GAMMA, _lib.F64, 2, 5, x.data_ptr(), a.data_ptr(), n_a, a.data_ptr(), n_b, 1.0,
                                       out.data_ptr(), None, None, None, st)
        assert rc == -2
        assert b'mxf_univariate_logpdf' in lib.mxf_last_error(h)
    assert lib.mxf_univariate_logpdf(h, 99, _lib.F64, 2, 5, x.data_ptr(), a.data_ptr(), 1, a.data_ptr(), 1, 1.0, out.data_ptr(), None, None,
                                     None, st) == -2
    rc = lib.mxf_univariate_logpdf_elem(h, _lib.D_GAMMA, _lib.F64, 2, 5, x.data_ptr(), a.data_ptr(), 1, ctypes.c_int64(3), a.data_ptr(), 1, 0,
                                        1.0, x.data_ptr(), st)
    assert rc == -2                                                     # a sample stride other than 0 or n
    torch.cuda.synchronize()
    assert float(out[0]) == 0.0
    with pytest.raises(_lib.MXFError):
        ops.univariate_logpdf_('gamma', x, a, a[:1], 1.0, out)
    with pytest.raises(TypeError):
        ops.univariate_logpdf_('gamma', x, a[:1].float(), a[:1], 1.0, out)
    with pytest.raises(ValueError):
        ops.univariate_logpdf_('gamma', x.transpose(0, 1), a[:1], a[:1], 1.0, out)


# ---- through the API -------------------------------------------------------------------------------------------------------------------

def _classes():
    from mxfusion_amd.components.distributions import Gamma, GammaMeanVariance, Beta, Laplace, Uniform
    return {'gamma': Gamma, 'gamma_mv': GammaMeanVariance, 'beta': Beta, 'laplace': Laplace, 'uniform': Uniform}


def _api_inputs(kind, a_s, b_s, rv_s, dtype, S=5, rv_shape=(3, 2)):
    """parameters and random variable with (True) or without a sample axis, float64 numpy"""
    r = np.random.RandomState(5)
    sh = lambda s: ((S,) if s else ()) + rv_shape
    if kind in ('gamma', 'gamma_mv'):
        a, b = r.uniform(0.5, 4.0, sh(a_s)), r.uniform(0.5, 2.0, sh(b_s))
        x = r.uniform(0.2, 3.0, sh(rv_s))
    elif kind == 'beta':
        a, b, x = r.uniform(0.5, 4.0, sh(a_s)), r.uniform(0.5, 4.0, sh(b_s)), r.uniform(0.05, 0.95, sh(rv_s))
    elif kind == 'laplace':
        a, b, x = r.randn(*sh(a_s)), r.uniform(0.5, 2.0, sh(b_s)), 2 * r.randn(*sh(rv_s))
    else:
        a, b, x = r.uniform(-2, -1, sh(a_s)), r.uniform(1, 2, sh(b_s)), r.uniform(-1, 1, sh(rv_s))
        x.reshape(-1)[0] = 5.0                                           # one element outside the support
    return _round(a, dtype), _round(b, dtype), _round(x, dtype)


def _with_axis(t, sampled, dtype):
    t = _dev(t, dtype)
    return t if sampled else t[None]


def _factor(kind, dtype, rv_shape=(3, 2), **kw):
    return _classes()[kind].define_variable(shape=rv_shape, dtype=dtype, **kw).factor


def _variables(f, a, a_s, b, b_s, x, x_s, dtype):
    v = {f.inputs[0][1].uuid: _with_axis(a, a_s, dtype), f.inputs[1][1].uuid: _with_axis(b, b_s, dtype)}
    if x is not None:
        v[f.random_variable.uuid] = _with_axis(x, x_s, dtype)
    return v


def _np_axis(t, sampled):
    return t if sampled else t[None]


@pytest.mark.parametrize('dtype, a_s, b_s, rv_s', [('float64', True, False, True), ('float64', False, True, True), ('float64', False, False, True),
                                                    ('float64', False, False, False), ('float32', True, False, True)])
@pytest.mark.parametrize('kind', KINDS)
def test_log_pdf_sample_axis_combinations(kind, dtype, a_s, b_s, rv_s):
    """the combinations of tests/test_gpu_normal.py: a parameter sampled or not, the variable sampled or not; values and reverse mode"""
    a, b, x = _api_inputs(kind, a_s, b_s, rv_s, dtype)
    f = _factor(kind, dtype)
    assert [n for n, _ in f.inputs] == {'gamma': ['alpha', 'beta'], 'gamma_mv': ['mean', 'variance'], 'beta': ['alpha', 'beta'],
                                        'laplace': ['location', 'scale'], 'uniform': ['low', 'high']}[kind]
    variables = _variables(f, a, a_s, b, b_s, x, rv_s, dtype)
    leaves = [t.requires_grad_(True) for t in variables.values()]
    got = f.log_pdf(F=None, variables=variables)
    any_s = a_s or b_s or rv_s
    assert got.dtype == _tdt(dtype) and got.shape == ((5 if any_s else 1), 3, 2)
    A, B, X = [np.broadcast_to(_np_axis(t, s), got.shape) for t, s in ((a, a_s), (b, b_s), (x, rv_s))]
    want = scipy_logpdf(kind, X, A, B)
    fin = np.isfinite(want)
    g = got.detach().double().cpu().numpy()
    assert (np.isfinite(g) == fin).all()
    cot = np.random.RandomState(6).uniform(0.5, 1.5, got.shape)
    mag = magnitudes(kind, X, A, B, cot)
    masked = torch.where(torch.isfinite(got), got, torch.zeros_like(got))
    check(masked, np.where(fin, want, 0.0), mag[0], dtype, 'log p')
    flat = lambda t: np.ascontiguousarray(t).reshape(got.shape[0], -1)
    gw = [t.reshape(got.shape) for t in reference(kind, flat(X), flat(A), flat(B), flat(cot))[1]]
    masked.mul(_dev(cot, dtype)).sum().backward()
    for leaf, gp, mg, s, key in zip(leaves, (gw[1], gw[2], gw[0]), (mag[2], mag[3], mag[1]), (a_s, b_s, rv_s), ('da', 'db', 'dx')):
        keep = s or not any_s                       # a leaf without the sample axis receives the sum over the samples
        check(leaf.grad, gp if keep else gp.sum(0, keepdims=True), mg if keep else mg.sum(0, keepdims=True), dtype, key)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('per_element', [True, False], ids=['per_element', 'single'])
@pytest.mark.parametrize('kind', KINDS)
def test_log_pdf_sum_is_the_fused_mean_and_sum(kind, dtype, per_element):
    """log_pdf_sum (what FactorGraph.log_pdf adds) against log_pdf(...).mean(0).sum(), values and gradients; a sampled parameter falls back to
    exactly that expression."""
    a, b, x = _api_inputs(kind, False, False, True, dtype)
    if kind == 'uniform':
        x = np.clip(x, -0.9, 0.9)                       # all inside: a finite sum to compare
    if not per_element:
        a, b = a[:1, :1], b[:1, :1]
    f = _factor(kind, dtype)
    rtol, atol = (1e-9, 1e-11) if dtype == 'float64' else (1e-4, 1e-5)
    res = []
    for route in ('sum', 'elementwise'):
        variables = _variables(f, a, False, b, False, x, True, dtype)
        leaves = [t.requires_grad_(True) for t in variables.values()]
        val = f.log_pdf_sum(None, variables) if route == 'sum' else f.log_pdf(F=None, variables=variables).mean(0).sum()
        val.backward()
        res.append([val.detach()] + [t.grad for t in leaves])
    for u, v in zip(*res):
        assert np.allclose(u.double().cpu().numpy(), v.double().cpu().numpy(), rtol=rtol, atol=atol)
    A, B = np.broadcast_to(a[None], x.shape), np.broadcast_to(b[None], x.shape)
    assert np.allclose(float(res[0][0]), scipy_logpdf(kind, x, A, B).mean(0).sum(), rtol=rtol, atol=atol)
    a5 = np.broadcast_to(a[None], (5,) + a.shape) * (1 + 0.01 * np.arange(5).reshape(5, 1, 1)) if kind != 'uniform' else \
        np.broadcast_to(a[None], (5,) + a.shape) - 0.01 * np.arange(5).reshape(5, 1, 1)
    a5 = _round(a5, dtype)
    variables = _variables(f, a5, True, b, False, x, True, dtype)
    want = scipy_logpdf(kind, x, np.broadcast_to(a5, x.shape), B).mean(0).sum()
    assert np.allclose(float(f.log_pdf_sum(None, variables)), want, rtol=rtol, atol=atol)


@pytest.mark.parametrize('kind', KINDS)
def test_log_pdf_scaling_follows_the_reference(kind):
    """laplace.py:54 and uniform.py:61 multiply by log_pdf_scaling; gamma.py and beta.py never do."""
    a, b, x = _api_inputs(kind, False, False, True, 'float64')
    if kind == 'uniform':
        x = np.clip(x, -0.9, 0.9)
    f = _factor(kind, 'float64')
    base = scipy_logpdf(kind, x, np.broadcast_to(a[None], x.shape), np.broadcast_to(b[None], x.shape))
    f.log_pdf_scaling = 3.0
    k = 3.0 if kind in ('laplace', 'uniform') else 1.0
    variables = _variables(f, a, False, b, False, x, True, 'float64')
    assert np.allclose(f.log_pdf(F=None, variables=variables).cpu().numpy(), k * base, rtol=1e-9, atol=1e-12)
    assert np.allclose(float(f.log_pdf_sum(None, variables)), k * base.mean(0).sum(), rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', KINDS)
def test_draw_samples_with_injected_noise(kind, dtype):
    """MockRandomGenerator replays the injected buffer; the draw is the reference's formula applied to it."""
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    S, rv_shape = 5, (3, 2)
    a, b, _ = _api_inputs(kind, kind == 'beta', kind == 'beta', True, dtype)
    buf = _round(np.random.RandomState(7).uniform(0.1, 2.0, (2, S) + rv_shape), dtype)
    f = _factor(kind, dtype, rand_gen=MockRandomGenerator(_dev(buf.reshape(-1), dtype)))
    variables = _variables(f, a, kind == 'beta', b, kind == 'beta', None, None, dtype)
    got = f.draw_samples(F=None, variables=variables, num_samples=S)
    assert got.dtype == _tdt(dtype) and tuple(got.shape) == (S,) + rv_shape
    want = {'laplace': a[None] + b[None] * buf[0], 'beta': buf[0] / (buf[0] + buf[1])}.get(kind, buf[0])
    rtol, atol = (1e-12, 0) if dtype == 'float64' else (1e-6, 0)
    assert np.allclose(got.double().cpu().numpy(), want, rtol=rtol, atol=atol)


def test_beta_draw_samples_refuses_parameters_without_the_sample_shape():
    """beta.py:91-93"""
    a, b, _ = _api_inputs('beta', False, False, True, 'float64')
    f = _factor('beta', 'float64')
    with pytest.raises(ValueError, match='Shape mismatch'):
        f.draw_samples(F=None, variables=_variables(f, a, False, b, False, None, None, 'float64'), num_samples=5)


def test_device_generators_draw_from_the_named_distributions():
    """the real generators: 200 000 draws have the distribution's mean and variance (5 standard errors of either)"""
    torch.manual_seed(0)
    N = 200000
    cases = {'gamma': (3.0, 2.0, 1.5, 0.75), 'gamma_mv': (1.5, 0.75, 1.5, 0.75), 'beta': (2.0, 3.0, 0.4, 0.04), 'laplace': (0.5, 2.0, 0.5, 8.0),
             'uniform': (-1.0, 3.0, 1.0, 16.0 / 12.0)}
    for kind, (a, b, mean, var) in cases.items():
        f = _factor(kind, 'float64', rv_shape=(1,))
        shape = (N, 1) if kind == 'beta' else (1, 1)
        variables = {f.inputs[0][1].uuid: torch.full(shape, a, dtype=torch.float64).cuda(), f.inputs[1][1].uuid: torch.full(shape, b, dtype=torch.float64).cuda()}
        s = f.draw_samples(F=None, variables=variables, num_samples=N).double()
        assert tuple(s.shape) == (N, 1)
        assert abs(float(s.mean()) - mean) < 5 * (var / N) ** 0.5, kind
        assert abs(float(s.var()) - var) < 0.05 * var, kind
        if kind == 'uniform':
            assert float(s.min()) >= a and float(s.max()) < b


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

def test_gp_notebook_with_gamma_priors_end_to_end():
    """The notebook GP (20 points, RBF, float64) with Gamma(2, 1) on the lengthscale and GammaMeanVariance(0.01, 1e-4) on the noise variance,
    through GradBasedInference(MAP) with softplus-constrained point-mass locations (MAP's `locations`): initial loss = the oracle's exact-GP negative log-likelihood minus the two scipy log-pdfs; gradient
    w.r.t. the unconstrained lengthscale and 5 Adam steps against a float64 CPU replay with the oracle's Adam."""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Gamma, GammaMeanVariance
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.modules.gp_modules import GPRegression
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.inference import GradBasedInference, MAP
    from oracle import gp_oracle as O
    np.random.seed(0)
    X = np.random.uniform(-3., 3., (20, 1))
    Y = np.sin(X) + np.random.randn(20, 1) * 0.05
    dev = lambda t: torch.as_tensor(t, dtype=torch.float64).cuda()
    m = Model()
    m.N = Variable()
    m.X = Variable(shape=(m.N, 1))
    m.lengthscale = Gamma.define_variable(alpha=2., beta=1., shape=(1,), dtype='float64')
    m.noise_var = GammaMeanVariance.define_variable(mean=0.01, variance=1e-4, shape=(1,), dtype='float64')
    m.kernel = RBF(input_dim=1, variance=dev([1.0]), lengthscale=m.lengthscale, dtype='float64')
    m.Y = GPRegression.define_variable(X=m.X, kernel=m.kernel, noise_var=m.noise_var, shape=(m.N, 1), dtype='float64')
    positive = lambda v0: Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=dev([v0]))
    alg = MAP(model=m, observed=[m.X, m.Y], locations={m.lengthscale: positive(1.0), m.noise_var: positive(0.01)})
    infr = GradBasedInference(inference_algorithm=alg, dtype='float64')
    infr.initialize(X=dev(X), Y=dev(Y))
    loc = {k: alg.posterior[v].factor.location for k, v in (('lengthscale', m.lengthscale), ('noise_var', m.noise_var))}
    loc['variance'] = m.kernel.variance

    kern = O.RBF(1, ARD=False)

    def cpu_loss(raw):
        ls, noise = O.softplus(raw['lengthscale']), O.softplus(raw['noise_var'])
        prior = torch.distributions.Gamma(2.0, 1.0).log_prob(ls).sum() + \
            torch.distributions.Gamma(0.01 * 0.01 / 1e-4, 0.01 / 1e-4).log_prob(noise).sum()
        return O.map_gp_loss(kern, O.T(X), O.T(Y), raw) - prior
    raw = {'lengthscale': O.inv_softplus(O.T([1.0])), 'variance': O.inv_softplus(O.T([1.0])), 'noise_var': O.inv_softplus(O.T([0.01]))}
    for k in raw:
        assert abs(float(infr.params.raw(loc[k])) - float(raw[k])) < 1e-12, k

    nll = float(O.map_gp_loss(kern, O.T(X), O.T(Y), raw))
    want = nll - stats.gamma.logpdf(1.0, 2.0, scale=1.0) - stats.gamma.logpdf(0.01, 1.0, scale=0.01)
    loss, loss_for_gradient = infr.create_executor()(dev(X), dev(Y))
    assert abs(float(loss) - want) <= 1e-9 * (abs(nll) + abs(want - nll)), (float(loss), want)
    loss_for_gradient.backward()
    lv = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    cpu_loss(lv).backward()
    for k in raw:
        got_g = float(infr.params.grad(loc[k]))
        assert abs(got_g - float(lv[k].grad)) <= 1e-9 * max(1.0, abs(float(lv[k].grad))), (k, got_g, float(lv[k].grad))
    infr.params.zero_grad()

    infr.run(X=dev(X), Y=dev(Y), max_iter=5, learning_rate=0.05)
    opt = O.MXNetAdam(0.05)
    for _ in range(5):
        lv = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
        cpu_loss(lv).backward()
        raw = opt.step({k: v.detach() for k, v in lv.items()}, {k: v.grad for k, v in lv.items()}, batch_size=1)
    for k in raw:
        assert abs(float(infr.params[loc[k]]) - float(O.softplus(raw[k]))) < 1e-8, k
    assert abs(float(O.softplus(raw['lengthscale'])) - 1.0) > 1e-3                      # the steps moved the parameters
