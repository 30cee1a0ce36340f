"""mxf_lik_expect, mxf_lik_expect_elem and mxf_lik_moments against the float64 reference of tests/_lik_ref.py (same nodes, SciPy special
functions on the CPU): three kinds, both dtypes, row counts on either side of a wavefront, of a 256-thread block and into the grid-stride
tail, S in {1, 3}, P in {1, 3} with v shared by the columns, labels shared by the samples or with their own sample axis, 1 / 20 / 64 nodes,
scale != 1, per-sample weights, accumulation into pre-filled buffers, the tails m = +-30 and v in {0, 1e-8, 0.3, 4, 100} (Poisson: v <= 4, so
that exp(f_k) stays inside float32), a negative v of -1e-12.  Bars of tests/test_gpu_univariate.py: float64 rtol 1e-9, atol 1e-11; float32
rtol 1e-4, atol 1e-5; a sum is taken relative to the sum of the magnitudes of its terms."""
import math

import numpy as np
import pytest
import torch

import _lik_ref as R

pytestmark = pytest.mark.gpu

BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
# (n, S, P, labels with their own sample axis, nodes): every n, and every value of the other axes at least twice
CASES = [(1, 1, 1, False, 20), (63, 3, 3, True, 1), (64, 3, 1, False, 64), (65, 1, 3, False, 20), (257, 3, 3, True, 20), (1000, 3, 3, False, 64)]
SCALE = 0.7


def _inputs(kind, n, S, P, y_own, dtype, seed):
    """y, m, v rounded to the working dtype (the reference sees what the kernel sees), as float64 arrays"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-5.0, 5.0, (S, n, P))
    vs = [0.0, 1e-8, 0.3, 4.0] + ([] if kind == 'poisson_exp' else [100.0])
    v = np.array([vs[i % len(vs)] for i in range(n)])[None].repeat(S, 0)
    y = rng.integers(0, 7 if kind == 'poisson_exp' else 2, (S if y_own else 1, n, P)).astype(np.float64)
    if n >= 63:
        m[:, 0], m[:, 1], m[:, 3], m[:, 4] = 30.0, -30.0, 30.0, -30.0        # (v = 0, 1e-8, 4 and 100 -- Poisson: 0 -- there)
        v[:, 5], v[:, 6] = -1e-12, 0.0
        m[:, 6], y[:, 6] = m[:, 5], y[:, 5]
    r = lambda a: torch.as_tensor(a, dtype=dtype).double().numpy()
    return r(y), r(m), r(v)


def _reference(kind, y, m, v, nq):
    """per element: E[g], d/dm, and per row d/dv (Price), each with the sum of the magnitudes of its terms; E[mu], E[mu^2]"""
    x, w = np.polynomial.hermite.hermgauss(nq)
    w = w / math.sqrt(math.pi)
    f = m[..., None] + np.sqrt(2.0 * np.maximum(v, 0.0))[..., None, None] * x
    g, g1, g2 = R.g_np(kind, y[..., None], f)
    assert np.isfinite(g).all() and np.isfinite(g1).all() and np.isfinite(g2).all()
    mu = R.mu_np(kind, f)
    q = lambda a: (a * w).sum(-1)
    return dict(e=q(g), e_mag=q(np.abs(g)), dm=q(g1), dm_mag=q(np.abs(g1)), dv=0.5 * q(g2).sum(-1), dv_mag=0.5 * q(np.abs(g2)).sum(-1),
                mu1=q(mu), mu2=q(mu * mu))


def _close(got, ref, mag, dtype, what):
    rtol, atol = BARS[dtype]
    got = got.double().cpu().numpy()
    err = np.abs(got - ref)
    bad = err > rtol * mag + atol
    assert not bad.any(), '%s: %d off, worst %.3g against %.3g allowed' % (what, int(bad.sum()), float(err.max()), float((rtol * mag + atol).min()))


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('kind', R.KINDS)
def test_kernel_against_reference(kind, dtype):
    from mxfusion_amd import ops
    for seed, (n, S, P, y_own, nq) in enumerate(CASES):
        y, m, v = _inputs(kind, n, S, P, y_own, dtype, seed)
        ref = _reference(kind, y, m, v, nq)
        d = lambda a: torch.as_tensor(a, dtype=dtype).cuda()
        yd, md, vd = d(y), d(m), d(v)
        tag = '%s n=%d S=%d P=%d nq=%d' % (kind, n, S, P, nq)
        # the per-element entry
        elem = ops.lik_expect_elem(kind, yd, md, vd, scale=SCALE, num_nodes=nq)
        assert elem.shape == (S, n, P)
        _close(elem, SCALE * ref['e'], SCALE * ref['e_mag'], dtype, tag + ' elem')
        # the reduced entry with gradients and per-sample weights, into pre-filled buffers
        cot = np.linspace(0.5, 1.5, S)
        out, dm, dv = d(np.full(S, 3.0)), d(np.full((S, n, P), 0.25)), d(np.full((S, n), -0.5))
        ops.lik_expect_(kind, yd, md, vd, SCALE, out, dm_acc=dm, dv_acc=dv, cot=d(cot), num_nodes=nq)
        wgt = SCALE * cot
        _close(out, 3.0 + SCALE * ref['e'].sum((-1, -2)), 3.0 + SCALE * ref['e_mag'].sum((-1, -2)), dtype, tag + ' out')
        _close(dm, 0.25 + wgt[:, None, None] * ref['dm'], 0.25 + wgt[:, None, None] * ref['dm_mag'], dtype, tag + ' dm')
        _close(dv, -0.5 + wgt[:, None] * ref['dv'], 0.5 + wgt[:, None] * ref['dv_mag'], dtype, tag + ' dv')
        # the reduced entry without weights or gradients agrees with the sum of the per-element one
        out2 = d(np.zeros(S))
        ops.lik_expect_(kind, yd, md, vd, SCALE, out2, num_nodes=nq)
        _close(out2, elem.double().sum((-1, -2)).cpu().numpy(), SCALE * ref['e_mag'].sum((-1, -2)), dtype, tag + ' out against elem')
        # the moments entry
        e1, e2 = ops.lik_moments(kind, md, vd, num_nodes=nq)
        _close(e1, ref['mu1'], np.abs(ref['mu1']), dtype, tag + ' E[mu]')
        _close(e2, ref['mu2'], np.abs(ref['mu2']), dtype, tag + ' E[mu^2]')
        if kind == 'poisson_exp':       # E[g] = y m - E[mu] - lgamma(y + 1): the entries agree with each other
            lg = R.special.gammaln(y + 1.0)
            _close(elem, SCALE * (y * m - e1.double().cpu().numpy() - lg), SCALE * (np.abs(y * m) + ref['mu1'] + lg), dtype, tag + ' elem against moments')
        if n >= 63:                     # v = -1e-12 counts as v = 0
            for t in (elem, dm, e1):
                assert torch.equal(t[:, 5], t[:, 6]), tag
            assert torch.equal(dv[:, 5], dv[:, 6]), tag


def test_shared_m_and_v_under_sampled_labels():
    """y (S, n, P) over m (1, n, P), v (1, n): strides 0 on the large operands; the gradients still come per sample"""
    from mxfusion_amd import ops
    y, m, v = _inputs('bernoulli_probit', 65, 3, 3, True, torch.float64, 11)
    m, v = m[:1], v[:1]
    ref = _reference('bernoulli_probit', y, m, v, 20)
    d = lambda a: torch.as_tensor(a).cuda()
    out, dm, dv = d(np.zeros(3)), d(np.zeros((3, 65, 3))), d(np.zeros((3, 65)))
    ops.lik_expect_('bernoulli_probit', d(y), d(m), d(v), 1.0, out, dm_acc=dm, dv_acc=dv)
    _close(out, ref['e'].sum((-1, -2)), ref['e_mag'].sum((-1, -2)), torch.float64, 'out')
    _close(dm, ref['dm'], ref['dm_mag'], torch.float64, 'dm')
    _close(dv, ref['dv'], ref['dv_mag'], torch.float64, 'dv')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_closed_forms_on_the_device(dtype):
    """Poisson: E[g] = y m - exp(m + v / 2) - lgamma(y + 1) exactly, at the kernel bars; probit: E[mu] = Phi(m / sqrt(1 + v)) within the 1e-4
    of the 20-node rule (tests/test_likelihood_host.py)"""
    from mxfusion_amd import ops
    rng = np.random.default_rng(5)
    n = 500
    r = lambda a: torch.as_tensor(a, dtype=dtype).double().numpy()
    m, v = r(rng.uniform(-3.0, 3.0, (1, n, 1))), r(np.exp(rng.uniform(np.log(1e-4), np.log(4.0), (1, n))))
    y = rng.integers(0, 7, (1, n, 1)).astype(np.float64)
    d = lambda a: torch.as_tensor(a, dtype=dtype).cuda()
    lg, ex = R.special.gammaln(y + 1.0), np.exp(m + 0.5 * v[..., None])
    _close(ops.lik_expect_elem('poisson_exp', d(y), d(m), d(v)), y * m - ex - lg, np.abs(y * m) + ex + lg, dtype, 'poisson closed form')
    e1, _ = ops.lik_moments('bernoulli_probit', d(m), d(v))
    assert float(np.abs(e1.double().cpu().numpy()[..., 0] - R.special.ndtr(m[..., 0] / np.sqrt(1.0 + v))).max()) <= 1e-4


def test_bad_arguments_are_refused():
    from mxfusion_amd import ops, _lib
    t = torch.zeros(1, 4, 1, dtype=torch.float64).cuda()
    v = torch.ones(1, 4, dtype=torch.float64).cuda()
    with pytest.raises(ValueError):
        ops.lik_expect_elem('bernoulli_logit', t, t, v, num_nodes=65)
    with pytest.raises(ValueError):
        ops.lik_expect_elem('bernoulli_logit', t, t, torch.ones(1, 5, dtype=torch.float64).cuda())
    with pytest.raises(_lib.MXFError):
        ops.lik_expect_elem(7, t, t, v)
    with pytest.raises(TypeError):
        ops.lik_expect_elem('bernoulli_logit', t, t.float(), v)
