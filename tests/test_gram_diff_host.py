"""Host checks of the difference-form covariances (no GPU): the float64 restatement tests/_gram_diff_ref.py tied to the RBF restatement the
project already trusts (tests/_gram_ref.py) through limiting cases; the ABI of mxf_gram_diff / mxf_gram_diff_bwd in the header, the binding
and the built library; the pure launch plan (csrc/gram_diff_plan.h, printed by tests/host/gram_diff_plan_check.cpp); and the per-pair math
of csrc/gram_diff.h, compiled for the host (tests/host/gram_diff_check.cpp), against the restatement."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _gram_diff_ref as R
import _gram_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_gram_diff', 'mxf_gram_diff_bwd')
KD = {'periodic': 0, 'rq': 1, 'sm': 2}
t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
N, Q = 40, 3


def _rbf(X, X2, ls):
    return t64(G.gram_ref('rbf', X[None], X2[None], np.atleast_2d(ls), np.ones((1, 1)))[0])


# ---- the restatement against the RBF restatement --------------------------------------------------------------------------------------------
def test_rq_at_large_alpha_is_the_rbf():
    """truncation x^2 e^-x / (2 alpha) <= 2.7e-9 (x = r2 / 2), the rounding of 1 + x / alpha ~1e-8: 1e-7 absolute"""
    rng = np.random.default_rng(0)
    X, X2, ls = rng.uniform(-2, 2, (N, Q)), rng.uniform(-2, 2, (N, Q)), rng.uniform(0.8, 1.8, Q)
    K, _ = R.gram('rq', t64(X), t64(X2), t64([1.0]), t64(ls), t64([1e8]))
    assert float((K - _rbf(X, X2, ls)).abs().max()) <= 1e-7


def test_sm_with_one_component_at_zero_frequency_is_the_rbf():
    """2 pi^2 tau^2 s^2 = tau^2 / (2 l^2) at s = 1 / (2 pi l)"""
    rng = np.random.default_rng(1)
    X, X2, ls = rng.uniform(-2, 2, (N, Q)), rng.uniform(-2, 2, (N, Q)), rng.uniform(0.8, 1.8, Q)
    K, T = R.gram('sm', t64(X), t64(X2), t64([1.0]), torch.zeros(1, Q, dtype=torch.float64), t64(1 / (2 * math.pi * ls))[None])
    assert float((K - _rbf(X, X2, ls)).abs().max()) <= 1e-12 and torch.equal(K, T)


def test_periodic_at_a_whole_period_is_the_variance():
    rng = np.random.default_rng(2)
    X, per = rng.uniform(-2, 2, (N, Q)), rng.uniform(0.5, 2.0, Q)
    K, _ = R.gram('periodic', t64(X), t64(X + per), t64([1.0]), t64(rng.uniform(0.8, 1.8, Q)), t64(per))
    assert float((torch.diagonal(K) - 1).abs().max()) <= 1e-14


def test_periodic_small_angle_limit_is_the_rbf():
    """sin^2(x) = x^2 (1 - x^2 / 3 + ...) at x = pi tau / p: with p = 1e4 the RBF of lengthscale p l / pi, up to E e^-E x^2 / 3 with E the
    exponent -- at most 0.37 (pi tau / p)^2 / 3, which is below the bar of 1e-9 for |tau| <= 0.25 (at |tau| = 3 it is 1e-7: the inputs are drawn
    from [-0.125, 0.125] and the RBF lengthscales from [0.05, 0.15], so that the exponent still runs from 0 to beyond 1)"""
    rng = np.random.default_rng(3)
    X, X2, ls = rng.uniform(-0.125, 0.125, (N, Q)), rng.uniform(-0.125, 0.125, (N, Q)), rng.uniform(0.05, 0.15, Q)
    K, _ = R.gram('periodic', t64(X), t64(X2), t64([1.0]), t64(ls * math.pi / 1e4), t64(np.full(Q, 1e4)))
    assert float(K.min()) < 0.3 and float((K - _rbf(X, X2, ls)).abs().max()) <= 1e-9


def _case(kind, rng, Q=Q, A=3, ard=True):
    n = Q if ard else 1
    if kind == 'sm':
        return t64(rng.uniform(0.3, 1.0, A)), t64(rng.uniform(0.05, 0.6, (A, Q))), t64(rng.uniform(0.05, 0.4, (A, Q)))
    return t64(rng.uniform(0.5, 1.5, 1)), t64(rng.uniform(0.8, 1.8, n)), t64(rng.uniform(0.7, 2.5, n if kind == 'periodic' else 1))


@pytest.mark.parametrize('kind', R.KINDS)
def test_gram_is_symmetric_positive_semidefinite(kind):
    rng = np.random.default_rng(4)
    X = t64(rng.uniform(-2, 2, (N, Q)))
    K, _ = R.gram(kind, X, None, *_case(kind, rng))
    assert torch.equal(K, K.T)
    assert float(torch.linalg.eigvalsh(K).min()) >= -N * 1e-12
    p = _case(kind, np.random.default_rng(5))
    assert torch.allclose(torch.diagonal(R.gram(kind, X, None, *p)[0]), R.kdiag(kind, p[0]).expand(N), rtol=1e-15, atol=0)


@pytest.mark.parametrize('kind', R.KINDS)
def test_forward_mode_sums_are_the_reverse_mode_gradient(kind):
    """R.grads (one forward-mode pass per element, so that the absolute sums come with it) against torch.autograd.grad, square and not"""
    rng = np.random.default_rng(6)
    X, X2 = t64(rng.uniform(-2, 2, (9, 2))), t64(rng.uniform(-2, 2, (7, 2)))
    p = _case(kind, rng, Q=2)
    for Z in (X2, None):
        dK = t64(rng.standard_normal((9, 9 if Z is None else 7)))
        leaves = [t.clone().requires_grad_(True) for t in (X,) + (() if Z is None else (Z,)) + p]
        K = R.components(kind, leaves[0], leaves[0] if Z is None else leaves[1], *leaves[-3:]).sum(0)
        want = torch.autograd.grad((K * dK).sum(), leaves)
        got = R.grads(kind, X, Z, *p, dK)
        names = ('X',) + (() if Z is None else ('X2',)) + ('p0', 'p1', 'p2')
        assert set(got) == set(names)
        for n, w in zip(names, want):
            g, T = got[n]
            assert torch.allclose(g, w, rtol=1e-12, atol=1e-14) and bool((T >= g.abs() * (1 - 1e-12)).all()), n


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert 'int ' + name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    for macro, value in (('MXF_GD_MAX_Q', _lib.GD_MAX_Q), ('MXF_GD_SM_MAX_Q', _lib.GD_SM_MAX_Q), ('MXF_GD_SM_MAX_A', _lib.GD_SM_MAX_A)):
        assert '#define %s %d' % (macro, value) in header
    assert (_lib.GD_MAX_Q, _lib.GD_SM_MAX_Q, _lib.GD_SM_MAX_A) == (16, 8, 8)
    assert 'enum { MXF_KD_PERIODIC = 0, MXF_KD_RQ = 1, MXF_KD_SM = 2 };' in header
    assert (_lib.KD_PERIODIC, _lib.KD_RQ, _lib.KD_SM) == (0, 1, 2) and _lib.K_WHITE == 6


def test_ops_refuse_cpu_tensors_and_classes_refuse_beyond_the_limits():
    from mxfusion_amd import _lib, ops
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import Periodic, RationalQuadratic, SpectralMixture
    X, one = torch.ones(1, 5, 2, dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.gram_diff('periodic', X, None, one, one, one, False)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.gram_diff_bwd('rq', X, None, one, one, one, False, torch.ones(1, 5, 5, dtype=torch.float64))
    for make, limit in ((lambda: SpectralMixture(9, 2), '8 input dimensions'), (lambda: SpectralMixture(2, 9), '8 mixture components'),
                        (lambda: Periodic(17), '16 input dimensions'), (lambda: RationalQuadratic(17), '16 input dimensions')):
        with pytest.raises(ModelSpecificationError, match=limit):
            make()
    k = SpectralMixture(2, 3)
    assert k.parameter_names == ['sm_weights', 'sm_means', 'sm_scales'] and k.fused_spec() is None and not hasattr(k, '_kind')
    assert (k.weights.shape, k.means.shape, k.scales.shape) == ((3,), (3, 2), (3, 2))
    mu = np.asarray(k.means.initial_value)
    assert len({tuple(r) for r in mu}) == 3                                    # the default components differ
    assert Periodic(2, ARD=True).parameter_names == ['periodic_variance', 'periodic_lengthscale', 'periodic_period']
    assert RationalQuadratic(2).parameter_names == ['rq_variance', 'rq_lengthscale', 'rq_alpha']


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
COLS = 'bwd esize kind S N N2 Q A square has_X has_p has_K ldk'.split()
BASE = dict(bwd=0, esize=4, kind=0, S=1, N=300, N2=200, Q=3, A=1, square=0, has_X=1, has_p=1, has_K=1, ldk=200)
SIZES = (1, 63, 64, 65, 257, 70000)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('gram_diff_plan') / 'gram_diff_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'gram_diff_plan_check.cpp'), '-o', exe], check=True)
    line = lambda r: ' '.join(str(int(r[c])) for c in COLS)
    return lambda reqs, text=False: subprocess.run([exe], input=('text 1\n' if text else '') + '\n'.join(line(r) for r in reqs), capture_output=True,
                                                   text=True, check=True).stdout.strip().split('\n')


def test_plan_owns_every_row_and_column_once(plan):
    reqs = [dict(BASE, bwd=b, esize=e, kind=k, S=S, N=n, N2=n2, Q=q, A=3 if k == 2 else 1, ldk=n2) for b in (0, 1) for e in (4, 8) for k, q in ((0, 16), (1, 1), (2, 8))
            for S in (1, 3) for n in SIZES for n2 in SIZES]
    for r, out in zip(reqs, plan(reqs)):
        rc, QT, rb, gx, gy, gz, lds, rmin, rmax, cmin, cmax = (int(t) for t in out.split())
        assert rc == 0 and (rmin, rmax, cmin, cmax) == (1, 1, 1, 1), (r, out)
        assert QT == r['Q'] and rb % 64 == 0 and rb >= 64 and (gy - 1) * rb < r['N'] <= gy * rb and (gx - 1) * 256 < r['N2'] <= gx * 256 and gz == r['S'], (r, out)
        assert gx <= 2 ** 31 - 1 and gy <= 65535 and gz <= 65535, (r, out)                   # HIP's grid limits
        assert lds == (rb * QT * r['esize'] if r['bwd'] else 0) and lds <= 16 * 1024, (r, out)
        if not r['bwd']:
            assert rb == 64, (r, out)


def test_plan_of_a_square_gram_ignores_n2_and_pads_q(plan):
    outs = plan([dict(BASE, square=1, N=300, N2=0, ldk=300, Q=q) for q in (1, 2, 3, 4, 5, 8, 9, 16)])
    assert [int(o.split()[1]) for o in outs] == [1, 2, 4, 4, 8, 8, 16, 16] and all(o.split()[0] == '0' and o.split()[3] == '2' for o in outs)


REFUSALS = [(dict(Q=17), -3, 'Q above the limit of 16 input dimensions'), (dict(kind=1, Q=17, has_X=0), -3, 'Q above the limit of 16 input dimensions'),
            (dict(kind=2, Q=9), -3, 'Q above the limit of 8 input dimensions (SpectralMixture)'), (dict(kind=2, A=9), -3, 'A above the limit of 8 components'),
            (dict(kind=3), -2, 'unknown kind'), (dict(N=0), -2, 'S, N, N2, Q, A >= 1'), (dict(N2=0), -2, 'S, N, N2, Q, A >= 1'), (dict(S=0), -2, 'S, N, N2, Q, A >= 1'),
            (dict(Q=0), -2, 'S, N, N2, Q, A >= 1'), (dict(kind=2, A=0), -2, 'S, N, N2, Q, A >= 1'), (dict(Q=17, N=0), -2, 'S, N, N2, Q, A >= 1'),
            (dict(has_X=0), -2, 'null X, parameter operand or matrix'), (dict(has_p=0), -2, 'null X, parameter operand or matrix'),
            (dict(has_K=0, bwd=1), -2, 'null X, parameter operand or matrix'), (dict(ldk=199), -2, 'negative sample stride or row stride below N2'),
            (dict(N=64 * 65536, bwd=0), -3, 'grid too large'), (dict(S=65536), -3, 'grid too large')]


@pytest.mark.parametrize('over,rc,why', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_plan_refusals(plan, over, rc, why):
    code, _, text = plan([dict(BASE, **over)], text=True)[0].partition(' ')
    assert (int(code), text) == (rc, why)


# ---- the per-pair math of gram_diff.h -------------------------------------------------------------------------------------------------------
def _points():
    """(kind, Q, A, ard, tau, p0, p1, p2): some hundred random pairs and the corners: tau = 0, |tau / p| ~ 1e3, a cosine factor within 1e-9
    of zero, a pair far outside the envelope"""
    rng = np.random.default_rng(7)
    pts = []
    for i in range(40):
        for kind in R.KINDS:
            q, A, ard = int(rng.integers(1, 9)), int(rng.integers(1, 9)) if kind == 'sm' else 1, int(rng.integers(0, 2)) if kind != 'sm' else 1
            p0, p1, p2 = _case(kind, rng, Q=q, A=A, ard=bool(ard))
            pts.append((kind, q, A, ard, rng.uniform(-3, 3, q), p0.numpy(), p1.numpy(), p2.numpy()))
    one = np.ones(1)
    pts += [(k, 2, 1, 1, np.zeros(2), one * 1.3, np.array([[0.4, 0.7]]) if k == 'sm' else np.array([0.9, 1.4]), np.array([[0.2, 0.3]]) if k == 'sm' else
             (one * 0.8 if k == 'rq' else np.array([0.7, 1.9]))) for k in R.KINDS]
    pts += [('periodic', 2, 1, 1, np.array([1003.3, -917.8]), one, np.array([0.9, 1.4]), np.array([1.0, 0.9])),
            ('periodic', 1, 1, 0, np.array([-1.0e-3]), one, one * 0.05, one),
            ('sm', 2, 1, 1, np.array([900.4, -1.0]), one, np.array([[1.1, 0.3]]), np.array([[2e-4, 0.1]])),
            ('sm', 3, 2, 1, np.array([0.25 + 1e-10, 0.6, -0.9]), np.array([0.7, 0.4]), np.array([[1.0, 0.3, 0.2], [0.1, 0.2, 0.3]]), np.full((2, 3), 0.05)),
            ('sm', 2, 1, 1, np.array([0.25, 0.75]), one, np.array([[1.0, 1.0]]), np.array([[0.05, 0.05]])),
            ('rq', 3, 1, 1, np.array([1e-4, 2e-4, -1e-4]), one, np.array([0.9, 1.1, 1.4]), one * 2.5),
            ('rq', 2, 1, 0, np.array([40.0, -30.0]), one, one, one * 0.4)]
    return pts


def _sm_envelope(tau, w, mu, s):
    """the SpectralMixture columns with every cosine and sine at 1, summed in absolute value: K, dK/dtau, dK/dw, dK/dmu, dK/ds, K"""
    tau, pi = np.abs(tau), math.pi
    env = w * np.exp(-2 * pi ** 2 * (tau ** 2 * s ** 2).sum(-1))                    # (A,)
    dtau = (env[:, None] * (4 * pi ** 2 * s ** 2 * tau + 2 * pi * np.abs(mu))).sum(0)
    return np.concatenate([[env.sum()], dtau, env / w, (env[:, None] * 2 * pi * tau * np.ones_like(mu)).ravel(), (env[:, None] * 4 * pi ** 2 * tau ** 2 * s).ravel(),
                           [env.sum()]])


def _periodic_envelope(tau, K, var, ls, per):
    """the Periodic columns with every sine at 1: K, dK/dtau, dK/dvariance, dK/dlengthscale, dK/dperiod, K"""
    q, ard = len(tau), len(ls) > 1 or len(tau) == 1
    l, p = np.broadcast_to(ls, (q,)), np.broadcast_to(per, (q,))
    dtau = K * math.pi / (2 * p * l ** 2)
    dl, dp = K / l ** 3, dtau * np.abs(tau) / p
    return np.concatenate([[K], dtau, [K / var[0]], dl if ard else [dl.sum()], dp if ard else [dp.sum()], [K]])


@pytest.mark.parametrize('kind,ard', [('periodic', True), ('periodic', False), ('sm', True)])
def test_majorant_derivatives_are_the_closed_form_envelopes(kind, ard):
    """the scale T that R.grads returns for ONE pair with cotangent 1 (forward-mode derivatives of R.majorant) is the slope with its sines and
    cosines at 1, as _periodic_envelope and _sm_envelope state it in closed form: 1e-13 relative"""
    rng = np.random.default_rng(8)
    for _ in range(10):
        q = int(rng.integers(1, 5))
        ps = _case(kind, rng, Q=q, A=3, ard=ard)
        x, z = rng.uniform(-3, 3, q), rng.uniform(-3, 3, q)
        X, Z = t64(x)[None], t64(z)[None]
        g = R.grads(kind, X, Z, *ps, torch.ones(1, 1, dtype=torch.float64))
        got = np.concatenate([g[n][1].numpy().ravel() for n in ('X', 'p0', 'p1', 'p2')])
        assert np.array_equal(g['X'][1].numpy(), g['X2'][1].numpy())
        if kind == 'sm':
            want = _sm_envelope(x - z, *(p.numpy() for p in ps))[1:-1]
        else:
            want = _periodic_envelope(x - z, float(R.gram(kind, X, Z, *ps)[0]), *(p.numpy() for p in ps))[1:-1]
        assert got.shape == want.shape and np.allclose(got, want, rtol=1e-13, atol=0), (kind, got, want)


def test_device_math_against_the_restatement(tmp_path):
    """Value and every partial derivative, both precisions, against automatic differentiation of the restatement at the arguments each
    precision saw.  The bar is the one of the GPU tests (tests/test_gpu_gram_diff.py) for ONE pair: C eps amp T with T the sum of the absolute
    terms (over the components; a single pair has no other sum) and amp = 1 + the largest phase or exponent argument; C = 32 here: a libm
    sine, cosine, exp and log1p carry an ulp each, every term passes through about ten roundings, and the RQ alpha slope is a difference of
    two such terms.  For ONE SpectralMixture or Periodic pair T is replaced by the term with its cosines and sines at 1 (_sm_envelope, _periodic_envelope): a phase rounded by
    eps |phase| moves a cosine by that much absolutely, however small the cosine is; summed over a Gram's pairs that is the T of the GPU tests.
    A term below 1e-300 (float32: 1e-37) has left the format and is not asked for."""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path / 'gram_diff_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'gram_diff_check.cpp'),
                    '-o', exe, '-lm'], check=True)
    pts = _points()
    text = '\n'.join('%d %d %d %d ' % (KD[k], q, A, ard) + ' '.join('%.17g' % v for a in (tau, p0, p1, p2) for v in np.ravel(a)) for k, q, A, ard, tau, p0, p1, p2 in pts)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split('\n')
    assert len(out) == len(pts) >= 100
    worst = {}
    for line, (kind, q, A, ard, tau, p0, p1, p2) in zip(out, pts):
        got = np.array([float(t) for t in line.split()])
        assert np.isfinite(got).all(), (kind, tau)
        half = len(got) // 2
        for cols, cast, eps, tiny in ((got[:half], np.float64, 2.0 ** -53, 1e-300), (got[half:], np.float32, 2.0 ** -24, 1e-37)):
            X, Z = t64(np.asarray(tau).astype(cast))[None], torch.zeros(1, q, dtype=torch.float64)
            ps = [t64(np.asarray(p).astype(cast)) for p in (p0, p1, p2)]
            K, T = R.gram(kind, X, Z, *ps)
            g = R.grads(kind, X, Z, *ps, torch.ones(1, 1, dtype=torch.float64), need=('X', 'p0', 'p1', 'p2'))
            ref = np.concatenate([[float(K)]] + [g[n][0].numpy().ravel() for n in ('X', 'p0', 'p1', 'p2')] + [[float(K)]])
            scale = np.concatenate([[float(T)]] + [g[n][1].numpy().ravel() for n in ('X', 'p0', 'p1', 'p2')] + [[float(T)]])
            if kind == 'sm':
                scale = np.maximum(scale, _sm_envelope(X[0].numpy(), *(p.numpy() for p in ps)))
            if kind == 'rq':          # dK/dalpha = K (x / (1 + x) - log1p(x)): two terms; the restatement's own 1 + x costs it K eps on top
                x = float(((X[0] / ps[1]) ** 2).sum() / (2 * ps[2]))
                scale[-2] = max(scale[-2], float(K) * (x / (1 + x) + math.log1p(x))) + float(K)
            if kind == 'periodic':
                scale = np.maximum(scale, _periodic_envelope(X[0].numpy(), float(K), *(p.numpy() for p in ps)))
            assert cols.shape == ref.shape, (kind, cols.shape, ref.shape)
            amp = R.amplification(kind, X, Z, *ps)
            ratio = np.abs(cols - ref) / (eps * amp * np.maximum(scale, tiny))
            ratio[(scale < tiny) & (np.abs(cols) < tiny)] = 0
            key = (kind, cast.__name__)
            worst[key] = max(worst.get(key, 0.0), float(ratio.max()))
            assert ratio.max() <= 32, (kind, cast.__name__, tau, int(ratio.argmax()), cols, ref)
        if not np.any(tau):
            assert got[0] == float(np.sum(p0)) and np.float32(got[half]) == np.float32(np.sum(np.float32(p0)))                   # an exact diagonal
    print('worst ratios', worst)
