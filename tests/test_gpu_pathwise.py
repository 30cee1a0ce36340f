"""The three pathwise sampling algorithms end to end on the GPU against tests/_pathwise_ref.py replaying the draws a recording generator handed
out: SVGPRegression (N = 60, M = 7, Q = 2, P = 2), GPRegression (N = 25), SparseGPRegression and BayesianGPLVM (at deterministic test inputs),
with an ARD RBF kernel, a Matern32 kernel and Matern52 + RBF, 3 samples of 8 features per kernel at 23 test points.  float64: rtol 1e-7 of the
largest sample value; a float32 model (the update in float64, the features in float32): rtol 1e-4 of it, the reference at the rounded
parameters.  Then: row chunks, re-evaluation of the same paths, the gradient in the test inputs, the noise, a mean function, and the three
*SamplingPrediction algorithms bit for bit unchanged by a pathwise draw in between.  Inducing points are well separated (the recipe of
tests/test_gpu_bayesian_gplvm.py); the posteriors of the exact and the sparse GP are what one evaluation of the module's log-pdf persists."""
import numpy as np
import pytest
import torch

import _pathwise_ref as PW

pytestmark = pytest.mark.gpu

N_SV, N_GP, M, Q, P, NT, S, D = 60, 25, 7, 2, 2, 23, 3, 8
JITTER = 1e-6
KERNELS = ['rbf', 'matern32', 'matern52+rbf']
RTOL = {torch.float64: 1e-7, torch.float32: 1e-4}


class Recording(object):
    """a generator that records what it hands out (seeded; the gamma draws come from numpy)"""

    def __init__(self, seed):
        self.g = torch.Generator(device='cuda').manual_seed(seed)
        self.rng = np.random.default_rng(seed)
        self.draws = []

    def _keep(self, t):
        self.draws.append(t.clone())
        return t

    def sample_normal(self, loc=0, scale=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._keep(torch.randn(tuple(shape), generator=self.g, dtype=dtype, device='cuda'))

    def sample_gamma(self, alpha=1, beta=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._keep(torch.as_tensor(self.rng.gamma(alpha, 1.0 / beta, tuple(shape)), dtype=dtype).cuda())

    def sample_uniform(self, low=0., high=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._keep(torch.rand(tuple(shape), generator=self.g, dtype=dtype, device='cuda') * (high - low) + low)


class Replay(object):
    """hands the recorded draws out again, in order"""

    def __init__(self, draws):
        self.draws = [d.clone() for d in draws]

    def _next(self, shape, dtype):
        t = self.draws.pop(0)
        assert tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape))
        return t.to(dtype)

    def sample_normal(self, loc=0, scale=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._next(shape, dtype)

    def sample_gamma(self, alpha=1, beta=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._next(shape, dtype)

    def sample_uniform(self, low=0., high=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._next(shape, dtype)


def _kernel(name, dtype):
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Matern32, Matern52
    if name == 'rbf':
        return RBF(input_dim=Q, ARD=True, dtype=dtype)
    if name == 'matern32':
        return Matern32(input_dim=Q, ARD=False, dtype=dtype)
    return Matern52(input_dim=Q, ARD=True, dtype=dtype) + RBF(input_dim=Q, ARD=False, dtype=dtype)


def _data(which, kname):
    """numpy float64 values of everything a model holds"""
    N = N_GP if which == 'gp' else N_SV
    rng = np.random.default_rng(N + len(kname))
    X = rng.uniform(-2.0, 2.0, (N, Q))
    pick = [0]
    for _ in range(M - 1):
        pick.append(int(np.argmax(np.min(((X[:, None] - X[pick][None]) ** 2).sum(-1), 1))))
    p = dict(X=X, Z=X[pick] + 0.1 * rng.standard_normal((M, Q)), Y=np.sin(X @ rng.standard_normal((Q, P))) + 0.1 * rng.standard_normal((N, P)),
             noise=np.array([0.3]), Xt=rng.uniform(-2.5, 2.5, (NT, Q)), qm=rng.standard_normal((M, P)), qW=0.3 * rng.standard_normal((M, M)),
             qd=rng.uniform(0.2, 0.8, M), mean_train=rng.standard_normal((N, P)), mean_test=rng.standard_normal((NT, P)),
             raw=rng.uniform(-2.0, 0.5, (N, Q)))
    names = {'rbf': ['rbf'], 'matern32': ['matern32'], 'matern52+rbf': ['add_matern52', 'add_rbf']}[kname]
    for n in names:
        p[n + '_lengthscale'] = rng.uniform(0.8, 1.4, Q if n in ('rbf', 'add_matern52') else 1)
        p[n + '_variance'] = rng.uniform(0.6, 1.4, 1)
    p['kernel_names'] = names
    return p


def _blocks(p, c):
    return [(n.split('_')[-1], c(p[n + '_lengthscale']), c(p[n + '_variance'])[0]) for n in p['kernel_names']]


def _model(which, kname, dtype, with_mean=False):
    """(module, runtime dict holding the parameters, the test inputs and -- exact, sparse GP and GPLVM -- the persisted posterior, data)"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.inference.inference_alg import SET_PARAMETER_PREFIX
    from mxfusion_amd.modules.gp_modules import GPRegression, SVGPRegression, SparseGPRegression, BayesianGPLVM
    from mxfusion_amd.util.inference import VariablesDict
    p = _data(which, kname)
    dts = 'float64' if dtype == torch.float64 else 'float32'
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).cuda()[None]
    N = p['X'].shape[0]
    m = Model()
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.3)
    kern = _kernel(kname, dts)
    if which != 'gplvm':
        m.X = Variable(shape=(N, Q))
    if which != 'gp':
        m.Z = Variable(shape=(M, Q))
    if with_mean:
        m.mean = Variable(shape=(N, P))
    mean = m.mean if with_mean else None
    if which == 'gp':
        m.Y = GPRegression.define_variable(X=m.X, kernel=kern, noise_var=m.noise_var, shape=(N, P), mean=mean, dtype=dts)
    elif which == 'gplvm':
        m.Y = BayesianGPLVM.define_variable(kernel=kern, noise_var=m.noise_var, shape=(N, P), inducing_inputs=m.Z, dtype=dts)
    else:
        cls = SVGPRegression if which == 'svgp' else SparseGPRegression
        m.Y = cls.define_variable(X=m.X, kernel=kern, noise_var=m.noise_var, inducing_inputs=m.Z, shape=(N, P), mean=mean, dtype=dts)
    gp = m.Y.factor
    g, post = gp._module_graph, gp._extra_graphs[0]
    vs = VariablesDict({g.X.uuid: d(p['X']), m.noise_var.uuid: d(p['noise']), m.Y.uuid: d(p['Y'])})
    for n, v in gp.kernel.parameters.items():
        vs[v.uuid] = d(p[n])
    if which != 'gp':
        vs[m.Z.uuid] = d(p['Z'])
    if with_mean:
        vs[g.mean.uuid] = d(p['mean_train'])
    if which == 'gplvm':
        vs[g.X_var.uuid] = PositiveTransformation().transform(d(p['raw']))
    if which == 'svgp':
        vs[post.qU_mean.uuid], vs[post.qU_cov_W.uuid], vs[post.qU_cov_diag.uuid] = d(p['qm']), d(p['qW']), d(p['qd'])
    else:
        alg = {'gp': 'gp_log_pdf', 'sgp': 'sgp_log_pdf', 'gplvm': 'gplvm_log_pdf'}[which]
        getattr(gp, alg).jitter = 0.0 if which == 'gp' else JITTER
        with torch.no_grad():
            getattr(gp, alg).compute(None, vs)
        for v in post.get_parameters():
            vs[v.uuid] = vs[SET_PARAMETER_PREFIX + v.uuid][1][None]
    vs[g.X.uuid] = d(p['Xt'])
    if with_mean:
        vs[g.mean.uuid] = d(p['mean_test'])
    return m, gp, vs, p


def _algorithm(which, gp, rand_gen, **kw):
    from mxfusion_amd.modules.gp_modules import GPRegressionPathwiseSampling, SVGPRegressionPathwiseSampling, SparseGPRegressionPathwiseSampling
    cls = {'gp': GPRegressionPathwiseSampling, 'svgp': SVGPRegressionPathwiseSampling}.get(which, SparseGPRegressionPathwiseSampling)
    alg = cls(gp._module_graph, gp._extra_graphs[0], [gp._module_graph.X], num_features=D, rand_gen=rand_gen, jitter=JITTER, **kw)
    alg.num_samples = S
    return alg


def _reference(which, p, draws, dtype, Xt=None, with_mean=False, posterior=None):
    """the restatement at the values the run sees (rounded for a float32 model), replaying the recorded draws"""
    c = lambda a: (torch.as_tensor(a, dtype=torch.float32) if dtype == torch.float32 else torch.as_tensor(a)).double()
    draws = [t.double().cpu() for t in draws]
    blocks = _blocks(p, c)
    Xt = c(p['Xt']) if Xt is None else Xt
    Y = c(p['Y']) - c(p['mean_train']) if with_mean else c(p['Y'])
    if which == 'svgp':
        return PW.svgp_paths(blocks, Xt, c(p['Z']), c(p['qm']), c(p['qW']), c(p['qd']), draws, jitter=JITTER)
    if which == 'gp':
        return PW.gp_paths(blocks, Xt, c(p['X']), Y, c(p['noise'])[0], draws)
    L, LA, wv = posterior if posterior is not None else PW.sgp_posterior(blocks, c(p['X']), Y, c(p['Z']), c(p['noise'])[0], jitter=JITTER)
    return PW.sgp_paths(blocks, Xt, c(p['Z']), L, LA, wv, draws)


def _close(got, ref, rtol, what):
    got, ref = got.double().cpu(), ref.double()
    err, top = float((got - ref).abs().max()), float(ref.abs().max())
    print(what, 'max error', err, 'largest value', top, 'ratio to the bar', err / (rtol * top))
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    assert err <= rtol * top, (what, err, top)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('kname', KERNELS)
@pytest.mark.parametrize('which', ['svgp', 'gp', 'sgp'])
def test_output_is_the_restatement_on_the_recorded_draws(which, kname, dtype):
    m, gp, vs, p = _model(which, kname, dtype)
    rec = Recording(7)
    out = _algorithm(which, gp, rec).compute(None, vs)[m.Y.uuid]
    R = {'svgp': M, 'gp': N_GP, 'sgp': M}[which]
    nk = len(p['kernel_names'])
    assert out.shape == (S, NT, P) and out.dtype == dtype
    assert tuple(rec.draws[-1].shape) == (S, R, P) and tuple(rec.draws[-2].shape) == (S, nk * D, P)
    assert len(rec.draws) == 2 + sum(2 if n.endswith('rbf') else 3 for n in p['kernel_names'])
    _close(out, _reference(which, p, rec.draws, dtype), RTOL[dtype], '%s %s' % (which, kname))


def test_bayesian_gplvm_posterior_works_unchanged():
    """SparseGPRegressionPathwiseSampling on a BayesianGPLVM: the persisted L, LA, wv, X_mean as graph.X, deterministic test inputs"""
    m, gp, vs, p = _model('gplvm', 'rbf', torch.float64)
    post = gp._extra_graphs[0]
    rec = Recording(9)
    out = _algorithm('gplvm', gp, rec).compute(None, vs)[m.Y.uuid]
    L, LA, wv = [vs[v.uuid][0].double().cpu() for v in (post.L, post.LA, post.wv)]
    assert out.shape == (S, NT, P)
    _close(out, _reference('gplvm', p, rec.draws, torch.float64, posterior=(L, LA, wv)), 1e-7, 'gplvm')


@pytest.mark.parametrize('which', ['svgp', 'gp'])
def test_row_chunks_and_reevaluation(which):
    """chunk_rows = 64 at Nt = 150 equals chunk_rows = 65536 on the same draws to 1e-12; paths(Xa) and paths(Xb) are the rows of paths(cat(Xa, Xb))"""
    m, gp, vs, p = _model(which, 'matern52+rbf', torch.float64)
    Xbig = torch.as_tensor(np.random.default_rng(1).uniform(-2.5, 2.5, (150, Q))).cuda()
    vs[gp._module_graph.X.uuid] = Xbig[None]
    rec = Recording(3)
    whole = _algorithm(which, gp, rec).compute(None, vs)[m.Y.uuid]
    chunked = _algorithm(which, gp, Replay(rec.draws), chunk_rows=64).compute(None, vs)[m.Y.uuid]
    top = float(whole.abs().max())
    print('chunks', float((whole - chunked).abs().max()), 'largest', top)
    assert whole.shape == (S, 150, P) and float((whole - chunked).abs().max()) <= 1e-12 * top
    paths = _algorithm(which, gp, Replay(rec.draws)).draw(None, vs)
    both, a, b = paths(Xbig), paths(Xbig[:37]), paths(Xbig[None, 37:])
    assert float((both - whole).abs().max()) <= 1e-12 * top
    assert a.shape == (S, 37, P) and float((torch.cat([a, b], 1) - both).abs().max()) <= 1e-12 * top
    _close(both, _reference(which, p, rec.draws, torch.float64, Xt=Xbig.cpu()), 1e-7, 'at 150 points')


@pytest.mark.parametrize('which,kname', [('svgp', 'matern52+rbf'), ('gp', 'rbf'), ('sgp', 'matern32')])
def test_gradient_in_the_test_inputs(which, kname):
    """paths(X).sum().backward(): X.grad against autograd through the restatement, rtol 1e-7 of the largest entry"""
    m, gp, vs, p = _model(which, kname, torch.float64)
    rec = Recording(5)
    paths = _algorithm(which, gp, rec).draw(None, vs)
    X = vs[gp._module_graph.X.uuid][0].clone().requires_grad_(True)
    wts = torch.as_tensor(np.random.default_rng(2).standard_normal((S, NT, P))).cuda()
    (paths(X) * wts).sum().backward()
    Xr = torch.as_tensor(p['Xt']).clone().requires_grad_(True)
    (_reference(which, p, rec.draws, torch.float64, Xt=Xr) * wts.cpu()).sum().backward()
    _close(X.grad, Xr.grad, 1e-7, 'gradient %s %s' % (which, kname))
    with torch.no_grad():
        assert not paths(X).requires_grad


def test_noise_is_the_last_draw_times_its_standard_deviation():
    m, gp, vs, p = _model('svgp', 'rbf', torch.float64)
    rec = Recording(4)
    noisy = _algorithm('svgp', gp, rec, noise_free=False).compute(None, vs)[m.Y.uuid]
    clean = _algorithm('svgp', gp, Replay(rec.draws[:-1])).compute(None, vs)[m.Y.uuid]
    assert tuple(rec.draws[-1].shape) == (S, NT, P)
    assert float((noisy - clean - np.sqrt(p['noise'][0]) * rec.draws[-1]).abs().max()) <= 1e-13


@pytest.mark.parametrize('which', ['svgp', 'gp', 'sgp'])
def test_mean_function_is_added(which):
    m, gp, vs, p = _model(which, 'rbf', torch.float64, with_mean=True)
    rec = Recording(6)
    out = _algorithm(which, gp, rec).compute(None, vs)[m.Y.uuid]
    ref = _reference(which, p, rec.draws, torch.float64, with_mean=which != 'svgp') + torch.as_tensor(p['mean_test'])
    _close(out, ref, 1e-7, 'mean function, ' + which)


def test_the_sampling_predictions_are_unchanged_by_a_pathwise_draw():
    """the three *SamplingPrediction algorithms, full covariance, on a fixed generator: bit for bit the same before and after a pathwise draw
    from the same module"""
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    from mxfusion_amd.modules.gp_modules.gp_regression import GPRegressionSamplingPrediction
    from mxfusion_amd.modules.gp_modules.svgp_regression import SVGPRegressionSamplingPrediction
    from mxfusion_amd.modules.gp_modules.sparsegp_regression import SparseGPRegressionSamplingPrediction
    eps = torch.as_tensor(np.random.default_rng(8).standard_normal((S, NT, P))).cuda()
    for which, cls in (('gp', GPRegressionSamplingPrediction), ('svgp', SVGPRegressionSamplingPrediction), ('sgp', SparseGPRegressionSamplingPrediction)):
        m, gp, vs, p = _model(which, 'rbf', torch.float64)
        outs = []
        for _ in range(2):
            alg = cls(gp._module_graph, gp._extra_graphs[0], [gp._module_graph.X], rand_gen=MockRandomGenerator(eps), diagonal_variance=False, jitter=1e-8)
            alg.num_samples = S
            with torch.no_grad():
                outs.append(alg.compute(None, vs)[m.Y.uuid].clone())
            _algorithm(which, gp, Recording(1)).compute(None, vs)
        assert outs[0].shape == (S, NT, P) and torch.equal(outs[0], outs[1]), which
