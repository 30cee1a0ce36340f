"""IterativeGPRegression on the GPU: log_pdf and its gradients against the host restatement tests/_iterative_ref.py on replayed probes
and against GPRegression on exact probes, prediction against GPRegressionMeanVariancePrediction, a short MAP run, and the refusal of a
non-stationary kernel.

How the bars follow from cg_tol.  Both the module and the restatement stop a column at the relative residual tol, so each solution is
within kappa tol of the exact one in relative 2-norm, kappa <= (N variance + noise) / noise (the trace bounds the largest eigenvalue of K,
the noise the smallest of Khat).  Two such solutions differ by at most 2 kappa tol; the value and the gradients are bilinear in two
solutions, 4 kappa tol; the Lanczos quadrature of a column that stops one iteration apart moves by the square of the CG error, far below.
The bar is 10 kappa tol, relative to the sum of the magnitudes of a quantity's terms (the restatement's `scale`).  In float64 tol = 1e-10;
the float32 run is held to the project's float32 bar, rtol 1e-4 / atol 1e-5 on the same scales, at tol = 2e-6 and noise 0.5."""
import functools

import numpy as np
import pytest
import torch

import _iterative_ref as IR

pytestmark = pytest.mark.gpu

N, Q, P, T = 300, 3, 2, 6
HOST_BAR = 1.7e-11      # tests/test_iterative_host.py: 100 x the error measured there


class Replay(object):
    """a rand_gen that hands out recorded draws in order and records the shapes asked for"""

    def __init__(self, draws):
        self.draws, self.asked = list(draws), []

    def sample_normal(self, loc=0, scale=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        self.asked.append(tuple(shape))
        d = self.draws.pop(0)
        assert tuple(d.shape) == tuple(shape), (d.shape, shape)
        return d


@functools.lru_cache(maxsize=None)
def _data(n=N, noise=0.1, rounded=False):
    rng = np.random.default_rng(n)
    q = Q if n == N else 2
    p = dict(X=rng.uniform(-2, 2, (n, q)), noise=np.array([noise]), ls=rng.uniform(0.9, 1.4, q), var=np.array([1.1]),
             Xt=rng.uniform(-2.2, 2.2, (70, q)))
    p['Y'] = np.sin(p['X'] @ rng.standard_normal((q, P))) + 0.3 * rng.standard_normal((n, P))
    if rounded:
        p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    return p


def _model(cls, p, dtype, **kw):
    """(module, runtime variables with the sample axis, {name: leaf tensor that requires a gradient})"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.util.inference import VariablesDict
    dts = 'float64' if dtype == torch.float64 else 'float32'
    n, q = p['X'].shape
    m = Model()
    m.X = Variable(shape=(n, q))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    m.Y = cls.define_variable(X=m.X, kernel=RBF(q, ARD=True, dtype=dts), noise_var=m.noise_var, shape=(n, P), dtype=dts, **kw)
    gp = m.Y.factor
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).cuda()[None]
    leaves = dict(Y=d(p['Y']).requires_grad_(True), noise=d(p['noise']).requires_grad_(True), ls=d(p['ls']).requires_grad_(True),
                  var=d(p['var']).requires_grad_(True))
    vs = VariablesDict({gp._module_graph.X.uuid: d(p['X']), m.noise_var.uuid: leaves['noise'], m.Y.uuid: leaves['Y']})
    for name, v in gp.kernel.parameters.items():
        vs[v.uuid] = leaves['ls' if name.endswith('lengthscale') else 'var']
    return gp, vs, leaves


def _value_and_grads(alg, vs, leaves):
    logL = alg.compute(None, vs)
    assert tuple(logL.shape) == (1,)
    g = torch.autograd.grad(logL.sum(), [leaves[k] for k in ('ls', 'var', 'noise', 'Y')])
    c = lambda t: t.detach().double().cpu().numpy()
    return dict(value=float(logL.detach().double().cpu()[0]), dls=c(g[0])[0], dvar=float(c(g[1])[0, 0]), dnoise=float(c(g[2])[0, 0]), dY=c(g[3])[0])


def _compare(got, ref, scale, rtol, atol, what):
    worst = 0.0
    for k in ('value', 'dls', 'dvar', 'dnoise', 'dY'):
        err = np.abs(np.asarray(got[k]) - np.asarray(ref[k]))
        ratio = float(np.max(err / (rtol * np.asarray(scale[k]) + atol)))
        print(what, k, 'max error', float(err.max()), 'scale', float(np.max(scale[k])), 'ratio to the bar', ratio)
        worst = max(worst, ratio)
    assert worst <= 1.0, (what, worst)


def _replayed(rank, dtype, tol, noise):
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression
    p = _data(N, noise, dtype == torch.float32)
    eps = np.random.default_rng(7 + rank).standard_normal((N + rank, T))
    rg = Replay([torch.as_tensor(eps, dtype=dtype).cuda()])
    gp, vs, leaves = _model(IterativeGPRegression, p, dtype, num_probes=T, precond_rank=rank, cg_tol=tol, max_cg_iter=400, rand_gen=rg)
    got = _value_and_grads(gp.iterative_gp_log_pdf, vs, leaves)
    assert rg.asked == [(N + rank, T)] and not rg.draws, 'the draw contract: one (N + r, T) call'
    e = eps.astype(np.float32).astype(np.float64) if dtype == torch.float32 else eps
    ref = IR.logpdf('rbf', p['X'], p['Y'], float(p['noise'][0]), p['ls'], float(p['var'][0]), e, rank, tol=tol, max_iter=400)
    assert ref['rank'] == rank and ref['residual'] <= tol
    print('iterations', int(gp.iterative_gp_log_pdf.cfg.last.iterations.max()), 'restatement', max(ref['iterations']))
    return got, ref, p


@pytest.mark.parametrize('rank', [0, 8])
def test_log_pdf_and_gradients_are_the_restatement_on_replayed_probes(rank):
    tol = 1e-10
    got, ref, p = _replayed(rank, torch.float64, tol, 0.1)
    kappa = (N * p['var'][0] + p['noise'][0]) / p['noise'][0]
    _compare(got, ref, ref['scale'], 10 * kappa * tol, 0.0, 'float64 rank %d' % rank)


@pytest.mark.parametrize('rank', [0, 8])
def test_float32_log_pdf_and_gradients(rank):
    got, ref, p = _replayed(rank, torch.float32, 2e-6, 0.5)
    _compare(got, ref, ref['scale'], 1e-4, 1e-5, 'float32 rank %d' % rank)


def test_exact_probes_give_gp_regression():
    """N = 64, Q = 2: the 64 draws sqrt(64) e_i at rank 0 make the trace exact, and at tol 1e-13 the value and gradients are GPRegression's"""
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression, GPRegression
    n = 64
    p = _data(n)
    rg = Replay([torch.as_tensor(IR.exact_probes(n)).cuda()])
    gp, vs, leaves = _model(IterativeGPRegression, p, torch.float64, num_probes=n, precond_rank=0, cg_tol=1e-13, max_cg_iter=4 * n, rand_gen=rg)
    got = _value_and_grads(gp.iterative_gp_log_pdf, vs, leaves)
    print('iterations', int(gp.iterative_gp_log_pdf.cfg.last.iterations.max()))
    gp2, vs2, leaves2 = _model(GPRegression, p, torch.float64)
    ref = _value_and_grads(gp2.gp_log_pdf, vs2, leaves2)
    scale = IR.logpdf('rbf', p['X'], p['Y'], 0.1, p['ls'], 1.1, IR.exact_probes(n), 0, tol=1e-13, max_iter=4 * n)['scale']
    _compare(got, ref, scale, HOST_BAR, 0.0, 'exact probes')


def test_prediction_is_gp_regression():
    """mean and variance at Nt = 70 from the persisted alpha against GPRegressionMeanVariancePrediction at the same parameters; the bar is the
    CG bound 10 kappa tol of the module docstring, relative to the largest mean and to the prior variance"""
    from mxfusion_amd.inference.inference_alg import SET_PARAMETER_PREFIX
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression, GPRegression
    p, tol, out = _data(N), 1e-10, {}
    for cls, kw, log_pdf, predict in ((IterativeGPRegression, dict(cg_tol=tol, precond_rank=8), 'iterative_gp_log_pdf', 'iterative_gp_predict'),
                                      (GPRegression, {}, 'gp_log_pdf', 'gp_predict')):
        gp, vs, _ = _model(cls, p, torch.float64, **kw)
        post = gp._extra_graphs[0]
        with torch.no_grad():
            getattr(gp, log_pdf).compute(None, vs)
            for v in post.get_parameters():
                vs[v.uuid] = vs[SET_PARAMETER_PREFIX + v.uuid][1][None]
            vs[gp._module_graph.X.uuid] = torch.as_tensor(p['Xt']).cuda()[None]
            alg = getattr(gp, predict)
            alg.noise_free = False
            if cls is IterativeGPRegression:
                alg.chunk_cols, alg.chunk_rows = 32, 33          # three column chunks (the last of 6) and three row chunks
            mu, var = alg.compute(None, vs)[gp._module_graph.Y.uuid]
        out[cls.__name__] = (mu.double().cpu().numpy(), var.double().cpu().numpy())
    (mu, var), (mu_ref, var_ref) = out['IterativeGPRegression'], out['GPRegression']
    assert mu.shape == mu_ref.shape == (1, 70, P) and var.shape == var_ref.shape == (1, 70)
    bar = 10 * (N * 1.1 + 0.1) / 0.1 * tol
    e_mu, e_var = np.abs(mu - mu_ref).max() / np.abs(mu_ref).max(), np.abs(var - var_ref).max() / 1.1
    print('mean error', e_mu, 'variance error', e_var, 'bar', bar)
    assert e_mu <= bar and e_var <= bar


def test_twenty_map_steps_lower_the_exact_objective():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.inference import GradBasedInference, MAP
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression, GPRegression
    p = _data(N)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).cuda()
    torch.manual_seed(0)
    m = Model()
    m.X = Variable(shape=(N, Q))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.5)
    m.Y = IterativeGPRegression.define_variable(X=m.X, kernel=RBF(Q, ARD=True, lengthscale=0.5, dtype='float64'), noise_var=m.noise_var, shape=(N, P),
                                                dtype='float64')
    infr = GradBasedInference(MAP(model=m, observed=[m.X, m.Y]), dtype='float64')
    infr.initialize(X=(N, Q), Y=(N, P))
    kern = m.Y.factor.kernel

    def exact():
        q = dict(p, noise=infr.params[m.noise_var].double().cpu().numpy().reshape(1), ls=infr.params[kern.lengthscale].double().cpu().numpy().reshape(Q),
                 var=infr.params[kern.variance].double().cpu().numpy().reshape(1))
        gp2, vs2, _ = _model(GPRegression, q, torch.float64)
        with torch.no_grad():
            return -float(gp2.gp_log_pdf.compute(None, vs2)[0])
    before = exact()
    infr.run(X=t(p['X']), Y=t(p['Y']), learning_rate=0.05, max_iter=20)
    after = exact()
    print('exact negative log-pdf before', before, 'after', after)
    assert np.isfinite(after) and after < before


def test_a_linear_kernel_is_a_specification_error():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import Linear
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression
    m = Model()
    m.X = Variable(shape=(N, Q))
    m.noise_var = Variable(shape=(1,), initial_value=0.1)
    with pytest.raises(ModelSpecificationError, match='single stationary kernel'):
        IterativeGPRegression.define_variable(X=m.X, kernel=Linear(Q), noise_var=m.noise_var, shape=(N, P))
