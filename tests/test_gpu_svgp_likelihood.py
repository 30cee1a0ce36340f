"""SVGPLikelihood on the GPU against tests/_lik_ref.py: the bound and its gradients in Z, the kernel parameters and q(u) for every likelihood
on an ARD RBF and on RBF + Linear (N = 50, M = 7, Q = 2, P in {1, 2}; jitter 1e-6, a full W and d, log_pdf_scaling 4, a mean function once,
float64 and the same model in float32), the latent and the observation-space prediction, a training run and a minibatch step.  The
reference differentiates by autograd, except d/dv of the data term, which is the Price form as in the kernel.  Bars: value rtol 1e-8,
gradients rtol 1e-6 with atol 1e-7 max|g| (those of smoke() for the regression bound); float32 rtol 1e-4, atol 1e-5."""
import numpy as np
import pytest
import torch

import _lik_ref as R

pytestmark = pytest.mark.gpu

N, M, Q = 50, 7, 2
LIKS = {'bernoulli_logit': 'BernoulliLogit', 'bernoulli_probit': 'BernoulliProbit', 'poisson_exp': 'PoissonExp'}


def _data(kind, P, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, Q))
    f = np.sin(X @ rng.standard_normal((Q, P)))
    Y = rng.poisson(np.exp(f)).astype(np.float64) if kind == 'poisson_exp' else (rng.uniform(size=(N, P)) < R.special.expit(3 * f)).astype(np.float64)
    p = dict(X=X, Y=Y, Z=X[:M] + 0.1 * rng.standard_normal((M, Q)), qm=0.5 * rng.standard_normal((M, P)), qW=0.2 * rng.standard_normal((M, M)),
             qd=rng.uniform(0.3, 1.0, M), ls=np.array([0.9, 1.4]), var=np.array([1.3]), variances=np.array([0.3, 0.6]),
             mean=0.3 * rng.standard_normal((N, P)))
    return p


def _module(which, kind, P, dtype='float64', with_mean=False):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Linear
    from mxfusion_amd.modules import gp_modules
    m = Model()
    m.N = Variable()
    m.X = Variable(shape=(m.N, Q))
    m.Z = Variable(shape=(M, Q))
    kern = RBF(input_dim=Q, ARD=True, dtype=dtype)
    if which == 'rbf+linear':
        kern = kern + Linear(input_dim=Q, ARD=True, dtype=dtype)
    if with_mean:
        m.mean = Variable(shape=(m.N, P))
    m.Y = gp_modules.SVGPLikelihood.define_variable(X=m.X, kernel=kern, likelihood=getattr(gp_modules, LIKS[kind])(), inducing_inputs=m.Z,
                                                    mean=m.mean if with_mean else None, shape=(m.N, P), dtype=dtype)
    return m


def _kernel_names(which):
    pre = 'add_' if which == 'rbf+linear' else ''
    names = {'ls': pre + 'rbf_lengthscale', 'var': pre + 'rbf_variance'}
    if which == 'rbf+linear':
        names['variances'] = 'add_linear_variances'
    return names


def _variables(m, which, p, leaves, dtype, with_mean=False, X=None, Y=None):
    """the runtime dict of the module's algorithms (leading sample axis 1) over the device leaves"""
    from mxfusion_amd.util.inference import VariablesDict
    gp = m.Y.factor
    post = gp._extra_graphs[0]
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).cuda()[None]
    kp = gp.kernel.parameters
    vs = VariablesDict({m.X.uuid: d(p['X'] if X is None else X), m.Z.uuid: leaves['Z'], post.qU_mean.uuid: leaves['qm'],
                        post.qU_cov_W.uuid: leaves['qW'], post.qU_cov_diag.uuid: leaves['qd']})
    if Y is not False:
        vs[m.Y.uuid] = d(p['Y'] if Y is None else Y)
    for short, name in _kernel_names(which).items():
        vs[kp[name].uuid] = leaves[short]
    if with_mean:
        vs[m.mean.uuid] = d(p['mean'])
    return vs


def _leaves(which, p, dtype, device):
    names = ['Z', 'qm', 'qW', 'qd'] + list(_kernel_names(which))
    mk = lambda a: torch.as_tensor(a, dtype=dtype, device=device)
    return {n: (mk(p[n])[None] if device == 'cuda' else mk(p[n]).double()).requires_grad_(True) for n in names}


def _ref_bound(which, kind, p, lv, scaling, with_mean, dtype, jitter=1e-6):
    r = lambda a: torch.as_tensor(a, dtype=dtype).double()
    K, Kd = R.make_kernel(which, lv)
    return R.svgp_bound(kind, K, Kd, r(p['X']), r(p['Y']), lv['Z'], lv['qm'], lv['qW'], lv['qd'], jitter=jitter, scaling=scaling,
                        mean=r(p['mean']) if with_mean else None)


CASES = [(w, k, P, False, torch.float64) for w in ('rbf', 'rbf+linear') for k in R.KINDS for P in (1, 2)]
CASES += [('rbf', 'bernoulli_logit', 2, True, torch.float64)]
CASES += [('rbf+linear', k, 2, k == 'poisson_exp', torch.float32) for k in R.KINDS]


@pytest.mark.parametrize('which,kind,P,with_mean,dtype', CASES,
                         ids=['%s-%s-P%d%s-%s' % (w, k, P, '-mean' if mn else '', 'f32' if dt == torch.float32 else 'f64') for w, k, P, mn, dt in CASES])
def test_bound_and_gradients(which, kind, P, with_mean, dtype):
    p = _data(kind, P)
    m = _module(which, kind, P, 'float32' if dtype == torch.float32 else 'float64', with_mean)
    alg = m.Y.factor.svgp_log_pdf
    alg.jitter, alg.log_pdf_scaling = 1e-6, 4
    dev = _leaves(which, p, dtype, 'cuda')
    got = alg.compute(None, _variables(m, which, p, dev, dtype, with_mean))
    assert got.shape == (1,) and got.dtype == dtype and int(alg._last_info.abs().sum()) == 0
    names = list(dev)
    ggot = torch.autograd.grad(got.sum(), [dev[n] for n in names])
    cpu = _leaves(which, p, dtype, 'cpu')
    ref = _ref_bound(which, kind, p, cpu, 4.0, with_mean, dtype)
    gref = torch.autograd.grad(ref, [cpu[n] for n in names])
    f64 = dtype == torch.float64
    assert abs(float(got.detach()) - float(ref)) <= (1e-8 if f64 else 1e-4) * abs(float(ref)) + (0 if f64 else 1e-5), (float(got.detach()), float(ref))
    for n, a, b in zip(names, ggot, gref):
        a, b = a[0].double().cpu().numpy(), b.numpy()
        if f64:
            assert np.allclose(a, b, rtol=1e-6, atol=1e-7 * float(np.abs(b).max())), (n, float(np.abs(a - b).max()), float(np.abs(b).max()))
        else:
            assert np.allclose(a, b, rtol=1e-4, atol=1e-5), (n, float(np.abs(a - b).max()), float(np.abs(b).max()))
    if f64 and P == 2 and which == 'rbf':
        # kl_weight = 1/2 with the scaling doubled: w (c / w data - KL) = 1/2 (16 data - KL)
        alg.kl_weight, alg.log_pdf_scaling = 0.5, 8
        with torch.no_grad():
            got2 = alg.compute(None, _variables(m, which, p, dev, dtype, with_mean))
        ref2 = 0.5 * _ref_bound(which, kind, p, cpu, 16.0, with_mean, dtype)
        assert abs(float(got2) - float(ref2)) <= 1e-8 * abs(float(ref2))
        assert alg.log_pdf_scaling == 8


@pytest.mark.parametrize('kind', R.KINDS)
def test_prediction(kind):
    """latent: the moments of q(f) equal SVGPRegressionMeanVariancePrediction (noise-free, diagonal) on a regression module with the same Z,
    kernel and q(u), at 1e-10; observations: (E[y], Var[y]) equal the reference at the kernel bars, Var[y] >= 0"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import SVGPRegression
    from mxfusion_amd.util.inference import VariablesDict
    P, dtype = 2, torch.float64
    p = _data(kind, P, seed=3)
    Xt = np.random.default_rng(9).uniform(-2.5, 2.5, (33, Q))
    m = _module('rbf', kind, P)
    gp = m.Y.factor
    alg = gp.svgp_predict
    alg.jitter = 1e-6
    dev = {n: t.detach() for n, t in _leaves('rbf', p, dtype, 'cuda').items()}
    vs = _variables(m, 'rbf', p, dev, dtype, X=Xt, Y=False)
    alg.latent, alg.target_variables = True, None
    mean_f, var_f = alg.compute(None, vs)[m.Y.uuid]
    # the regression module over the same inducing points
    r = Model()
    r.N = Variable()
    r.X = Variable(shape=(r.N, Q))
    r.Z = Variable(shape=(M, Q))
    r.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    r.Y = SVGPRegression.define_variable(X=r.X, kernel=RBF(input_dim=Q, ARD=True, dtype='float64'), noise_var=r.noise_var, inducing_inputs=r.Z,
                                         shape=(r.N, P), dtype='float64')
    rg = r.Y.factor
    rpost, rk = rg._extra_graphs[0], rg.kernel.parameters
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).cuda()[None]
    rvs = VariablesDict({r.X.uuid: d(Xt), r.Z.uuid: dev['Z'], r.noise_var.uuid: d([0.1]), rpost.qU_mean.uuid: dev['qm'], rpost.qU_cov_W.uuid: dev['qW'],
                         rpost.qU_cov_diag.uuid: dev['qd'], rk['rbf_lengthscale'].uuid: dev['ls'], rk['rbf_variance'].uuid: dev['var']})
    ralg = rg.svgp_predict
    ralg.jitter, ralg.noise_free, ralg.diagonal_variance, ralg.target_variables = 1e-6, True, True, None
    mean_r, var_r = ralg.compute(None, rvs)[r.Y.uuid]
    assert mean_f.shape == mean_r.shape and var_f.shape == var_r.shape
    assert torch.allclose(mean_f, mean_r, rtol=1e-10, atol=1e-10) and torch.allclose(var_f, var_r, rtol=1e-10, atol=1e-10)
    # observation space
    alg.latent = False
    ey, vy = alg.compute(None, vs)[m.Y.uuid]
    cpu = {n: torch.as_tensor(p[n]) for n in ('Z', 'qm', 'qW', 'qd', 'ls', 'var')}
    K, Kd = R.make_kernel('rbf', cpu)
    mr, vr, _ = R.marginals(K, Kd, torch.as_tensor(Xt), cpu['Z'], cpu['qm'], cpu['qW'], cpu['qd'], jitter=1e-6)
    ey_r, vy_r = R.predictive(kind, mr, vr)
    assert ey.shape == (1, 33, P) and vy.shape == (1, 33, P)
    assert np.allclose(ey[0].cpu().numpy(), ey_r.numpy(), rtol=1e-9, atol=1e-11) and np.allclose(vy[0].cpu().numpy(), vy_r.numpy(), rtol=1e-9, atol=1e-11)
    assert float(vy.min()) >= 0.0


def _classification_model():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.modules.gp_modules import SVGPLikelihood, BernoulliLogit
    rng = np.random.default_rng(1)
    X = np.sort(rng.uniform(-2.0, 2.0, (200, 1)), 0)
    Y = (np.sin(3 * X) > 0).astype(np.float64)
    m = Model()
    m.N = Variable()
    m.X = Variable(shape=(m.N, 1))
    m.Z = Variable(shape=(10, 1), initial_value=torch.as_tensor(np.linspace(-2, 2, 10)[:, None]).cuda())
    m.Y = SVGPLikelihood.define_variable(X=m.X, kernel=RBF(input_dim=1, ARD=True, dtype='float64'), likelihood=BernoulliLogit(),
                                         inducing_inputs=m.Z, shape=(m.N, 1), dtype='float64')
    m.Y.factor.svgp_log_pdf.jitter = 1e-6
    m.Y.factor.svgp_predict.jitter = 1e-6
    return m, X, Y


def _read_back(m, infr):
    """the trained parameters as float64 CPU tensors shaped like their Variables"""
    gp = m.Y.factor
    post, kern = gp._extra_graphs[0], gp.kernel
    val = lambda v: infr.params[v].detach().double().cpu().reshape(tuple(v.shape))
    return dict(Z=val(m.Z), qm=val(post.qU_mean), qW=val(post.qU_cov_W), qd=val(post.qU_cov_diag), ls=val(kern.lengthscale), var=val(kern.variance))


def _device_bound(m, cpu, X, Y):
    dev = {n: t.cuda()[None] for n, t in cpu.items()}
    with torch.no_grad():
        return float(m.Y.factor.svgp_log_pdf.compute(None, _variables(m, 'rbf', dict(X=X, Y=Y), dev, torch.float64)))


def test_training_raises_the_bound_and_the_reference_reproduces_it():
    from mxfusion_amd.inference import GradBasedInference, MAP, TransferInference, ModulePredictionAlgorithm
    m, X, Y = _classification_model()
    Xd, Yd = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
    infr = GradBasedInference(MAP(model=m, observed=[m.X, m.Y]), dtype='float64')
    infr.initialize(X=X.shape, Y=Y.shape)
    start = _device_bound(m, _read_back(m, infr), X, Y)
    infr.run(X=Xd, Y=Yd, max_iter=150, learning_rate=0.05)
    cpu = _read_back(m, infr)
    end = _device_bound(m, cpu, X, Y)
    assert np.isfinite(start) and end > start, (start, end)
    K, Kd = R.make_kernel('rbf', cpu)
    ref = R.svgp_bound('bernoulli_logit', K, Kd, torch.as_tensor(X), torch.as_tensor(Y), cpu['Z'], cpu['qm'], cpu['qW'], cpu['qd'], jitter=1e-6)
    assert abs(end - float(ref)) <= 1e-8 * abs(float(ref)), (end, float(ref))
    pred = TransferInference(ModulePredictionAlgorithm(m, observed=[m.X], target_variables=[m.Y]), infr_params=infr.params, dtype='float64')
    ey, vy = pred.run(X=Xd)[0]
    mr, vr, _ = R.marginals(K, Kd, torch.as_tensor(X), cpu['Z'], cpu['qm'], cpu['qW'], cpu['qd'], jitter=1e-6)
    ey_r, _ = R.predictive('bernoulli_logit', mr, vr)
    assert np.allclose(ey.reshape(200, 1).cpu().numpy(), ey_r.numpy(), rtol=1e-6, atol=1e-7)
    assert float(vy.min()) >= 0.0


def test_minibatch_step():
    from mxfusion_amd.inference import GradBasedInference, MAP, MinibatchInferenceLoop
    m, X, Y = _classification_model()
    loop = MinibatchInferenceLoop(batch_size=64, rv_scaling={m.Y: 200 / 64})
    infr = GradBasedInference(MAP(model=m, observed=[m.X, m.Y]), grad_loop=loop, dtype='float64')
    infr.run(X=torch.as_tensor(X).cuda(), Y=torch.as_tensor(Y).cuda(), max_iter=1, learning_rate=0.01)
    assert len(loop.epoch_losses) == 1 and np.isfinite(float(loop.epoch_losses[0]))
    assert m.Y.factor.svgp_log_pdf.log_pdf_scaling == 200 / 64
    assert bool(torch.isfinite(infr.params.flat).all())
