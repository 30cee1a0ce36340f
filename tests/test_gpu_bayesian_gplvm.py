"""BayesianGPLVM on the GPU against tests/_psi_ref.py: the bound and the gradients in X_mean, the raw (pre-softplus) X_var, Z, the kernel
parameters and noise_var at N = 40, M = 7, Q = 2, P = 3 and at N = 130, M = 17, Q = 3, P = 1, float64 and float32, at the initial point and at a
perturbed one; the noisy-input form at X_var = 0 against SparseGPRegression; prediction; a training run; the checkpoint round trip; the
refusal of minibatches; the unsupported kernels.  Bars of tests/test_gpu_svgp_likelihood.py: value rtol 1e-8, gradients rtol 1e-6 with atol
1e-7 max|g|; float32 rtol 1e-4, atol 1e-5."""
import functools

import numpy as np
import pytest
import torch

import _psi_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(40, 7, 2, 3), (130, 17, 3, 1)]
JITTER = 1e-6
NAMES = ('mu', 'raw', 'Z', 'ls', 'var', 'noise')


def _data(size, perturbed=False):
    """Float32 statistics carry a rounding of 2^-24 of their entries whatever the kernel does, and the bound multiplies it by its sensitivity
    |dF / dPsi2| ~ P / (2 noise) |Kuu^-1|.  For the float32 bars to be within reach of the number format the problem is kept well conditioned:
    inducing points chosen greedily as far apart as possible (no near-duplicate rows of Kuu) and noise_var = 0.5.  (Measured with the first
    M rows as inducing points and noise_var = 0.1 instead: float64 agreed to 1e-13 of the largest gradient entry, the float32 bound to 7e-7,
    and three of the four float32 cases missed the gradient bar on small entries -- largest errors 6.4e-4 in dZ of magnitude 34, 3.8e-4 and
    4.6e-4 in dX_mean of magnitude 15.7 and 4.9: 2e-5 to 9e-5 of the largest entry, the rounding of Psi2 times that sensitivity.)"""
    N, M, Q, P = size
    rng = np.random.default_rng(N + 7 * int(perturbed))
    mu = rng.uniform(-2.0, 2.0, (N, Q))
    Y = np.sin(mu @ rng.standard_normal((Q, P))) + 0.1 * rng.standard_normal((N, P))
    pick = [0]
    for _ in range(M - 1):
        pick.append(int(np.argmax(np.min(((mu[:, None] - mu[pick][None]) ** 2).sum(-1), 1))))
    p = dict(mu=mu, raw=rng.uniform(-2.0, 0.5, (N, Q)), Z=mu[pick] + 0.1 * rng.standard_normal((M, Q)), ls=rng.uniform(0.8, 1.4, Q), var=np.array([1.3]),
             noise=np.array([0.5]), Y=Y, Xt=rng.uniform(-2.5, 2.5, (23, Q)))
    if perturbed:
        for k in NAMES:
            p[k] = p[k] + 0.05 * rng.standard_normal(p[k].shape) * (1.0 if k in ('mu', 'raw', 'Z') else 0.2)
    return p


def _module(size, dtype='float64', latent_prior=True, given=False, kernel=None):
    """given: X_mean and X_var are variables of the outer model; otherwise the module creates them"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import BayesianGPLVM
    N, M, Q, P = size
    m = Model()
    m.Z = Variable(shape=(M, Q))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    if given:
        m.X_mean = Variable(shape=(N, Q))
        m.X_var = Variable(shape=(N, Q))
    m.Y = BayesianGPLVM.define_variable(kernel=RBF(input_dim=Q, ARD=True, dtype=dtype) if kernel is None else kernel, noise_var=m.noise_var,
                                        shape=(N, P), X_mean=m.X_mean if given else None, X_var=m.X_var if given else None,
                                        latent_prior=latent_prior, inducing_inputs=m.Z, dtype=dtype)
    m.Y.factor.gplvm_log_pdf.jitter = JITTER
    return m


def _variables(m, p, lv, s, dtype):
    """the runtime dict of the module's algorithms (leading sample axis 1); s: the variances on the device"""
    from mxfusion_amd.util.inference import VariablesDict
    gp = m.Y.factor
    g, kp = gp._module_graph, gp.kernel.parameters
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).cuda()[None]
    return VariablesDict({g.X.uuid: lv['mu'], g.X_var.uuid: s, m.Z.uuid: lv['Z'], m.noise_var.uuid: lv['noise'], m.Y.uuid: d(p['Y']),
                          kp['rbf_lengthscale'].uuid: lv['ls'], kp['rbf_variance'].uuid: lv['var']})


def _leaves(p, dtype, device):
    mk = lambda a: torch.as_tensor(a, dtype=dtype, device=device)
    return {n: (mk(p[n])[None] if device == 'cuda' else mk(p[n]).double()).requires_grad_(True) for n in NAMES}


@functools.lru_cache(maxsize=None)
def _reference(size, perturbed, rounded):
    """the bound with its prior term and its gradients, float64 on the CPU, at the values the run sees"""
    p = _data(size, perturbed)
    lv = _leaves(p, torch.float32 if rounded else torch.float64, 'cpu')
    Y = torch.as_tensor(p['Y'], dtype=torch.float32 if rounded else torch.float64).double()
    F = R.bound(lv['mu'], torch.nn.functional.softplus(lv['raw']), lv['Z'], lv['ls'], lv['var'], lv['noise'], Y, jitter=JITTER, latent_prior=True)
    return float(F.detach()), [g.numpy() for g in torch.autograd.grad(F, [lv[n] for n in NAMES])]


@pytest.mark.parametrize('perturbed', [False, True], ids=['initial', 'perturbed'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('size', SIZES, ids=['N40-M7-Q2-P3', 'N130-M17-Q3-P1'])
def test_bound_and_gradients(size, dtype, perturbed):
    from mxfusion_amd.components.variables import PositiveTransformation
    f64 = dtype == torch.float64
    p = _data(size, perturbed)
    m = _module(size, 'float64' if f64 else 'float32')
    alg = m.Y.factor.gplvm_log_pdf
    dev = _leaves(p, dtype, 'cuda')
    got = alg.compute(None, _variables(m, p, dev, PositiveTransformation().transform(dev['raw']), dtype))
    assert got.shape == (1,) and got.dtype == dtype and int(alg._last_info.abs().sum()) == 0
    ggot = torch.autograd.grad(got.sum(), [dev[n] for n in NAMES])
    ref, gref = _reference(size, perturbed, not f64)
    print('bound', float(got.detach()), 'reference', ref)
    assert abs(float(got.detach()) - ref) <= (1e-8 if f64 else 1e-4) * abs(ref) + (0 if f64 else 1e-5), (float(got.detach()), ref)
    for n, a, b in zip(NAMES, ggot, gref):
        a = a[0].double().cpu().numpy().reshape(b.shape)
        print('d' + n, 'max error', float(np.abs(a - b).max()), 'max', float(np.abs(b).max()))
        if f64:
            assert np.allclose(a, b, rtol=1e-6, atol=1e-7 * float(np.abs(b).max())), (n, float(np.abs(a - b).max()), float(np.abs(b).max()))
        else:
            assert np.allclose(a, b, rtol=1e-4, atol=1e-5), (n, float(np.abs(a - b).max()), float(np.abs(b).max()))


@pytest.mark.parametrize('size', SIZES, ids=['N40-M7-Q2-P3', 'N130-M17-Q3-P1'])
def test_zero_input_variance_is_the_sparse_gp(size):
    """X_var observed as zeros, latent_prior=False: the bound is SparseGPRegression's log-pdf on X = X_mean"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import SparseGPRegression
    from mxfusion_amd.util.inference import VariablesDict
    N, M, Q, P = size
    p = _data(size)
    m = _module(size, latent_prior=False, given=True)
    dev = {n: t.detach() for n, t in _leaves(p, torch.float64, 'cuda').items()}
    with torch.no_grad():
        got = m.Y.factor.gplvm_log_pdf.compute(None, _variables(m, p, dev, torch.zeros_like(dev['mu']), torch.float64))
    r = Model()
    r.X = Variable(shape=(N, Q))
    r.Z = Variable(shape=(M, Q))
    r.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    r.Y = SparseGPRegression.define_variable(X=r.X, kernel=RBF(input_dim=Q, ARD=True, dtype='float64'), noise_var=r.noise_var, inducing_inputs=r.Z,
                                             shape=(N, P), dtype='float64')
    rk = r.Y.factor.kernel.parameters
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).cuda()[None]
    ralg = r.Y.factor.sgp_log_pdf
    ralg.jitter = JITTER
    with torch.no_grad():
        ref = ralg.compute(None, VariablesDict({r.X.uuid: dev['mu'], r.Z.uuid: dev['Z'], r.noise_var.uuid: dev['noise'], r.Y.uuid: d(p['Y']),
                                                rk['rbf_lengthscale'].uuid: dev['ls'], rk['rbf_variance'].uuid: dev['var']}))
    cpu = {n: torch.as_tensor(p[n]) for n in NAMES}
    rest = R.bound(cpu['mu'], torch.zeros_like(cpu['mu']), cpu['Z'], cpu['ls'], cpu['var'], cpu['noise'], torch.as_tensor(p['Y']), jitter=JITTER)
    print('gplvm', float(got), 'sparse gp', float(ref), 'restatement', float(rest))
    assert abs(float(got) - float(ref)) <= 1e-8 * abs(float(ref)), (float(got), float(ref))
    assert abs(float(got) - float(rest)) <= 1e-8 * abs(float(rest)), (float(got), float(rest))


def test_prediction():
    """the mean and the variance of the module's prediction algorithm at deterministic test inputs, from the posterior the bound persisted"""
    from mxfusion_amd.components.variables import PositiveTransformation
    size = SIZES[0]
    p = _data(size)
    m = _module(size)
    gp = m.Y.factor
    dev = {n: t.detach() for n, t in _leaves(p, torch.float64, 'cuda').items()}
    vs = _variables(m, p, dev, PositiveTransformation().transform(dev['raw']), torch.float64)
    with torch.no_grad():
        gp.gplvm_log_pdf.compute(None, vs)
    from mxfusion_amd.inference.inference_alg import SET_PARAMETER_PREFIX
    for v in gp._extra_graphs[0].get_parameters():           # what the inference writes back after compute: L, LA, wv of sample 0
        var, value = vs[SET_PARAMETER_PREFIX + v.uuid]
        assert var is v and tuple(value.shape) == tuple(v.shape)
        vs[v.uuid] = value[None]
    vs[gp._module_graph.X.uuid] = torch.as_tensor(p['Xt']).cuda()[None]
    alg = gp.gplvm_predict
    alg.target_variables = None
    mean, var = alg.compute(None, vs)[m.Y.uuid]
    cpu = {n: torch.as_tensor(p[n]) for n in NAMES}
    mr, vr = R.predict(torch.as_tensor(p['Xt']), cpu['mu'], torch.nn.functional.softplus(cpu['raw']), cpu['Z'], cpu['ls'], cpu['var'], cpu['noise'],
                       torch.as_tensor(p['Y']), jitter=JITTER)
    assert mean.shape == (1, 23, size[3]) and var.shape == (1, 23)
    assert np.allclose(mean[0].cpu().numpy(), mr.numpy(), rtol=1e-6, atol=1e-8) and np.allclose(var[0].cpu().numpy(), vr.numpy(), rtol=1e-6, atol=1e-8)


def _cluster_model():
    """three well-separated 1-D clusters embedded in 5-D; q(X) starts at the first principal component"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import BayesianGPLVM
    rng = np.random.default_rng(5)
    t = np.repeat([-2.0, 0.0, 2.0], 20) + 0.1 * rng.standard_normal(60)
    Y = np.tanh(t)[:, None] * rng.standard_normal((1, 5)) + 0.05 * rng.standard_normal((60, 5))
    Yc = Y - Y.mean(0)
    pc = Yc @ np.linalg.svd(Yc, full_matrices=False)[2][0]
    m = Model()
    m.X_mean = Variable(shape=(60, 1), initial_value=torch.as_tensor((pc / pc.std())[:, None]).cuda())
    m.X_var = Variable(shape=(60, 1), transformation=PositiveTransformation(), initial_value=0.5)
    m.Z = Variable(shape=(8, 1), initial_value=torch.as_tensor(np.linspace(-2, 2, 8)[:, None]).cuda())
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    m.Y = BayesianGPLVM.define_variable(kernel=RBF(input_dim=1, ARD=True, dtype='float64'), noise_var=m.noise_var, shape=(60, 5), X_mean=m.X_mean,
                                        X_var=m.X_var, inducing_inputs=m.Z, dtype='float64')
    m.Y.factor.gplvm_log_pdf.jitter = JITTER
    return m, Yc


def test_training_lowers_the_loss():
    """fifty Adam steps: the loss falls monotonically after the first ten"""
    from mxfusion_amd.inference import GradBasedInference, MAP
    from mxfusion_amd.inference.batch_loop import BatchInferenceLoop

    class Recording(BatchInferenceLoop):
        losses = []

        def step(self, *args):
            loss = super(Recording, self).step(*args)
            self.losses.append(float(loss.detach()))
            return loss

    m, Y = _cluster_model()
    loop = Recording()
    infr = GradBasedInference(MAP(model=m, observed=[m.Y]), grad_loop=loop, dtype='float64')
    infr.run(Y=torch.as_tensor(Y).cuda(), max_iter=50, learning_rate=0.02)
    L = np.array(loop.losses[:50])
    print('losses', L[[0, 10, 20, 30, 40, 49]])
    assert len(L) == 50 and np.isfinite(L).all() and L[49] < L[0]
    assert (np.diff(L[10:]) < 0).all(), L


def test_checkpoint_round_trip(tmp_path):
    """the module's own q(X), created inside it, and every other parameter come back from a checkpoint"""
    from mxfusion_amd.inference import GradBasedInference, MAP
    size = SIZES[0]
    p = _data(size)
    Y = torch.as_tensor(p['Y']).cuda()
    m = _module(size)
    infr = GradBasedInference(MAP(model=m, observed=[m.Y]), dtype='float64')
    infr.run(Y=Y, max_iter=3, learning_rate=0.01)
    z = str(tmp_path / 'gplvm.zip')
    infr.save(z)
    m2 = _module(size)
    infr2 = GradBasedInference(MAP(model=m2, observed=[m2.Y]), dtype='float64')
    infr2.initialize(Y=Y)
    infr2.load(z)
    g, g2 = m.Y.factor._module_graph, m2.Y.factor._module_graph
    assert infr2._uuid_map[g.X.uuid] == g2.X.uuid and infr2._uuid_map[g.X_var.uuid] == g2.X_var.uuid
    assert len(infr.params._slices) >= 6
    for u in infr.params._slices:
        assert torch.equal(infr.params.raw(u), infr2.params.raw(infr2._uuid_map[u])), u


def test_minibatches_are_refused():
    from mxfusion_amd.common.exceptions import InferenceError
    from mxfusion_amd.inference import GradBasedInference, MAP, MinibatchInferenceLoop
    m, Y = _cluster_model()
    loop = MinibatchInferenceLoop(batch_size=20, rv_scaling={m.Y: 3.0})
    infr = GradBasedInference(MAP(model=m, observed=[m.Y]), grad_loop=loop, dtype='float64')
    with pytest.raises(InferenceError, match='not a sum over data rows'):
        infr.run(Y=torch.as_tensor(Y).cuda(), max_iter=1, learning_rate=0.01)
    assert m.Y.factor.row_additive is False


def test_unsupported_kernels_are_named():
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Matern52, Linear
    for kernel in (Matern52(input_dim=2, dtype='float64'), RBF(input_dim=2, dtype='float64') + Linear(input_dim=2, dtype='float64'),
                   RBF(input_dim=1, active_dims=[0], dtype='float64')):
        with pytest.raises(ModelSpecificationError, match='single RBF kernel'):
            _module(SIZES[0], kernel=kernel)
    with pytest.raises(ModelSpecificationError, match='must be an integer'):
        from mxfusion_amd import Model, Variable
        from mxfusion_amd.modules.gp_modules import BayesianGPLVM
        m = Model()
        m.N = Variable()
        BayesianGPLVM.define_variable(kernel=RBF(input_dim=2, dtype='float64'), noise_var=Variable(shape=(1,)), shape=(m.N, 3))
