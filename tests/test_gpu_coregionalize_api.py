"""Multi-output GP regression through the public surface: RBF * Coregionalize in GPRegression on two outputs observed at different inputs,
against a dense float64 torch restatement (Cholesky over tests/_coreg_ref.py) at 1e-8 relative -- the bar of
tests/test_gpu_kernels_diff_api.py on this path -- through the fused pass (mxf_gram_icm) and through the generic path."""
import numpy as np
import pytest
import torch

import _coreg_ref as R

pytestmark = pytest.mark.gpu
DT = torch.float64
Q = 2
VALS = dict(var=1.3, ls=[0.9, 1.6], W=[[0.7], [-0.4]], kappa=[0.3, 0.6], noise=0.05)


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=DT).cuda()


@pytest.fixture(autouse=True)
def fused_everywhere(monkeypatch):
    """the tests exercise the fused branch whatever the measured defaults are"""
    from mxfusion_amd.components.distributions.gp.kernels import kernel as impl
    monkeypatch.setattr(impl, 'FUSED_ICM', {torch.float32: True, torch.float64: True})


def _generic(monkeypatch):
    from mxfusion_amd.components.distributions.gp.kernels import kernel as impl
    monkeypatch.setattr(impl, 'FUSED_ICM', {torch.float32: False, torch.float64: False})


def _data(seed=0, n0=37, n1=23):
    from mxfusion_amd.components.distributions.gp.kernels import Coregionalize
    rng = np.random.default_rng(seed)
    Xs = [rng.uniform(-2, 2, (n0, Q)), rng.uniform(-2, 2, (n1, Q))]
    f = lambda x: np.sin(1.3 * x[:, :1]) + 0.5 * np.cos(x[:, 1:])
    Ys = [f(Xs[0]) + 0.05 * rng.standard_normal((n0, 1)), 0.8 * f(Xs[1]) + 0.3 + 0.05 * rng.standard_normal((n1, 1))]
    X, Y = Coregionalize.stack(Xs, Ys)
    return Xs, Ys, X, Y


def _icm_kernel(T=2):
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Coregionalize
    rbf = RBF(Q, ARD=True, variance=VALS['var'], lengthscale=_t(VALS['ls']), active_dims=range(Q), dtype=DT)
    W = np.zeros((T, 1)); W[:2] = VALS['W']
    kappa = np.ones(T); kappa[:2] = VALS['kappa']
    return rbf, Coregionalize(T, rank=1, W=W, kappa=kappa, active_dims=[Q], dtype=DT)


def _model(kernel, noise=VALS['noise']):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import GPRegression
    m = Model()
    m.N = Variable()
    m.X = Variable(shape=(m.N, Q + 1))
    m.noise_var = Variable(transformation=PositiveTransformation(), initial_value=_t([noise]))
    m.Y = GPRegression.define_variable(X=m.X, kernel=kernel, noise_var=m.noise_var, shape=(m.N, 1), dtype=DT)
    return m


def _logpdf(kernel, X, Y, noise=VALS['noise']):
    from mxfusion_amd.inference import Inference, MAP
    m = _model(kernel, noise)
    infr = Inference(MAP(model=m, observed=[m.X, m.Y]), dtype=DT)
    loss, _ = infr.run(X=_t(X), Y=_t(Y))
    return -float(loss), m, infr


def _ref_K(X, X2, var, ls, W, kappa, T=2):
    """the restated ICM Gram of augmented inputs (N, Q + 1) float64 CPU tensors"""
    B = R.coreg_matrix(kappa[None], None if W is None else W[None])
    i = X[:, Q].numpy().astype(np.int64)
    j = None if X2 is None else X2[:, Q].numpy().astype(np.int64)
    return R.icm('rbf', X[None, :, :Q], None if X2 is None else X2[None, :, :Q], i, j, ls[None], var[None], B)[0]


def _ref_logpdf(X, Y, var, ls, W, kappa, noise):
    return R.gp_logpdf(_ref_K(X, None, var, ls, W, kappa) + noise * torch.eye(X.shape[0], dtype=DT), Y)


def _leaves():
    return {n: torch.tensor(np.atleast_1d(v), dtype=DT) for n, v in VALS.items()}


def _first_gradient(kernel, X, Y):
    from mxfusion_amd.inference import GradBasedInference, MAP, BatchInferenceLoop
    m = _model(kernel)
    grads = []

    class Rec(BatchInferenceLoop):
        def _exchange(self, param_dict, loss):
            grads.append(param_dict.flat.grad.clone())
            return loss
    infr = GradBasedInference(inference_algorithm=MAP(model=m, observed=[m.X, m.Y]), grad_loop=Rec(), dtype=DT)
    infr.run(X=_t(X), Y=_t(Y), max_iter=1, learning_rate=1e-3)
    return m, infr.params, grads[0]


def test_logpdf_and_its_gradient_in_every_parameter(monkeypatch):
    """fused and generic (the branch switched off: the path MultiplyKernel took before), each against the restatement and against each
    other: log-pdf 1e-8 relative; the gradient in the raw (pre-softplus) parameters rtol 1e-8, atol 1e-8 max|gradient|"""
    _, _, X, Y = _data()
    Xc, Yc = torch.as_tensor(X), torch.as_tensor(Y)
    sp, inv = torch.nn.functional.softplus, lambda v: torch.log(torch.expm1(v))
    L = _leaves()
    raw = {n: (L[n].clone() if n == 'W' else inv(L[n])).requires_grad_(True) for n in L}
    val = lambda n: raw[n] if n == 'W' else sp(raw[n])
    ref = _ref_logpdf(Xc, Yc, val('var'), val('ls'), val('W'), val('kappa'), val('noise'))
    want = dict(zip(raw, torch.autograd.grad(-ref, list(raw.values()))))
    gmax = max(float(w.abs().max()) for w in want.values())
    results = {}
    for route in ('fused', 'generic'):
        if route == 'generic':
            _generic(monkeypatch)
        rbf, coreg = _icm_kernel()
        got, _, _ = _logpdf(rbf * coreg, X, Y)
        assert abs(got - float(ref.detach())) <= 1e-8 * abs(float(ref.detach())), (route, got, float(ref.detach()))
        rbf, coreg = _icm_kernel()
        m, P, g = _first_gradient(rbf * coreg, X, Y)
        variables = dict(var=rbf.variance, ls=rbf.lengthscale, W=coreg.W, kappa=coreg.kappa, noise=m.noise_var)
        for n, v in variables.items():
            o, cnt = P._slices[v.uuid][0], P._slices[v.uuid][1]
            assert cnt == want[n].numel() and np.allclose(g[o:o + cnt].cpu().numpy(), want[n].numpy().ravel(), rtol=1e-8, atol=1e-8 * gmax), (route, n, g[o:o + cnt], want[n])
        results[route] = (got, g.cpu().numpy())
    assert abs(results['fused'][0] - results['generic'][0]) <= 1e-8 * abs(results['fused'][0])
    assert np.allclose(results['fused'][1], results['generic'][1], rtol=1e-8, atol=1e-8 * gmax)


def test_the_fused_branch_is_taken_and_only_where_it_applies(monkeypatch):
    from mxfusion_amd import ops
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Coregionalize, Periodic, MultiplyKernel
    calls = []
    real = ops.gram_icm
    monkeypatch.setattr(ops, 'gram_icm', lambda *a, **k: calls.append(1) or real(*a, **k))
    _, _, X, _ = _data()
    Xd = _t(X)[None]
    vals = lambda k: {n: _t(np.broadcast_to(np.asarray(v.initial_value.cpu() if torch.is_tensor(v.initial_value) else v.initial_value, dtype=np.float64),
                                            tuple(v.shape)).copy())[None] for n, v in k.parameters.items()}
    rbf, coreg = _icm_kernel()
    for k in (rbf * coreg, coreg * rbf):
        n = len(calls)
        k.K(torch, Xd, **vals(k))
        assert len(calls) == n + 1
    n = len(calls)
    three = MultiplyKernel([RBF(Q, active_dims=range(Q), dtype=DT), Coregionalize(2, active_dims=[Q], dtype=DT), RBF(1, name='r2', active_dims=[0], dtype=DT)])
    overlap = RBF(Q + 1, dtype=DT) * Coregionalize(2, active_dims=[Q], dtype=DT)
    other = Periodic(Q, active_dims=range(Q), dtype=DT) * Coregionalize(2, active_dims=[Q], dtype=DT)
    for k in (three, overlap, other):
        k.K(torch, Xd, **vals(k))
    assert len(calls) == n
    # more samples than one launch's grid takes (65 535): the branch declines instead of handing the entry point a request it refuses
    k = rbf * coreg
    p = vals(k)
    p['mul_rbf_variance'] = p['mul_rbf_variance'].expand(65536, 1)
    assert k._fused_icm(Xd, None, k._strip(p)) is None and k._fused_icm(Xd, None, k._strip(vals(k))) is not None


def test_prediction_of_output_1_where_only_output_0_was_observed():
    from mxfusion_amd.inference import TransferInference, ModulePredictionAlgorithm
    Xs, _, X, Y = _data()
    rbf, coreg = _icm_kernel()
    _, m, infr = _logpdf(rbf * coreg, X, Y)
    Xt = np.concatenate([Xs[0], np.ones((Xs[0].shape[0], 1))], 1)
    infr2 = TransferInference(ModulePredictionAlgorithm(m, observed=[m.X], target_variables=[m.Y]), infr_params=infr.params, dtype=DT)
    gp = infr2.inference_algorithm.model.Y.factor
    gp.gp_predict.noise_free, gp.gp_predict.diagonal_variance = True, True
    mu, var = infr2.run(X=_t(Xt))[0]
    L = _leaves()
    Xc, Xtc = torch.as_tensor(X), torch.as_tensor(Xt)
    K = _ref_K(Xc, None, L['var'], L['ls'], L['W'], L['kappa']) + L['noise'] * torch.eye(X.shape[0], dtype=DT)
    Ks = _ref_K(Xc, Xtc, L['var'], L['ls'], L['W'], L['kappa'])
    B11 = float(L['W'][1, 0] ** 2 + L['kappa'][1])
    rmu, rvar = R.gp_predict(K, Ks, torch.full((Xt.shape[0],), float(L['var']) * B11, dtype=DT), torch.as_tensor(Y))
    assert np.allclose(mu.cpu().numpy().reshape(-1), rmu.numpy().reshape(-1), rtol=1e-8, atol=1e-8 * float(rmu.abs().max()))
    assert np.allclose(var.cpu().numpy().reshape(-1), rvar.numpy().reshape(-1), rtol=1e-8, atol=1e-8 * float(rvar.abs().max()))


def test_w_zero_kappa_one_is_two_independent_gps():
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Coregionalize
    Xs, Ys, X, Y = _data()
    mk = lambda **kw: RBF(Q, ARD=True, variance=VALS['var'], lengthscale=_t(VALS['ls']), dtype=DT, **kw)
    coreg = Coregionalize(2, rank=1, W=np.zeros((2, 1)), kappa=np.ones(2), active_dims=[Q], dtype=DT)
    joint, _, _ = _logpdf(mk(active_dims=range(Q)) * coreg, X, Y)
    parts = 0.0
    for x, y in zip(Xs, Ys):
        pad = np.concatenate([x, np.zeros((x.shape[0], 1))], 1)         # the third column is not an active dimension of this kernel
        parts += _logpdf(mk(active_dims=range(Q)), pad, y)[0]
    assert abs(joint - parts) <= 1e-8 * abs(parts), (joint, parts)


def test_lmc_sum_and_per_output_noise():
    """the linear model of coregionalisation as a sum of two products, plus per-output noise White * Coregionalize(rank=0)"""
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Matern32, White, Coregionalize
    _, _, X, Y = _data()
    k1 = RBF(Q, ARD=True, variance=VALS['var'], lengthscale=_t(VALS['ls']), active_dims=range(Q), dtype=DT) \
        * Coregionalize(2, rank=1, W=VALS['W'], kappa=VALS['kappa'], active_dims=[Q], dtype=DT)
    k2 = Matern32(Q, variance=0.6, lengthscale=2.1, active_dims=range(Q), dtype=DT).multiply(
        Coregionalize(2, rank=1, W=[[0.2], [0.5]], kappa=[0.1, 0.2], name='coreg2', active_dims=[Q], dtype=DT), name='mul2')
    k3 = White(1, variance=1.0, active_dims=[Q], dtype=DT).multiply(Coregionalize(2, rank=0, kappa=[0.02, 0.11], name='coreg3', active_dims=[Q], dtype=DT), name='mul3')
    got, _, _ = _logpdf(k1 + k2 + k3, X, Y, noise=1e-3)
    Xc, L = torch.as_tensor(X), _leaves()
    i = Xc[:, Q].numpy().astype(np.int64)
    K = _ref_K(Xc, None, L['var'], L['ls'], L['W'], L['kappa'])
    B2 = R.coreg_matrix(R.t64([[0.1, 0.2]]), R.t64([[[0.2], [0.5]]]))
    K = K + R.icm('matern32', Xc[None, :, :Q], None, i, None, R.t64([[2.1]]), R.t64([[0.6]]), B2)[0]
    K = K + torch.diag(R.t64([0.02, 0.11])[i]) + 1e-3 * torch.eye(X.shape[0], dtype=DT)
    ref = float(R.gp_logpdf(K, torch.as_tensor(Y)))
    assert abs(got - ref) <= 1e-8 * abs(ref), (got, ref)


def test_t_33_takes_the_generic_path_and_agrees():
    from mxfusion_amd import ops
    _, _, X, Y = _data()
    rbf, coreg = _icm_kernel(T=33)
    calls = []
    real = ops.gram_icm
    try:
        ops.gram_icm = lambda *a, **k: calls.append(1) or real(*a, **k)
        got, _, _ = _logpdf(rbf * coreg, X, Y)
    finally:
        ops.gram_icm = real
    L = _leaves()
    W, kappa = torch.zeros(33, 1, dtype=DT), torch.ones(33, dtype=DT)
    W[:2], kappa[:2] = L['W'], L['kappa']
    ref = float(_ref_logpdf(torch.as_tensor(X), torch.as_tensor(Y), L['var'], L['ls'], W, kappa, L['noise']))
    assert not calls and abs(got - ref) <= 1e-8 * abs(ref), (calls, got, ref)


def test_twenty_adam_steps_learn_a_positive_output_correlation():
    """data drawn from a known B with off-diagonal correlation 0.9; from the defaults the loss decreases and the learnt correlation
    B01 / sqrt(B00 B11) is positive"""
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Coregionalize
    from mxfusion_amd.inference import GradBasedInference, MAP, BatchInferenceLoop
    rng = np.random.default_rng(5)
    Xs = [rng.uniform(-2, 2, (37, Q)), rng.uniform(-2, 2, (23, Q))]
    X = Coregionalize.stack(Xs)
    Xc = torch.as_tensor(X)
    Btrue = R.t64([[1.0, 0.9], [0.9, 1.0]])
    i = X[:, Q].astype(np.int64)
    K = R.icm('rbf', Xc[None, :, :Q], None, i, None, R.t64([[1.0]]), R.t64([[1.0]]), Btrue[None])[0] + 1e-6 * torch.eye(60, dtype=DT)
    Y = (torch.linalg.cholesky(K) @ torch.as_tensor(rng.standard_normal((60, 1)))).numpy() + 0.05 * rng.standard_normal((60, 1))
    coreg = Coregionalize(2, rank=1, active_dims=[Q], dtype=DT)
    m = _model(RBF(Q, active_dims=range(Q), dtype=DT) * coreg)
    losses = []

    class Rec(BatchInferenceLoop):
        def run(self, infr_executor, data, **kw):
            def wrapped(*a):
                out = infr_executor(*a)
                losses.append(float(out[0].detach()))
                return out
            return super(Rec, self).run(wrapped, data, **kw)
    infr = GradBasedInference(inference_algorithm=MAP(model=m, observed=[m.X, m.Y]), grad_loop=Rec(), dtype=DT)
    infr.run(X=_t(X), Y=_t(Y), max_iter=20, learning_rate=0.05)
    assert len(losses) >= 20 and all(np.isfinite(losses)) and losses[19] < losses[0], losses
    W, kappa = infr.params[coreg.W].detach().cpu().double().reshape(2, 1), infr.params[coreg.kappa].detach().cpu().double().reshape(2)
    B = W @ W.T + torch.diag(kappa)
    corr = float(B[0, 1] / torch.sqrt(B[0, 0] * B[1, 1]))
    print('learnt correlation', corr, 'losses', losses[0], losses[19])
    assert corr > 0, (corr, B)
