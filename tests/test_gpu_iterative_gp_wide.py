"""IterativeGPRegression above 16 input dimensions (the tiled kernel product, mxf_kmv_wide / mxf_kmv_wide_bwd) against GPRegression on the
same data: RBF(24, ARD) and Matern52(40), N = 200, P = 2, float64.  The log-pdf and its gradients on the exact-trace probes
sqrt(N) e_i at rank 0 and cg_tol 1e-13, to tests/test_gpu_iterative_gp.py's bar for that comparison (1.7e-11 of the restatement's scales);
the predicted mean and variance at 50 test rows from a rank-8 preconditioner at cg_tol 1e-10, to that file's CG bound 10 kappa tol."""
import numpy as np
import pytest
import torch

import _iterative_ref as IR
import test_gpu_iterative_gp as T        # Replay, _value_and_grads, _compare: that file's own

pytestmark = pytest.mark.gpu

N, P, NT, NOISE, VAR = 200, 2, 50, 0.1, 1.1
KERNELS = {'rbf24-ard': ('rbf', 24, True), 'matern52-40': ('matern52', 40, False)}


def _data(q, ard):
    rng = np.random.default_rng(q)
    p = dict(X=rng.uniform(-2, 2, (N, q)), Xt=rng.uniform(-2.2, 2.2, (NT, q)), ls=rng.uniform(0.9, 1.4, q if ard else 1) * np.sqrt(q / 3.0))
    p['Y'] = np.sin(p['X'] @ rng.standard_normal((q, P)) / np.sqrt(q)) + 0.3 * rng.standard_normal((N, P))
    return p


def _model(cls, kind, ard, p, **kw):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Matern52
    from mxfusion_amd.util.inference import VariablesDict
    q = p['X'].shape[1]
    m = Model()
    m.X = Variable(shape=(N, q))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=NOISE)
    kern = RBF(q, ARD=ard, dtype='float64') if kind == 'rbf' else Matern52(q, ARD=ard, dtype='float64')
    m.Y = cls.define_variable(X=m.X, kernel=kern, noise_var=m.noise_var, shape=(N, P), dtype='float64', **kw)
    gp = m.Y.factor
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).cuda()[None]
    leaves = dict(Y=d(p['Y']).requires_grad_(True), noise=d([NOISE]).requires_grad_(True), ls=d(p['ls']).requires_grad_(True),
                  var=d([VAR]).requires_grad_(True))
    vs = VariablesDict({gp._module_graph.X.uuid: d(p['X']), m.noise_var.uuid: leaves['noise'], m.Y.uuid: leaves['Y']})
    for name, v in gp.kernel.parameters.items():
        vs[v.uuid] = leaves['ls' if name.endswith('lengthscale') else 'var']
    return gp, vs, leaves


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_log_pdf_and_gradients_are_gp_regression(name):
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression, GPRegression
    kind, q, ard = KERNELS[name]
    p = _data(q, ard)
    gp, vs, leaves = _model(IterativeGPRegression, kind, ard, p, num_probes=N, precond_rank=0, cg_tol=1e-13, max_cg_iter=4 * N,
                           rand_gen=T.Replay([torch.as_tensor(IR.exact_probes(N)).cuda()]))
    got = T._value_and_grads(gp.iterative_gp_log_pdf, vs, leaves)
    gp2, vs2, leaves2 = _model(GPRegression, kind, ard, p)
    ref = T._value_and_grads(gp2.gp_log_pdf, vs2, leaves2)
    scale = IR.logpdf(kind, p['X'], p['Y'], NOISE, p['ls'], VAR, IR.exact_probes(N), 0, tol=1e-13, max_iter=4 * N)['scale']
    T._compare(got, ref, scale, T.HOST_BAR, 0.0, name)


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_prediction_is_gp_regression(name):
    from mxfusion_amd.inference.inference_alg import SET_PARAMETER_PREFIX
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression, GPRegression
    kind, q, ard = KERNELS[name]
    p, tol, out = _data(q, ard), 1e-10, {}
    for cls, kw, log_pdf, predict in ((IterativeGPRegression, dict(cg_tol=tol, precond_rank=8), 'iterative_gp_log_pdf', 'iterative_gp_predict'),
                                      (GPRegression, {}, 'gp_log_pdf', 'gp_predict')):
        gp, vs, _ = _model(cls, kind, ard, p, **kw)
        with torch.no_grad():
            getattr(gp, log_pdf).compute(None, vs)
            for v in gp._extra_graphs[0].get_parameters():
                vs[v.uuid] = vs[SET_PARAMETER_PREFIX + v.uuid][1][None]
            vs[gp._module_graph.X.uuid] = torch.as_tensor(p['Xt']).cuda()[None]
            alg = getattr(gp, predict)
            alg.noise_free = False
            mu, var = alg.compute(None, vs)[gp._module_graph.Y.uuid]
        out[cls] = (mu.double().cpu().numpy(), var.double().cpu().numpy())
    (mu, var), (mu_ref, var_ref) = out[IterativeGPRegression], out[GPRegression]
    bar = 10 * (N * VAR + NOISE) / NOISE * tol
    e_mu, e_var = np.abs(mu - mu_ref).max() / np.abs(mu_ref).max(), np.abs(var - var_ref).max() / VAR
    print(name, 'mean error', e_mu, 'variance error', e_var, 'bar', bar)
    assert e_mu <= bar and e_var <= bar
