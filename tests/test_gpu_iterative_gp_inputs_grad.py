"""IterativeGPRegression's gradient in its inputs on the GPU (mxf_kmv_bwd_x under _IterativeLogPdfFn.backward) against torch autograd through a
dense float64 Cholesky log-pdf on the same data, under GradBasedInference's MAP objective: X a latent parameter, and X the output of a
5 -> 2 linear layer.  The probes are the exact ones of tests/test_gpu_iterative_gp.py (sqrt(N) e_i at rank 0: the trace is exact) at cg_tol
1e-13 and the bar is that file's for its other gradients, HOST_BAR, relative to the sum of the magnitudes of a gradient's terms:
_gram_ref.gram_bwd_ref's scale of dX for the cotangent |1/2 alpha alpha^T| + |P/2 Khat^-1|, times |x| for the layer's weight."""
import math

import numpy as np
import pytest
import torch

import _gram_ref as GR
import _iterative_ref as IR
from test_gpu_iterative_gp import Replay, HOST_BAR

pytestmark = pytest.mark.gpu

N, P = 40, 2


def _dense(kind, X, Y, noise, ls, var):
    """(-log N(Y | 0, K + noise I), alpha, Khat^-1) in torch; a clipped pair of the Matern kind carries no slope, as in the library"""
    d = (X[:, None, :] - X[None, :, :]) / ls
    r = math.sqrt(3.0) * torch.sqrt(torch.clamp((d * d).sum(-1), min=1e-14))
    K = var * (torch.exp(-0.5 * (d * d).sum(-1)) if kind == 'rbf' else (1.0 + r) * torch.exp(-r))
    L = torch.linalg.cholesky(K + noise * torch.eye(N, dtype=X.dtype, device=X.device))
    alpha = torch.cholesky_solve(Y, L)
    nll = 0.5 * (Y * alpha).sum() + P * torch.log(torch.diagonal(L)).sum() + 0.5 * N * P * math.log(2 * math.pi)
    return nll, alpha.detach(), torch.cholesky_inverse(L).detach()


def _setup(kind, Q, net):
    """(inference, its batch, the parameter whose gradient is checked, the exact dense objective as a function of it, the data X, the kernel)"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.functions import MXFusionTorchFunction
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Matern32
    from mxfusion_amd.inference import GradBasedInference, MAP
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression
    rng = np.random.default_rng(Q)
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).cuda()
    X = d(rng.uniform(-2, 2, (N, Q)))
    Y = d(np.sin(X.cpu().numpy() @ rng.standard_normal((Q, P))) + 0.3 * rng.standard_normal((N, P)))
    m = Model()
    m.X = Variable(shape=(N, Q))
    if net is not None:
        m.f = MXFusionTorchFunction(net, num_outputs=1, name='nn')
        m.Z = m.f(m.X)
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.5)
    kern = (RBF if kind == 'rbf' else Matern32)(Q if net is None else 2, ARD=True, dtype='float64')
    m.Y = IterativeGPRegression.define_variable(X=m.X if net is None else m.Z, kernel=kern, noise_var=m.noise_var, shape=(N, P), dtype='float64',
                                                num_probes=N, precond_rank=0, cg_tol=1e-13, max_cg_iter=4 * N,
                                                rand_gen=Replay([torch.as_tensor(IR.exact_probes(N)).cuda()] * 8))
    batch = dict(Y=Y) if net is None else dict(X=X, Y=Y)
    infr = GradBasedInference(MAP(model=m, observed=[getattr(m, k) for k in batch]), dtype='float64')
    infr.initialize(**{k: tuple(v.shape) for k, v in batch.items()})
    p = lambda v: infr.params[v].detach().double()
    if net is None:
        infr.params[m.X] = X
        leaf, inputs = m.X, lambda t: t.reshape(N, Q)
    else:
        leaf, bias = [v for _, v in sorted(m.Z.factor.parameters.items(), key=lambda kv: m.f.torch_name(kv[0]), reverse=True)]
        inputs = lambda W: X @ W.reshape(2, Q).T + p(bias).reshape(-1)
    exact = lambda t: _dense(kind, inputs(t), Y, p(m.noise_var).reshape(()), p(kern.lengthscale).reshape(-1), p(kern.variance).reshape(()))
    return infr, batch, leaf, exact, X, kern


@pytest.mark.parametrize('kind,Q,layer', [('rbf', 3, False), ('matern32', 3, False), ('rbf', 5, True)], ids=['rbf-latent', 'matern32-latent', 'rbf-net'])
def test_exact_probes_give_the_dense_gradient_and_map_steps_descend(kind, Q, layer):
    torch.manual_seed(0)
    infr, batch, leaf, exact, X, kern = _setup(kind, Q, torch.nn.Linear(5, 2).double() if layer else None)
    infr.params.zero_grad()
    infr.create_executor()(*batch.values())[1].backward()
    got = infr.params.grad(leaf).detach().double().cpu().numpy()
    t = infr.params[leaf].detach().double().clone().requires_grad_(True)
    before, alpha, Ki = exact(t)
    ref, = torch.autograd.grad(before, t)
    Z = (t.reshape(N, Q) if not layer else X @ t.reshape(2, Q).T).detach().cpu().numpy()         # the bias shifts every row alike: the same scale
    c = lambda v: infr.params[v].detach().double().cpu().numpy().reshape(1, -1)
    dK = (0.5 * (alpha @ alpha.T).abs() + 0.5 * P * Ki.abs()).cpu().numpy()
    scale = GR.gram_bwd_ref(kind, Z[None], None, c(kern.lengthscale), c(kern.variance), dK[None])[1]['dX'][0]
    scale = scale.T @ np.abs(X.cpu().numpy()) if layer else scale
    err = np.abs(got.reshape(scale.shape) - ref.cpu().numpy().reshape(scale.shape))
    ratio = float(np.max(err / (HOST_BAR * scale)))
    print('max error', float(err.max()), 'max scale', float(scale.max()), 'ratio to the bar', ratio)
    assert np.isfinite(got).all() and ratio <= 1.0
    if layer:           # five MAP steps lower the exact dense objective
        infr.run(learning_rate=0.05, max_iter=5, **batch)
        after = float(exact(infr.params[leaf].detach().double())[0])
        print('exact negative log-pdf before', float(before.detach()), 'after', after)
        assert np.isfinite(after) and after < float(before.detach())
