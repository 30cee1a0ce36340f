"""The wide-input Gram passes through the public interface: Kernel.K and its autograd gradients under either setting of ops.WIDE_GRAM (bars of
test_gpu_gram_wide.py) and the exact-GP log-pdf at Q = 24 against the oracle (tolerances of test_wide_inputs_beyond_the_tiled_kernels)."""
import numpy as np
import pytest
import torch

import _gram_ref as G
from oracle import gp_oracle as O
from test_gpu_gram_wide import BAR, TOL_K, U

pytestmark = pytest.mark.gpu


@pytest.fixture
def switch():
    from mxfusion_amd import ops
    before = dict(ops.WIDE_GRAM)
    yield ops.WIDE_GRAM
    for dtype, on in before.items():
        ops.WIDE_GRAM[dtype] = on


@pytest.mark.parametrize('on', [True, False], ids=['wide', 'generic'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_rbf_k_and_its_gradients_under_either_switch(switch, dtype, on):
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    switch[dtype] = on
    Q = 24
    X, X2, ls, var, dK = G.make_case(5, 70, 45, Q, True, (False, False, False, False), S=1, f32=dtype == torch.float32)
    ls = (ls * np.sqrt(Q / 4.0)).astype(np.float32 if dtype == torch.float32 else np.float64).astype(np.float64)
    t = {n: torch.as_tensor(a).to(dtype).cuda().requires_grad_(True) for n, a in dict(dX=X, dX2=X2, dls=ls, dvar=var).items()}
    K = RBF(Q, ARD=True).K(None, t['dX'], t['dX2'], rbf_lengthscale=t['dls'], rbf_variance=t['dvar'])
    Kref = G.gram_ref('rbf', X, X2, ls, var, dtype=G.HI)
    assert float((np.abs(K.detach().cpu().numpy().astype(G.HI) - Kref) / (TOL_K[dtype] * (float(var.max()) + np.abs(Kref)))).max()) <= 1.0
    (K * torch.as_tensor(dK).to(dtype).cuda()).sum().backward()
    grad, scale = G.gram_bwd_ref('rbf', X, X2, ls, var, dK, dtype=G.HI)
    for name in t:
        worst = G.worst_ratio(t[name].grad.cpu().numpy().astype(G.HI), grad[name], scale[name], U[dtype])
        assert worst <= BAR[dtype], (name, worst)


def test_gp_regression_logpdf_at_24_inputs_against_the_oracle(switch):
    from mxfusion_amd import ops
    switch[torch.float64] = True
    rng = np.random.RandomState(4)
    N, Q, P = 40, 24, 2
    X, Y, noise, ls, var = rng.rand(1, N, Q), rng.randn(1, N, P), np.array([[0.1]]), rng.rand(1, Q) + 0.8, np.array([[1.1]])
    lv = {n: O.T(v).clone().requires_grad_(True) for n, v in dict(dX=X, dY=Y, dnoise=noise, dls=ls, dvar=var).items()}
    ref = O.gp_log_pdf(O.RBF(Q, ARD=True), lv['dX'], lv['dY'], lv['dnoise'], {'rbf_lengthscale': lv['dls'], 'rbf_variance': lv['dvar']})
    ref.sum().backward()
    d = lambda a: torch.as_tensor(a, dtype=torch.float64).cuda()
    r = ops.gp_logpdf('rbf', d(X), d(Y), d(noise), d(ls), d(var), True, want_grad=True)
    assert np.allclose(r['logL'].cpu().numpy(), ref.detach().numpy(), rtol=1e-9)
    for n in lv:
        assert np.allclose(r[n].cpu().numpy(), lv[n].grad.numpy(), rtol=1e-7, atol=1e-9 * float(lv[n].grad.abs().max())), n
