"""Host-side tests of the prediction at uncertain inputs (no GPU): mxf_psi_rbf_quad in the header, the binding and the built library; the op's
refusal of CPU tensors; the export of the algorithm; and the float64 restatement tests/_psi_predict_ref.py against the deterministic
prediction at s* = 0 and against a Gauss-Hermite average of the deterministic prediction at Q = 1."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _psi_ref as R
import _psi_predict_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def test_entry_point_is_declared_bound_and_exported():
    from mxfusion_amd import _lib
    name = 'mxf_psi_rbf_quad'
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert 'int ' + name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None
    decl = header[header.index('int ' + name + '('):].split(';')[0]
    assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1


def test_export_and_no_cpu_fallback():
    from mxfusion_amd import _lib, ops
    from mxfusion_amd.modules import gp_modules
    from mxfusion_amd.modules.gp_modules import BayesianGPLVMUncertainInputPrediction
    from mxfusion_amd.inference.inference_alg import SamplingAlgorithm
    assert gp_modules.BayesianGPLVMUncertainInputPrediction is BayesianGPLVMUncertainInputPrediction
    assert issubclass(BayesianGPLVMUncertainInputPrediction, SamplingAlgorithm)
    one = torch.ones(1, 3, 2, dtype=torch.float64)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.psi_rbf_quad(one, one, one, torch.ones(1, 1, dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64), False,
                         torch.ones(1, 2, 3, 3, dtype=torch.float64))


def _problem(Q, P, seed):
    """inducing points picked greedily as far apart as possible (the recipe of tests/test_gpu_bayesian_gplvm.py): near-duplicate rows of Kuu
    would put cond(Kuu) 2^-53, the reference's own rounding, next to the bars below"""
    rng = np.random.default_rng(seed)
    N, M, Nt = 30, 6, 9
    mu, s = t64(rng.uniform(-2, 2, (N, Q))), t64(rng.uniform(0.05, 0.8, (N, Q)))
    pick = [0]
    for _ in range(M - 1):
        pick.append(int(np.argmax(np.min(((mu.numpy()[:, None] - mu.numpy()[pick][None]) ** 2).sum(-1), 1))))
    Z = mu[pick].clone()
    Y = t64(np.sin(mu.numpy() @ rng.standard_normal((Q, P))) + 0.1 * rng.standard_normal((N, P)))
    ls, var, noise = t64(rng.uniform(0.8, 1.4, Q)), t64([1.3]), t64([0.3])
    Xt, st = t64(rng.uniform(-2.5, 2.5, (Nt, Q))), t64(rng.uniform(0.0, 0.6, (Nt, Q)))
    st[::4] = 0.0
    return (mu, s, Z, ls, var, noise, Y), Xt, st


@pytest.mark.parametrize('Q,P', [(1, 1), (2, 3)])
def test_zero_test_variance_is_the_deterministic_prediction(Q, P):
    """s* = 0: the moments are R.predict's, the variance the same in every output column; 1e-12"""
    fit, Xt, _ = _problem(Q, P, 3 + Q)
    m, v = PR.predict_uncertain(Xt, torch.zeros_like(Xt), *fit, jitter=1e-8)
    mr, vr = R.predict(Xt, *fit, jitter=1e-8)
    em, ev = float((m - mr).abs().max()), float((v - vr[:, None]).abs().max())
    print('mean', em, 'variance', ev)
    assert m.shape == v.shape == (Xt.shape[0], P) and em <= 1e-12 and ev <= 1e-12
    _, vn = PR.predict_uncertain(Xt, torch.zeros_like(Xt), *fit, jitter=1e-8, noise_free=False)
    assert float((vn - v - fit[5][0]).abs().max()) <= 1e-14


@pytest.mark.parametrize('P', [1, 3])
def test_against_a_gauss_hermite_average_of_the_deterministic_prediction(P):
    """Q = 1, s* in [0, 0.6] with exact zeros: the mean is E[m(x)] and the variance E[v(x) + m(x)^2] - E[m(x)]^2 of R.predict under a 120-node
    Gauss-Hermite rule; 1e-9"""
    fit, Xt, st = _problem(1, P, 11 + P)
    x, w = np.polynomial.hermite.hermgauss(120)
    x, w = t64(x), t64(w / np.sqrt(np.pi))
    nodes = Xt + torch.sqrt(2 * st) * x[None, :]                       # (Nt, 120)
    mr, vr = R.predict(nodes.reshape(-1, 1), *fit, jitter=1e-8)
    mr, vr = mr.reshape(Xt.shape[0], 120, P), vr.reshape(Xt.shape[0], 120, 1)
    mean = (w[None, :, None] * mr).sum(1)
    var = (w[None, :, None] * (vr + mr * mr)).sum(1) - mean * mean
    m, v = PR.predict_uncertain(Xt, st, *fit, jitter=1e-8)
    em, ev = float((m - mean).abs().max()), float((v - var).abs().max())
    print('mean', em, 'variance', ev)
    assert em <= 1e-9 and ev <= 1e-9
