"""Host checks of matrix-free exact GP regression: the restatement tests/_iterative_ref.py against the Cholesky closed form, the solver
pieces of components/distributions/gp/_iterative.py (plain torch, so they run on the CPU) against the restatement, the ABI, and the
refusals that need no GPU.

With the N + r draws sqrt(N + r) e_i the probes' outer products average to P exactly (1/T sum_i z_i z_i^T = noise I + L_r L_r^T), so
Hutchinson's trace and, at full Krylov convergence, the Lanczos quadrature are exact: value and gradients of the restatement must equal
log N(Y | 0, K + noise I) and its torch.linalg float64 autograd gradients.  At rank 0 these are the N probes sqrt(N) e_i.

Inputs: N = 48, Q = 2, P = 2, noise 0.1, RBF with ARD length-scales (1.3, 0.9), variance 1.2, x uniform on [-2, 2]^2; the spectrum of K decays
fast enough that every column reaches the relative residual 1e-13 within the cap of N iterations (asserted: a condition of the test).

Measured (float64, this file): largest error relative to an element's scale, over value, dls, dvar, dnoise, dY,
    rank 0: 1.7e-13 (dY; 5e-15 on the parameter gradients)        rank 8: 3.3e-14
The bar is 100 times the larger, 1.7e-11 (below the 1e-6 at which the restatement would be wrong)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _iterative_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_kmv', 'mxf_kmv_bwd')
N, Q, P, NOISE, LS, VAR = 48, 2, 2, 0.1, (1.3, 0.9), 1.2
BAR = 1.7e-11


def _data():
    rng = np.random.default_rng(48)
    X = rng.uniform(-2, 2, (N, Q))
    Y = np.sin(X @ rng.standard_normal((Q, P))) + 0.3 * rng.standard_normal((N, P))
    return X, Y


def _closed_form(X, Y):
    X, Y = torch.as_tensor(X), torch.as_tensor(Y)
    ls, var, noise = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (LS, VAR, NOISE))
    Yv = Y.clone().requires_grad_(True)
    d = (X[:, None, :] - X[None, :, :]) / ls
    K = var * torch.exp(-0.5 * (d * d).sum(-1)) + noise * torch.eye(N, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    a = torch.cholesky_solve(Yv, L)
    value = -0.5 * (Yv * a).sum() - P * torch.log(torch.diagonal(L)).sum() - 0.5 * N * P * np.log(2 * np.pi)
    g = torch.autograd.grad(value, [ls, var, noise, Yv])
    return dict(value=float(value.detach()), dls=g[0].numpy(), dvar=float(g[1]), dnoise=float(g[2]), dY=g[3].numpy())


@pytest.mark.parametrize('rank', [0, 8])
def test_restatement_is_the_cholesky_closed_form_on_exact_probes(rank):
    X, Y = _data()
    ref = _closed_form(X, Y)
    got = IR.logpdf('rbf', X, Y, NOISE, LS, VAR, IR.exact_probes(N, rank), rank, tol=1e-13, max_iter=N)
    assert got['rank'] == rank
    print('iterations', got['iterations'], 'worst residual', got['residual'])
    assert got['residual'] <= 1e-13 and max(got['iterations']) <= N, 'the inputs must converge within the cap'
    worst = 0.0
    for k in ('value', 'dls', 'dvar', 'dnoise', 'dY'):
        err = float(np.max(np.abs(np.asarray(got[k]) - np.asarray(ref[k])) / got['scale'][k]))
        print(k, 'error relative to its scale', err)
        worst = max(worst, err)
    print('worst', worst, 'bar', BAR)
    assert worst <= BAR


@pytest.mark.parametrize('rank', [0, 8])
def test_solver_pieces_are_the_restatement(rank):
    """_iterative.py on CPU float64 tensors with a dense product: the batched PCG, the pivoted Cholesky from a row oracle, the Woodbury
    preconditioner and the quadrature give the restatement's numbers (same recurrence, same probes: agreement to the
    CG tolerance of 1e-10 times the condition bound (N var + noise) / noise = 577, taken at 1e-7)"""
    from mxfusion_amd.components.distributions.gp import _iterative as it
    import _gram_ref as GR
    X, Y = _data()
    rng = np.random.default_rng(3)
    K = GR.gram_ref('rbf', X[None], None, np.array([LS]), np.array([[VAR]]))[0]
    Kt = torch.as_tensor(K)
    L = it.pivoted_cholesky(lambda i: Kt[i], torch.diagonal(Kt).clone(), rank)
    Lr = IR.pivoted_cholesky(K, rank)
    assert (L is None and rank == 0) or np.allclose(L.numpy(), Lr, rtol=1e-10, atol=1e-12)
    pre = it.Preconditioner(L, NOISE, N)
    solve, logdetP = IR.precond(Lr, NOISE, N)
    assert abs(pre.logdet - logdetP) <= 1e-10 * abs(logdetP)
    eps = rng.standard_normal((N + rank, 5))
    Z = pre.sample(torch.as_tensor(eps))
    Khat = Kt + NOISE * torch.eye(N, dtype=torch.float64)
    B = torch.cat([torch.as_tensor(Y), Z], 1)
    sol, iters, a, b = it.pcg(lambda V: Khat @ V, B, pre, tol=1e-10, max_iter=200, check_every=7)
    W = pre.solve(Z)
    logdet = it.slq_logdet(a[:, P:], b[:, P:], iters[P:], (Z * W).sum(0), pre.logdet)
    ref = IR.logpdf('rbf', X, Y, NOISE, LS, VAR, eps, rank, tol=1e-10, max_iter=200)
    assert max(abs(int(i) - r) for i, r in zip(iters, ref['iterations'])) <= 1          # a residual at the threshold may stop one iteration apart
    assert np.allclose(sol[:, :P].numpy(), ref['alpha'], rtol=1e-7, atol=1e-9)
    assert abs(logdet - ref['logdet']) <= 1e-7 * abs(ref['logdet'])
    resid = (Khat @ sol - B).norm(dim=0) / B.norm(dim=0)
    assert float(resid.max()) <= 2e-10


def test_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert 'int ' + name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert '#define MXF_KMV_MAX_Q %d' % _lib.KMV_MAX_Q in header and _lib.KMV_MAX_Q == 16


def test_ops_refuse_cpu_tensors():
    from mxfusion_amd import _lib, ops
    one = lambda *s: torch.ones(*s, dtype=torch.float64)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.kernel_matvec('rbf', one(1, 3, 2), None, one(1, 2), one(1, 1), True, one(1, 3, 4))
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.kernel_matvec_bwd_('rbf', one(1, 3, 2), None, one(1, 2), one(1, 1), True, one(1, 3, 4), one(1, 3, 4), None, one(1, 2), one(1, 1))


def test_unsupported_kernels_are_a_specification_error():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Linear, Bias, White
    from mxfusion_amd.modules.gp_modules import IterativeGPRegression
    for kern in (Linear(2), Bias(2), White(2), RBF(2) + Linear(2), RBF(2) * RBF(2), RBF(1, active_dims=[0])):
        m = Model()
        m.X = Variable(shape=(5, 2))
        m.noise_var = Variable(shape=(1,), initial_value=0.1)
        with pytest.raises(ModelSpecificationError, match='single stationary kernel'):
            IterativeGPRegression.define_variable(X=m.X, kernel=kern, noise_var=m.noise_var, shape=(5, 1))
        with pytest.raises(ModelSpecificationError, match='single stationary kernel'):
            kern.matvec(None, torch.ones(1, 5, 2), torch.ones(1, 5, 1))
