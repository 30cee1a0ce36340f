"""Host-side tests of the psi statistics (no GPU): the float64 restatement tests/_psi_ref.py against a Gauss-Hermite tensor rule and against the
oracle's sparse-GP bound at s = 0; the element functions of mxfusion_amd/csrc/psi.h, built with the system C++ compiler, against the
restatement; the new entry points in the header, the binding and the built library."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _psi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_psi_rbf_fwd', 'mxf_psi_rbf_bwd')
t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def test_new_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert '#define MXF_PSI_MAX_Q %d' % _lib.PSI_MAX_Q in header and _lib.PSI_MAX_Q >= 16


def test_exports_and_no_cpu_fallback():
    from mxfusion_amd import _lib, ops
    from mxfusion_amd.modules import gp_modules
    from mxfusion_amd.modules.gp_modules import BayesianGPLVM
    assert gp_modules.BayesianGPLVM is BayesianGPLVM and BayesianGPLVM.row_additive is False
    one = torch.ones(1, 3, 2, dtype=torch.float64)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.psi_rbf(one, one, one, torch.ones(1, 1, dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64), False)


@pytest.mark.parametrize('Q', [1, 2])
def test_restatement_against_gauss_hermite(Q):
    """Psi1 and Psi2 of the restatement equal E[K(Z, x)] and sum_n E[K(Z, x_n) K(x_n, Z)] under an 80-node Gauss-Hermite tensor rule, s in
    [0.05, 1.5], to 1e-10"""
    rng = np.random.default_rng(Q)
    N, M = 7, 4
    mu, s, Z = t64(rng.uniform(-2, 2, (N, Q))), t64(rng.uniform(0.05, 1.5, (N, Q))), t64(rng.uniform(-2, 2, (M, Q)))
    ls, var = t64(rng.uniform(0.7, 1.5, Q)), t64([1.7])
    x, w = np.polynomial.hermite.hermgauss(80)
    x, w = t64(x), t64(w / np.sqrt(np.pi))
    P1, P2 = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, M, dtype=torch.float64)
    for n in range(N):
        axes = [mu[n, q] + torch.sqrt(2 * s[n, q]) * x for q in range(Q)]
        X = torch.stack(torch.meshgrid(*axes, indexing='ij'), -1).reshape(-1, Q)
        W = w if Q == 1 else (w[:, None] * w[None, :]).reshape(-1)
        K = R.rbf(Z, X, ls, var)
        P1[:, n] = (K * W).sum(-1)
        P2 += (K * W) @ K.T
    e1, e2 = float((R.psi1(mu, s, Z, ls, var) - P1).abs().max()), float((R.psi2(mu, s, Z, ls, var) - P2).abs().max())
    print('Psi1', e1, 'Psi2', e2)
    assert e1 <= 1e-10 and e2 <= 1e-10
    assert abs(float(R.psi0(mu, var)) - N * 1.7) <= 1e-14


@pytest.mark.parametrize('P', [1, 3])
def test_bound_at_zero_variance_is_the_oracles_sparse_gp(P):
    """s = 0: psi0, Psi1, Psi2 are sum Kdiag, Kuf, Kuf Kuf^T, and the restated bound is the oracle's sparse-GP log-pdf; rtol 1e-10"""
    from oracle import gp_oracle as O
    rng = np.random.default_rng(10 + P)
    N, M, Q = 30, 6, 2
    X, Z, Y = t64(rng.uniform(-2, 2, (N, Q))), t64(rng.uniform(-2, 2, (M, Q))), t64(rng.standard_normal((N, P)))
    ls, var, noise = t64([0.9, 1.3]), t64([1.4]), t64([0.2])
    got = R.bound(X, torch.zeros_like(X), Z, ls, var, noise, Y, jitter=1e-6)
    ref = O.sgp_log_pdf(O.RBF(Q, ARD=True), X[None], Y[None], Z[None], noise[None], {'rbf_lengthscale': ls[None], 'rbf_variance': var[None]}, jitter=1e-6)
    assert abs(float(got) - float(ref)) <= 1e-10 * abs(float(ref)), (float(got), float(ref))
    K = R.rbf(Z, X, ls, var)
    assert torch.allclose(R.psi1(X, torch.zeros_like(X), Z, ls, var), K, rtol=1e-13, atol=0)
    assert torch.allclose(R.psi2(X, torch.zeros_like(X), Z, ls, var), K @ K.T, rtol=1e-12, atol=0)


POINTS = [  # mu, s, z, z2, l, var
    (0.3, 0.4, -0.5, 0.9, 1.1, 1.3), (0.3, 0.0, -0.5, 0.9, 1.1, 1.3), (0.3, 1e-8, -0.5, 0.9, 1.1, 1.3), (0.3, 100.0, -0.5, 0.9, 1.1, 1.3),
    (-1.7, 0.05, 1.2, 1.2, 0.7, 0.8), (1.0, 1.5, 1.0, -1.0, 2.0, 2.5), (60.0, 0.3, -0.5, 0.9, 1.1, 1.3), (60.0, 0.0, 0.5, 0.5, 1.1, 1.3),
    (4.0, 0.0, -2.0, -1.0, 0.7, 1.0)]


def test_element_functions_against_the_restatement(tmp_path):
    """tests/host/psi_check.cpp prints the Psi1 and psi2n terms of psi.h and their partial derivatives in mu, s, z (z'), l and var at Q = 1 in
    both precisions, at s = 0, 1e-8 and 100 and at a row 55 lengthscales away (a finite zero); against autograd on the restatement at the
    argument each precision saw.  float64: 1e-12 relative or 1e-300 absolute; float32: 16 * 2^-24 relative (the exponent's rounding,
    |x| 2^-24 for |x| <= 16 here) or 1e-30 absolute; every value finite."""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path / 'psi_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'psi_check.cpp'),
                    '-o', exe, '-lm'], check=True)
    out = subprocess.run([exe], input='\n'.join(' '.join('%.17g' % v for v in r) for r in POINTS), capture_output=True, text=True, check=True).stdout
    got = np.array([[float(t) for t in line.split()] for line in out.strip().split('\n')])
    assert got.shape == (len(POINTS), 26) and np.isfinite(got).all()
    for row, pt in zip(got, POINTS):
        for cols, cast, rtol, atol in ((row[:13], np.float64, 1e-12, 1e-300), (row[13:], np.float32, 16 * 2.0 ** -24, 1e-30)):
            v = [torch.tensor([[float(cast(x))]], dtype=torch.float64, requires_grad=True) for x in pt[:4]]
            l, var = [torch.tensor([float(cast(x))], dtype=torch.float64, requires_grad=True) for x in pt[4:]]
            mu, s, z, z2 = v
            P1 = R.psi1(mu, s, z, l, var)[0, 0]
            P2 = R.psi2n(mu, s, torch.cat([z, z2]), l, var)[0, 0, 1]
            g1 = torch.autograd.grad(P1, [mu, s, z, l, var])
            g2 = torch.autograd.grad(P2, [mu, s, z, z2, l, var])
            ref = np.array([float(P1.detach())] + [float(g) for g in g1] + [float(P2.detach())] + [float(g) for g in g2])
            assert np.allclose(cols, ref, rtol=rtol, atol=atol), (pt, cast.__name__, cols, ref)
        if pt[0] == 60.0:
            assert (row == 0).all(), pt
