"""Host checks of the inducing-input initialisation: the restatement tests/_kmeans_ref.py against itself (brute force, torch.linalg), the
ABI of mxf_nearest / mxf_kmeans_step, the pure launch plan of csrc/nearest.hip (fused_plan.h: nearest_plan, printed by
tests/host/nearest_plan_check.cpp) against a numpy transcription, pivoted_cholesky's new return_pivots argument, and the refusal that needs
no GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _kmeans_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_nearest', 'mxf_kmeans_step')


# ---- the restatement against itself --------------------------------------------------------------------------------------------------------
def test_reference_nearest_is_brute_force():
    rng = np.random.default_rng(5)
    X, C = rng.standard_normal((50, 3)), rng.standard_normal((7, 3))
    idx, d2 = KR.nearest(X, C)
    for n in range(50):
        best, bi = np.inf, -1
        for m in range(7):
            d = sum((X[n, q] - C[m, q]) ** 2 for q in range(3))
            if d < best:
                best, bi = d, m
        assert idx[n] == bi and abs(d2[n] - best) <= 1e-15 * best
    Xl, Cl = KR.lattice()
    il, dl = KR.nearest(Xl, Cl)
    assert not np.any(il == 2) and not np.any(il == 5), 'a duplicated centre loses every tie to its first copy'
    D = ((Xl[:, None, :] - Cl[None, [0, 1, 3, 4, 6], :]) ** 2).sum(-1)
    assert int(((D == D.min(1, keepdims=True)).sum(1) > 1).sum()) >= 5, 'several rows are equidistant from two distinct centres'
    assert np.array_equal(dl, np.round(dl))
    C_new, counts = KR.lloyd_step(Xl, Cl, il)
    assert counts.sum() == 49 and counts[2] == 0 and np.array_equal(C_new[2], Cl[2]) and np.allclose(C_new[0], Xl[il == 0].mean(0))


def test_reference_greedy_variance_maximises_the_linalg_conditional_variance():
    rng = np.random.default_rng(9)
    X = torch.as_tensor(rng.uniform(-2, 2, (40, 2)))
    K = torch.exp(-0.5 * torch.cdist(X, X) ** 2) * 1.3
    rows, gaps = KR.greedy_variance(K.numpy(), 6)
    assert len(set(rows.tolist())) == 6 and rows[0] == 0 and gaps[0] == 0 and np.all(gaps[1:] > 0)      # (the first step: 40 equal prior variances)
    for k in range(6):
        S = torch.as_tensor(rows[:k])
        if k:
            A = torch.linalg.solve_triangular(torch.linalg.cholesky(K[S][:, S]), K[S], upper=False)
            v = torch.diagonal(K) - (A * A).sum(0)
        else:
            v = torch.diagonal(K).clone()
        v[S] = -1.0
        assert int(torch.argmax(v)) == rows[k]


def test_reference_kmeanspp_rows():
    X, _ = KR.lattice()
    u = np.random.RandomState(3).random_sample(6)
    rows = KR.kmeanspp_rows(X, u)
    assert rows[0] == int(u[0] * 49) and len(set(rows.tolist())) == 6
    with pytest.raises(ValueError, match='distinct'):
        KR.kmeanspp_rows(np.repeat(X[:3], 4, 0), np.random.RandomState(0).random_sample(4))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert 'int ' + name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert '#define MXF_NEAREST_MAX_Q %d' % _lib.NEAREST_MAX_Q in header and _lib.NEAREST_MAX_Q == 16


def test_ops_refuse_cpu_tensors():
    from mxfusion_amd import _lib, ops
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.nearest(torch.ones(5, 2, dtype=torch.float64), torch.ones(3, 2, dtype=torch.float64))
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.kmeans_step(torch.ones(5, 2), torch.ones(3, 2))


def test_pivoted_cholesky_with_pivots_is_the_same_factor():
    from mxfusion_amd.components.distributions.gp import _iterative as it
    rng = np.random.default_rng(2)
    X = torch.as_tensor(rng.uniform(-2, 2, (30, 2)))
    K = torch.exp(-0.5 * torch.cdist(X, X) ** 2)
    row, diag = (lambda i: K[i]), torch.diagonal(K).clone()
    for rank in (0, 1, 7, 30, 45):
        L = it.pivoted_cholesky(row, diag, rank)
        L2, piv = it.pivoted_cholesky(row, diag, rank, return_pivots=True)
        assert (L is None and L2 is None and piv.numel() == 0) or (torch.equal(L, L2) and piv.numel() == L.shape[1]), rank
        assert piv.dtype == torch.int64 and len(set(piv.tolist())) == piv.numel()
    _, piv = it.pivoted_cholesky(row, diag, 7, return_pivots=True)
    assert piv.tolist() == KR.greedy_variance(K.numpy(), 7)[0].tolist()
    # a rank-deficient matrix stops early, with as many pivots as columns
    Kd = torch.ones(5, 5, dtype=torch.float64)
    L, piv = it.pivoted_cholesky(lambda i: Kd[i], torch.diagonal(Kd).clone(), 3, return_pivots=True)
    assert L.shape == (5, 1) and piv.tolist() == [0] and torch.equal(L, it.pivoted_cholesky(lambda i: Kd[i], torch.diagonal(Kd).clone(), 3))


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
COLS_IN = 'esize step N M Q has_X has_C has_idx has_Cnew has_counts has_inertia alias'.split()
COLS_OUT = 'rc qp grid n_prep n_close at_cp at_zero at_sums at_counts at_inertia zero_bytes bytes'.split()
BASE = dict(esize=4, step=0, N=300, M=17, Q=3, has_X=1, has_C=1, has_idx=1, has_Cnew=1, has_counts=1, has_inertia=1, alias=0)


@pytest.fixture(scope='module')
def check(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('nearest_plan') / 'nearest_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'nearest_plan_check.cpp'), '-o', exe], check=True)
    return lambda text: subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout


def _line(req):
    return 'nearest ' + ' '.join(str(int(req[k])) for k in COLS_IN)


def _plan_ref(r):
    """numpy-free transcription of nearest_plan: the columns of COLS_OUT, zeros after the code of a refusal"""
    refused = lambda rc: [rc] + [0] * (len(COLS_OUT) - 1)
    if r['N'] < 1 or r['M'] < 1 or r['Q'] < 1:
        return refused(-2)
    if r['Q'] > 16:
        return refused(-3)
    if r['N'] > 2 ** 31 or r['M'] > 2 ** 31 - 1 or not r['has_X'] or not r['has_C']:
        return refused(-2)
    if r['step'] and (not r['has_Cnew'] or not r['has_counts'] or not r['has_inertia'] or r['alias']):
        return refused(-2)
    if not r['step'] and not r['has_idx']:
        return refused(-2)
    al = lambda b: (b + 255) // 256 * 256
    qp = 4 if r['Q'] <= 4 else (8 if r['Q'] <= 8 else 16)
    off = al(r['M'] * qp * r['esize'])
    at_zero = at_sums = at_counts = at_inertia = 0
    if r['step']:
        at_zero = at_sums = off
        off += al(r['M'] * qp * 8)
        at_counts = off
        off += al(r['M'] * 8)
        at_inertia = off
        off += al(8)
    return [0, qp, -(-r['N'] // 128), r['M'], r['M'] if r['step'] else 0, 0, at_zero, at_sums, at_counts, at_inertia, off - at_zero if r['step'] else 0, off]


def test_plan_columns_over_a_sweep(check):
    reqs = [dict(BASE, esize=e, step=s, N=N, M=M, Q=Q) for e in (4, 8) for s in (0, 1) for N in (1, 127, 128, 129, 300, 128 * 1024 + 1, 2 ** 31)
            for M in (1, 2, 17, 65, 1024, 2 ** 31 - 1) for Q in (1, 3, 4, 5, 8, 9, 16)]
    got = np.array(check('\n'.join(_line(r) for r in reqs)).split(), dtype=np.int64).reshape(len(reqs), len(COLS_OUT))
    want = np.array([_plan_ref(r) for r in reqs], dtype=np.int64)
    assert np.array_equal(got, want), reqs[int(np.nonzero((got != want).any(1))[0][0])]
    assert not got[:, 0].any()


def test_plan_grid_and_scratch(check):
    """the grid at N in {1, 128, 129, 2^31}: blocks of 128 rows; the scratch per QP: M QP elements, and M (QP + 1) + 1 doubles for a step,
    each piece in 256-byte granules"""
    for N, grid in ((1, 1), (128, 1), (129, 2), (2 ** 31, 2 ** 24)):
        out = check(_line(dict(BASE, N=N))).split()
        assert (int(out[0]), int(out[2])) == (0, grid), N
    for Q, qp in ((1, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16)):
        for esize in (4, 8):
            p = dict(zip(COLS_OUT, map(int, check(_line(dict(BASE, Q=Q, M=64, esize=esize))).split())))
            assert (p['qp'], p['bytes'], p['zero_bytes']) == (qp, 64 * qp * esize, 0)
            s = dict(zip(COLS_OUT, map(int, check(_line(dict(BASE, Q=Q, M=64, esize=esize, step=1))).split())))
            assert s['at_zero'] == s['at_sums'] == 64 * qp * esize and s['at_counts'] == s['at_sums'] + 64 * qp * 8
            assert s['at_inertia'] == s['at_counts'] + 64 * 8 and s['zero_bytes'] == 64 * qp * 8 + 64 * 8 + 256 == s['bytes'] - s['at_zero']


REFUSALS = [(dict(Q=17), -3, 'Q = 17 above the limit of 16 input dimensions'), (dict(Q=17, step=1, has_X=0), -3, 'Q = 17 above the limit of 16 input dimensions')]
REFUSALS += [(over, -2, 'N, M, Q >= 1') for over in (dict(N=0), dict(M=0), dict(Q=0), dict(N=-1, step=1), dict(Q=17, N=0))]
REFUSALS += [(over, -2, 'N <= 2^31, M <= 2^31 - 1') for over in (dict(N=2 ** 31 + 1), dict(M=2 ** 31), dict(M=2 ** 31, step=1))]
REFUSALS += [(dict(step=s, **{k: 0}), -2, 'null X or C') for s in (0, 1) for k in ('has_X', 'has_C')]
REFUSALS += [(dict(has_idx=0), -2, 'null idx')]
REFUSALS += [(dict(step=1, **{k: 0}), -2, 'null C_new, counts or inertia') for k in ('has_Cnew', 'has_counts', 'has_inertia')]
REFUSALS += [(dict(step=1, alias=1), -2, 'C_new must not alias C')]


@pytest.mark.parametrize('over,rc,why', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_plan_refusals(check, over, rc, why):
    line = check('text 1\n' + _line(dict(BASE, **over))).rstrip('\n')
    code, _, text = line.partition(' ')
    assert (int(code), text) == (rc, why)
    assert _plan_ref(dict(BASE, **over))[0] == rc


def test_plan_accepts_what_is_optional(check):
    """a step without idx, a nearest call without the step's buffers: not refusals"""
    assert check(_line(dict(BASE, step=1, has_idx=0))).split()[0] == '0'
    assert check(_line(dict(BASE, has_Cnew=0, has_counts=0, has_inertia=0, alias=1))).split()[0] == '0'
