"""Host checks of nearest-neighbour (Vecchia) GP regression: the restatement tests/_vecchia_ref.py against itself (torch.distributions, a
triple loop), the ABI of mxf_knn / mxf_vecchia_*, the pure launch plans of csrc/knn.hip and csrc/vecchia.hip (fused_plan.h: knn_plan,
vecchia_plan, printed by tests/host/vecchia_plan_check.cpp) against a Python transcription, and the refusals that need no GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _vecchia_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_knn', 'mxf_vecchia_cond', 'mxf_vecchia_logpdf', 'mxf_vecchia_logpdf_bwd')


# ---- the restatement against itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', VR.KINDS)
def test_reference_with_all_predecessors_is_the_exact_log_pdf(kind):
    rng = np.random.default_rng(3)
    N, Q, P = 25, 2, 2
    X, Y = rng.uniform(-2, 2, (N, Q)), rng.standard_normal((N, P))
    ls, var, noise = np.array([0.8, 1.2]), 1.2, 0.05
    for k in (N - 1, N + 3):
        nbr, _ = VR.knn(X / ls, None, k, True)
        value = float(VR.terms(kind, X, Y, nbr, ls, var, noise).sum())
        Xs = torch.as_tensor(X / ls)
        K = VR.cov(kind, ((Xs[:, None, :] - Xs[None, :, :]) ** 2).sum(-1), torch.tensor(var, dtype=torch.float64)) + noise * torch.eye(N, dtype=torch.float64)
        mvn = torch.distributions.MultivariateNormal(torch.zeros(N, dtype=torch.float64), covariance_matrix=K)
        exact = float(mvn.log_prob(torch.as_tensor(Y).T).sum())
        assert abs(value - exact) <= 1e-12 * abs(exact), (kind, k, value, exact)


def test_reference_knn_is_a_triple_loop():
    rng = np.random.default_rng(5)
    X = np.round(rng.uniform(-2, 2, (40, 2)), 1)           # a coarse grid: exact ties occur
    C = X[:11] + 0.1
    for causal, Cc, k in ((True, None, 4), (False, C, 5), (False, C, 13)):
        idx, d2 = VR.knn(X, Cc, k, causal)
        cand = X if Cc is None else Cc
        for n in range(40):
            found = []
            for j in range(n if causal else cand.shape[0]):
                d = 0.0
                for q in range(2):
                    d += (X[n, q] - cand[j, q]) ** 2
                found.append((d, j))
            found.sort()
            want = found[:k] + [(np.inf, -1)] * (k - len(found[:k]))
            assert [j for _, j in want] == idx[n].tolist() and np.array_equal(np.array([d for d, _ in want]), d2[n]), n


def test_reference_cond_with_all_rows_is_the_gp_posterior():
    rng = np.random.default_rng(7)
    N, Q, P = 12, 3, 2
    X, Y, Xt = rng.uniform(-2, 2, (N, Q)), rng.standard_normal((N, P)), rng.uniform(-2, 2, (5, Q))
    ls, var, noise = np.array([0.9]), 1.2, 0.05
    nbr = np.tile(np.arange(N, dtype=np.int32), (5, 1))
    mu, v, _ = VR.cond('rbf', Xt, X, Y, nbr, ls, var, noise)
    K = var * np.exp(-0.5 * ((X[:, None] - X[None]) ** 2).sum(-1) / ls[0] ** 2) + noise * np.eye(N)
    Ks = var * np.exp(-0.5 * ((X[:, None] - Xt[None]) ** 2).sum(-1) / ls[0] ** 2)
    assert np.allclose(mu, Ks.T @ np.linalg.solve(K, Y), rtol=1e-11, atol=1e-13)
    assert np.allclose(v, var - (Ks * np.linalg.solve(K, Ks)).sum(0), rtol=1e-11, atol=1e-13)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert 'int ' + name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    for macro, value in (('MXF_KNN_MAX_Q', _lib.KNN_MAX_Q), ('MXF_KNN_MAX_K', _lib.KNN_MAX_K), ('MXF_VECCHIA_MAX_P', _lib.VECCHIA_MAX_P)):
        assert '#define %s %d' % (macro, value) in header
    assert (_lib.KNN_MAX_Q, _lib.KNN_MAX_K, _lib.VECCHIA_MAX_P) == (16, 32, 32)


def test_ops_refuse_cpu_tensors():
    from mxfusion_amd import _lib, ops
    X, Y, one = torch.ones(5, 2, dtype=torch.float64), torch.ones(5, 1, dtype=torch.float64), torch.ones(1, dtype=torch.float64)
    nbr = torch.full((5, 2), -1, dtype=torch.int32)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.knn(X, None, 2, causal=True)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.vecchia_cond('rbf', X, X, Y, nbr, one, one, one, False)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.vecchia_logpdf('rbf', X, Y, nbr, one, one, one, False)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.VecchiaLogPdf.apply('rbf', False, X, Y, nbr, one, one, one)


def test_module_refuses_what_the_kernels_do_not_cover():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Linear
    from mxfusion_amd.modules.gp_modules import VecchiaGPRegression
    m = Model()
    m.X = Variable(shape=(30, 3))
    m.noise_var = Variable(shape=(1,), initial_value=0.1)
    define = lambda kernel, **kw: VecchiaGPRegression.define_variable(X=m.X, kernel=kernel, noise_var=m.noise_var, shape=(30, 1), **kw)
    for kernel in (Linear(3), RBF(2, active_dims=[0, 1]), RBF(3) + RBF(3, name='rbf2'), RBF(17)):
        with pytest.raises(ModelSpecificationError, match='single stationary kernel'):
            define(kernel)
    for kw in (dict(num_neighbours=0), dict(num_neighbours=33), dict(ordering='maxmin')):
        with pytest.raises(ModelSpecificationError):
            define(RBF(3), **kw)
    assert define(RBF(3), num_neighbours=32, ordering='given').factor is not None


# ---- the plans -----------------------------------------------------------------------------------------------------------------------------
KNN_IN = 'esize N Nc Q k causal has_X has_C has_idx same'.split()
KNN_OUT = 'rc qp kp grid n_prep at_cp bytes'.split()
KNN_BASE = dict(esize=4, N=300, Nc=300, Q=3, k=9, causal=1, has_X=1, has_C=1, has_idx=1, same=1)
VEC_IN = 'esize call Nt N Q P k has_Xt has_X has_Y has_nbr has_ls has_var has_noise has_mean has_vout has_value has_g has_dY'.split()
VEC_OUT = 'rc qp rows grid n_acc at_acc zero_bytes bytes dy_bytes'.split()
VEC_BASE = dict(esize=4, call=1, Nt=70, N=300, Q=3, P=2, k=9, has_Xt=1, has_X=1, has_Y=1, has_nbr=1, has_ls=1, has_var=1, has_noise=1, has_mean=1,
                has_vout=1, has_value=1, has_g=1, has_dY=1)
COND, LOGPDF, BWD = 0, 1, 2


@pytest.fixture(scope='module')
def check(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('vecchia_plan') / 'vecchia_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'vecchia_plan_check.cpp'), '-o', exe], check=True)
    return lambda text: subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout


def _knn_line(r):
    return 'knn ' + ' '.join(str(int(r[c])) for c in KNN_IN)


def _vec_line(r):
    return 'vecchia ' + ' '.join(str(int(r[c])) for c in VEC_IN)


_al = lambda b: (b + 255) // 256 * 256
_qp = lambda Q: 4 if Q <= 4 else (8 if Q <= 8 else 16)


def _knn_ref(r):
    """transcription of knn_plan: the columns of KNN_OUT, zeros after the code of a refusal"""
    refused = lambda rc: [rc] + [0] * (len(KNN_OUT) - 1)
    if min(r['N'], r['Nc'], r['Q'], r['k']) < 1:
        return refused(-2)
    if r['Q'] > 16 or r['k'] > 32:
        return refused(-3)
    if r['N'] > 2 ** 31 or r['Nc'] > 2 ** 31 - 1 or not (r['has_X'] and r['has_C'] and r['has_idx']):
        return refused(-2)
    if r['causal'] and (not r['same'] or r['Nc'] != r['N']):
        return refused(-2)
    qp = _qp(r['Q'])
    return [0, qp, 8 if r['k'] <= 8 else (16 if r['k'] <= 16 else 32), -(-r['N'] // 128), r['Nc'], 0, _al(r['Nc'] * qp * r['esize'])]


def _vec_ref(r):
    """transcription of vecchia_plan"""
    refused = lambda rc: [rc] + [0] * (len(VEC_OUT) - 1)
    cond = r['call'] == COND
    if min(r['N'], r['Q'], r['P'], r['k']) < 1 or (cond and r['Nt'] < 1):
        return refused(-2)
    if r['Q'] > 16 or r['k'] > 32 or r['P'] > 32:
        return refused(-3)
    if r['N'] > 2 ** 31 - 1 or (cond and r['Nt'] > 2 ** 31 - 1):
        return refused(-2)
    if not all(r[c] for c in 'has_X has_Y has_nbr has_ls has_var has_noise'.split()):
        return refused(-2)
    if (cond and not (r['has_Xt'] and r['has_mean'] and r['has_vout'])) or (r['call'] == LOGPDF and not r['has_value']) or (r['call'] == BWD and not r['has_g']):
        return refused(-2)
    qp, rows = _qp(r['Q']), r['Nt'] if cond else r['N']
    n_acc = 0 if cond else (1 if r['call'] == LOGPDF else qp + 2)
    return [0, qp, rows, min(max(-(-rows // 2), 1), 4096), n_acc, 0, n_acc * 8, _al(n_acc * 8),
            r['N'] * r['P'] * r['esize'] if r['call'] == BWD and r['has_dY'] else 0]


def test_knn_plan_over_a_sweep(check):
    reqs = [dict(KNN_BASE, esize=e, N=N, Nc=N if c else Nc, Q=Q, k=k, causal=c, same=c) for e in (4, 8) for N in (1, 127, 128, 129, 65537, 2 ** 31 - 1)
            for Nc in (1, 7, 300) for Q in (1, 4, 5, 8, 9, 16) for k in (1, 8, 9, 16, 17, 32) for c in (0, 1)]
    got = np.array(check('\n'.join(_knn_line(r) for r in reqs)).split(), dtype=np.int64).reshape(len(reqs), len(KNN_OUT))
    want = np.array([_knn_ref(r) for r in reqs], dtype=np.int64)
    assert np.array_equal(got, want), reqs[int(np.nonzero((got != want).any(1))[0][0])]
    assert not got[:, 0].any()


def test_vecchia_plan_over_a_sweep(check):
    reqs = [dict(VEC_BASE, esize=e, call=call, Nt=Nt, N=N, Q=Q, P=P, k=k, has_dY=dy) for e in (4, 8) for call in (COND, LOGPDF, BWD)
            for Nt in (1, 70) for N in (1, 2, 3, 8191, 8192, 8193, 2 ** 31 - 1) for Q in (1, 4, 5, 16) for P in (1, 32) for k in (1, 32) for dy in (0, 1)]
    got = np.array(check('\n'.join(_vec_line(r) for r in reqs)).split(), dtype=np.int64).reshape(len(reqs), len(VEC_OUT))
    want = np.array([_vec_ref(r) for r in reqs], dtype=np.int64)
    assert np.array_equal(got, want), reqs[int(np.nonzero((got != want).any(1))[0][0])]
    assert not got[:, 0].any()
    grid = lambda **kw: int(check(_vec_line(dict(VEC_BASE, **kw))).split()[3])
    assert [grid(N=n) for n in (1, 2, 3, 4097, 8192, 8193, 10 ** 7)] == [1, 1, 2, 2049, 4096, 4096, 4096]
    assert grid(call=COND, Nt=5, N=10 ** 6) == 3


KNN_REFUSALS = [(dict(Q=17), -3, 'Q = 17 above the limit of 16 input dimensions'), (dict(k=33), -3, 'k = 33 above the limit of 32 neighbours'),
                (dict(Q=17, has_X=0), -3, 'Q = 17 above the limit of 16 input dimensions')]
KNN_REFUSALS += [(o, -2, 'N, Nc, Q, k >= 1') for o in (dict(N=0), dict(Nc=0), dict(Q=0), dict(k=0), dict(k=33, N=0), dict(N=-1))]
KNN_REFUSALS += [(o, -2, 'N <= 2^31, Nc <= 2^31 - 1') for o in (dict(N=2 ** 31 + 1, causal=0), dict(Nc=2 ** 31, causal=0), dict(N=2 ** 31, Nc=2 ** 31))]
KNN_REFUSALS += [({c: 0}, -2, 'null X, C or idx') for c in ('has_X', 'has_C', 'has_idx')]
KNN_REFUSALS += [(o, -2, 'a causal search takes C == X and Nc == N') for o in (dict(same=0), dict(Nc=299), dict(Nc=301))]


@pytest.mark.parametrize('over,rc,why', KNN_REFUSALS, ids=[str(i) for i in range(len(KNN_REFUSALS))])
def test_knn_plan_refusals(check, over, rc, why):
    line = check('text 1\n' + _knn_line(dict(KNN_BASE, **over))).rstrip('\n')
    code, _, text = line.partition(' ')
    assert (int(code), text) == (rc, why)
    assert _knn_ref(dict(KNN_BASE, **over))[0] == rc


VEC_REFUSALS = [(dict(Q=17), -3, 'Q = 17 above the limit of 16 input dimensions'), (dict(k=33), -3, 'k = 33 above the limit of 32 neighbours'),
                (dict(P=33), -3, 'P = 33 above the limit of 32 output columns'), (dict(P=33, has_Y=0, call=BWD), -3, 'P = 33 above the limit of 32 output columns')]
VEC_REFUSALS += [(o, -2, 'N, Nt, Q, P, k >= 1') for o in (dict(N=0), dict(Q=0), dict(P=0), dict(k=0), dict(call=COND, Nt=0), dict(call=BWD, N=-3), dict(Q=17, N=0))]
VEC_REFUSALS += [(o, -2, 'N, Nt <= 2^31 - 1') for o in (dict(N=2 ** 31), dict(call=COND, Nt=2 ** 31))]
VEC_REFUSALS += [(dict(call=call, **{c: 0}), -2, 'null X, Y, nbr, lengthscale, variance or noise') for call in (COND, LOGPDF, BWD)
                 for c in 'has_X has_Y has_nbr has_ls has_var has_noise'.split()]
VEC_REFUSALS += [(dict(call=COND, **{c: 0}), -2, 'null Xt, mean_out or var_out') for c in ('has_Xt', 'has_mean', 'has_vout')]
VEC_REFUSALS += [(dict(has_value=0), -2, 'null value_out'), (dict(call=BWD, has_g=0), -2, 'null g')]


@pytest.mark.parametrize('over,rc,why', VEC_REFUSALS, ids=[str(i) for i in range(len(VEC_REFUSALS))])
def test_vecchia_plan_refusals(check, over, rc, why):
    line = check('text 1\n' + _vec_line(dict(VEC_BASE, **over))).rstrip('\n')
    code, _, text = line.partition(' ')
    assert (int(code), text) == (rc, why)
    assert _vec_ref(dict(VEC_BASE, **over))[0] == rc


def test_plans_accept_what_is_optional(check):
    """Nt and the predictor's buffers do not matter to the other two calls; a reverse pass without dY zeroes nothing"""
    assert check(_vec_line(dict(VEC_BASE, Nt=0, has_Xt=0, has_mean=0, has_vout=0, has_g=0))).split()[0] == '0'
    assert check(_vec_line(dict(VEC_BASE, call=BWD, Nt=0, has_Xt=0, has_value=0, has_dY=0))).split() == ['0', '4', '300', '150', '6', '0', '48', '256', '0']
    assert check(_knn_line(dict(KNN_BASE, causal=0, same=0, Nc=7))).split()[0] == '0'
