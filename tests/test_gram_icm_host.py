"""Host checks of the multi-output (coregionalisation) support (no GPU): the ABI of mxf_gram_icm / mxf_gram_icm_bwd in the header, the
binding and the built library; the pure launch plan (csrc/gram_icm_plan.h, printed by tests/host/gram_icm_plan_check.cpp); the Coregionalize
kernel on CPU tensors against the float64 restatement tests/_coreg_ref.py; and that restatement tied to the one the project already trusts
(tests/_gram_ref.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _coreg_ref as R
import _gram_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_gram_icm', 'mxf_gram_icm_bwd')
t64 = R.t64


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert 'int ' + name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert '#define MXF_ICM_MAX_T %d' % _lib.ICM_MAX_T in header and _lib.ICM_MAX_T == 32
    plan = open(os.path.join(ROOT, 'mxfusion_amd', 'csrc', 'gram_icm_plan.h')).read()
    assert 'r.T > MXF_ICM_MAX_T' in plan and 'constexpr int MXF_ICM_MAX_Q = 16;' in plan


def test_ops_refuse_cpu_tensors():
    from mxfusion_amd import _lib, ops
    X, one = torch.ones(1, 5, 2, dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64)
    idx, B = torch.zeros(5, dtype=torch.int32), torch.ones(1, 2, 2, dtype=torch.float64)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.gram_icm('rbf', X, None, idx, None, one, one, False, B)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.gram_icm_bwd('rbf', X, None, idx, None, one, one, False, B, torch.ones(1, 5, 5, dtype=torch.float64))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
COLS = 'bwd esize kind S N N2 Q T ard square has_X has_idx has_idx2 has_ls has_var has_B has_K want_dB sls svar sB ldk'.split()
BASE = dict(bwd=0, esize=4, kind=0, S=1, N=300, N2=200, Q=3, T=3, ard=1, square=0, has_X=1, has_idx=1, has_idx2=1, has_ls=1, has_var=1, has_B=1, has_K=1,
            want_dB=1, sls=0, svar=0, sB=0, ldk=200)
SIZES = (1, 63, 64, 65, 257, 70000)
LDS_MAX = 112 * 1024          # MXF_ICM_LDS_MAX


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('gram_icm_plan') / 'gram_icm_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'gram_icm_plan_check.cpp'), '-o', exe], check=True)
    line = lambda r: ' '.join(str(int(r[c])) for c in COLS)
    return lambda reqs, text=False: subprocess.run([exe], input=('text 1\n' if text else '') + '\n'.join(line(r) for r in reqs), capture_output=True,
                                                   text=True, check=True).stdout.strip().split('\n')


def test_plan_owns_every_row_and_column(plan):
    """exactly once in the forward pass (every element of K is written by one lane), at least once -- here also exactly once -- in the
    reverse pass; the grid within HIP's limits; the LDS bytes what the layout adds up to and within the bound the plan states"""
    reqs = [dict(BASE, bwd=b, esize=e, kind=k, S=S, N=n, N2=n2, Q=q, T=T, ldk=n2, want_dB=w) for b in (0, 1) for e in (4, 8) for k, q, T in ((0, 16, 32), (1, 1, 1), (3, 8, 3))
            for S in (1, 3) for w in (0, 1) for n in SIZES for n2 in SIZES]
    up = lambda x: (x + 15) // 16 * 16
    for r, out in zip(reqs, plan(reqs)):
        rc, QT, rb, gx, gy, gz, lds, rmin, rmax, cmin, cmax, dbp = (int(t) for t in out.split())
        assert rc == 0, (r, out)
        if r['bwd']:
            assert rmin >= 1 and cmin >= 1 and (rmin, rmax, cmin, cmax) == (1, 1, 1, 1), (r, out)
        else:
            assert (rmin, rmax, cmin, cmax) == (1, 1, 1, 1) and rb == 64, (r, out)
        assert QT == r['Q'] and rb % 64 == 0 and rb >= 64 and (gy - 1) * rb < r['N'] <= gy * rb and (gx - 1) * 256 < r['N2'] <= gx * 256 and gz == r['S'], (r, out)
        assert gx <= 2 ** 31 - 1 and gy <= 65535 and gz <= 65535, (r, out)                   # HIP's grid limits
        e, T = r['esize'], r['T']
        want = up(64 * QT * e) + up(64 * 4) + up(T * T * e)
        if r['bwd']:
            assert rb * QT * e <= 16 * 1024, (r, out)
            want += up(rb * QT * e) + (up(T * 256 * e) + up(T * T * 8) if r['want_dB'] else 0) + 16 * 8
        assert dbp == (up(T * 256 * e) if r['bwd'] and r['want_dB'] else 0), (r, out)
        assert lds == want and lds <= LDS_MAX, (r, out, want)


def test_plan_of_a_square_gram_ignores_n2_and_idx2_and_pads_q(plan):
    outs = plan([dict(BASE, square=1, N=300, N2=0, has_idx2=0, ldk=300, Q=q) for q in (1, 2, 3, 4, 5, 8, 9, 16)])
    assert [int(o.split()[1]) for o in outs] == [1, 2, 4, 4, 8, 8, 16, 16] and all(o.split()[0] == '0' and o.split()[3] == '2' for o in outs)


NULLS = 'null X, index, parameter operand, B or matrix'
STRIDE = "a sample stride of lengthscale, variance or B that is neither 0 nor the operand's row"
REFUSALS = [(dict(T=0), -2, 'S, N, N2, Q, T >= 1'), (dict(T=33), -3, 'T above the limit of 32 outputs'), (dict(T=33, has_B=0), -3, 'T above the limit of 32 outputs'),
            (dict(Q=17), -3, 'Q above the limit of 16 input dimensions'), (dict(Q=17, has_X=0), -3, 'Q above the limit of 16 input dimensions'),
            (dict(kind=4), -2, 'stationary kinds only (RBF, Matern12, Matern32, Matern52)'), (dict(N=0), -2, 'S, N, N2, Q, T >= 1'),
            (dict(N2=0), -2, 'S, N, N2, Q, T >= 1'), (dict(S=0), -2, 'S, N, N2, Q, T >= 1'), (dict(Q=0), -2, 'S, N, N2, Q, T >= 1'),
            (dict(has_X=0), -2, NULLS), (dict(has_idx=0), -2, NULLS), (dict(has_idx2=0), -2, NULLS), (dict(has_ls=0), -2, NULLS), (dict(has_var=0), -2, NULLS),
            (dict(has_B=0), -2, NULLS), (dict(has_K=0), -2, NULLS), (dict(has_K=0, bwd=1), -2, NULLS),
            (dict(ldk=199), -2, 'negative sample stride or row stride below N2'), (dict(sls=2), -2, STRIDE), (dict(svar=2), -2, STRIDE), (dict(sB=8), -2, STRIDE),
            (dict(N=64 * 65536, bwd=0), -3, 'grid too large'), (dict(S=65536), -3, 'grid too large')]


@pytest.mark.parametrize('over,rc,why', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_plan_refusals(plan, over, rc, why):
    code, _, text = plan([dict(BASE, **over)], text=True)[0].partition(' ')
    assert (int(code), text) == (rc, why)


def test_plan_accepts_the_packed_parameter_strides(plan):
    assert all(o.split()[0] == '0' for o in plan([dict(BASE, S=2, sls=3, svar=1, sB=9), dict(BASE, S=2, ard=0, sls=1)]))


# ---- the restatement, anchored to the Gram restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_restatement_is_the_trusted_gram_times_the_gathered_b(kind):
    """B all ones: the plain Gram of _gram_ref.gram_ref; B = diag(kappa) on stacked data: block-diagonal K with kappa_t gram(X_t, X_t) blocks"""
    rng = np.random.RandomState(0)
    c = R.make_case(1, 40, 30, 3, 2, 3, True)
    n = lambda t: t.numpy()
    plain = t64(G.gram_ref(kind, n(c['X']), n(c['X2']), n(c['ls']), n(c['var'])))
    K = R.icm(kind, c['X'], c['X2'], c['idx'], c['idx2'], c['ls'], c['var'], torch.ones(1, 3, 3, dtype=torch.float64))
    assert float((K - plain).abs().max()) <= 1e-14
    K = R.icm(kind, c['X'], c['X2'], c['idx'], c['idx2'], c['ls'], c['var'], c['B'])
    want = plain * t64(n(c['B'])[:, c['idx'][:, None], c['idx2'][None, :]])
    assert float((K - want).abs().max()) <= 1e-14
    from mxfusion_amd.components.distributions.gp.kernels import Coregionalize
    Xs = [rng.uniform(-2, 2, (m, 3)) for m in (5, 7, 4)]
    X = t64(Coregionalize.stack(Xs))[None]
    kappa = t64([[0.5, 1.0, 1.5]])
    K = R.icm(kind, X[..., :3], None, X[0, :, 3].numpy().astype(np.int32), None, c['ls'], c['var'], R.coreg_matrix(kappa))[0]
    o = np.cumsum([0, 5, 7, 4])
    for a in range(3):
        for b in range(3):
            blk = K[o[a]:o[a + 1], o[b]:o[b + 1]]
            if a != b:
                assert float(blk.abs().max()) == 0.0
            else:
                assert float((blk - float(kappa[0, a]) * t64(G.gram_ref(kind, Xs[a][None], None, n(c['ls']), n(c['var']))[0])).abs().max()) <= 1e-14


# ---- Coregionalize on CPU tensors -----------------------------------------------------------------------------------------------------------
def test_coregionalize_k_and_kdiag_on_cpu():
    from mxfusion_amd.components.distributions.gp.kernels import Coregionalize
    rng = np.random.RandomState(1)
    T = 4
    X, X2 = t64(rng.randint(0, T, (9, 1)))[None], t64(rng.randint(0, T, (6, 1)))[None]
    W, kappa = t64(rng.randn(2, T, 2)), t64(rng.uniform(0.5, 1.5, (2, T)))
    k = Coregionalize(T, rank=2)
    B = R.coreg_matrix(kappa, W)
    i, j = X[0, :, 0].long(), X2[0, :, 0].long()
    K = k.K(None, X, X2, coreg_W=W, coreg_kappa=kappa)
    assert K.shape == (2, 9, 6) and float((K - R.gather(B, i, j)).abs().max()) <= 1e-12
    K = k.K(None, X, coreg_W=W, coreg_kappa=kappa)
    assert K.shape == (2, 9, 9) and float((K - R.gather(B, i)).abs().max()) <= 1e-12
    assert float((k.Kdiag(None, X, coreg_W=W, coreg_kappa=kappa) - torch.diagonal(K, dim1=-2, dim2=-1)).abs().max()) <= 1e-12
    # rank 0: B = diag(kappa), no W parameter at all
    k0 = Coregionalize(T, rank=0)
    assert k0.parameter_names == ['coreg_kappa'] and not hasattr(k0, 'W')
    K0 = k0.K(None, X, X2, coreg_kappa=kappa)
    assert float((K0 - R.gather(torch.diag_embed(kappa), i, j)).abs().max()) == 0.0
    # the index column carries no gradient; W and kappa do
    Xg, Wg = X.clone().requires_grad_(True), W.clone().requires_grad_(True)
    k.K(None, Xg, coreg_W=Wg, coreg_kappa=kappa).sum().backward()
    assert Xg.grad is None or float(Xg.grad.abs().max()) == 0.0
    assert float(Wg.grad.abs().max()) > 0


def test_coregionalize_parameters_defaults_and_replication():
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Coregionalize, MultiplyKernel
    k = RBF(2, ARD=True, active_dims=[0, 1]) * Coregionalize(3, rank=2, active_dims=[2])
    assert isinstance(k, MultiplyKernel) and k.parameter_names == ['mul_rbf_variance', 'mul_rbf_lengthscale', 'mul_coreg_W', 'mul_coreg_kappa']
    c = k.coreg
    assert c.input_dim == 1 and c.fused_spec() is None and not hasattr(c, '_kind')
    assert (tuple(c.W.shape), tuple(c.kappa.shape)) == ((3, 2), (3,))
    for T, rank in ((3, 2), (2, 1), (2, 2), (4, 3), (5, 5), (8, 4), (32, 6), (3, 5)):
        W0 = np.asarray(Coregionalize(T, rank=rank).W.initial_value)
        assert W0.shape == (T, rank) and len(set(np.round(np.abs(W0).ravel(), 12))) == T * rank, (T, rank)       # different in every entry, in magnitude too
        assert float(np.abs(W0).max()) <= 0.1 and float(np.abs(W0).min()) > 1e-4, (T, rank)                     # small, none at zero
        sv = np.linalg.svd(W0, compute_uv=False)
        assert np.linalg.matrix_rank(W0) == min(T, rank) and sv[min(T, rank) - 1] >= 0.1 * sv[0] / rank, (T, rank, sv)      # full column rank, with a margin
    assert np.array_equal(np.asarray(c.kappa.initial_value), np.ones(3))
    r = k.replicate_self()
    assert r.parameter_names == k.parameter_names and r.coreg is not c and (r.coreg.num_outputs, r.coreg.rank) == (3, 2)
    assert [v.uuid for v in r.parameters.values()] == [v.uuid for v in k.parameters.values()]
    two = Coregionalize(2) * Coregionalize(2)
    assert two.parameter_names == ['mul_coreg_W', 'mul_coreg_kappa', 'mul_coreg0_W', 'mul_coreg0_kappa']


def test_stack_builds_the_index_column():
    from mxfusion_amd.components.distributions.gp.kernels import Coregionalize
    Xs = [np.arange(6.0).reshape(3, 2), 10 + np.arange(4.0).reshape(2, 2)]
    Ys = [np.ones((3, 1)), 2 * np.ones((2, 1))]
    X, Y = Coregionalize.stack(Xs, Ys)
    assert X.shape == (5, 3) and np.array_equal(X[:, :2], np.concatenate(Xs)) and X[:, 2].tolist() == [0, 0, 0, 1, 1] and Y[:, 0].tolist() == [1, 1, 1, 2, 2]
    Xt = Coregionalize.stack([torch.as_tensor(x) for x in Xs])
    assert isinstance(Xt, torch.Tensor) and np.array_equal(Xt.numpy(), X)
    with pytest.raises(ValueError):
        Coregionalize.stack(Xs, Ys[:1])
    with pytest.raises(ValueError):
        Coregionalize.stack([Xs[0], np.zeros((2, 3))])


@pytest.mark.parametrize('bad', [2.5, -1.0, 3.0])
def test_a_bad_index_is_a_model_specification_error_naming_the_value(bad):
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import Coregionalize
    k = Coregionalize(3, rank=1)
    X = t64([[0.0], [2.0], [bad], [1.0]])[None]
    kw = dict(coreg_W=torch.zeros(1, 3, 1, dtype=torch.float64), coreg_kappa=torch.ones(1, 3, dtype=torch.float64))
    for call in (lambda: k.K(None, X, **kw), lambda: k.K(None, X[:, :2], X, **kw), lambda: k.Kdiag(None, X, **kw)):
        with pytest.raises(ModelSpecificationError, match=repr(bad).replace('.', r'\.')):
            call()
