"""mxf_nearest, mxf_kmeans_step and mxfusion_amd/util/inducing.py on the GPU, in both dtypes, against the float64 restatement
tests/_kmeans_ref.py.

Sizes of csrc/nearest.hip that the shapes are chosen from: a wavefront is 64 rows, a workgroup NEAREST_RB = 128 rows, a thread one row; Q is
padded to 4, 8 or 16; M is never split; a step adds every row into M x QP double sums by atomics.  So N in {1, 127, 128, 129, 300} x M in
{1, 2, 17, 65} at Q = 3, Q in {1, 3, 4, 5, 8, 9, 16} at N = 129, M = 17, and N = 128 * 1024 + 1, M = 2, Q = 3 (1 025 workgroups onto two
accumulators).  Operands: standard normal times 2; the reference of a float32 run sees the float32-rounded operands.

Bars (derived, eps the dtype's epsilon): a squared distance is a sum of Q non-negative terms, each a rounded difference squared (3 roundings
apiece, relative to itself) summed with at most Q more, so rtol = 4 (Q + 2) eps on d2 and on the inertia, atol 0.  The assignment is checked by
property on every row: the float64 distance to the chosen centre is within (1 + 2 rtol) of the float64 minimum.  C_new is the double sum
of the assigned rows divided and rounded once: rtol 2^-23 (float32) / 1e-12 (float64) against the float64 means under the returned idx,
atol the same factor times max |X|.  On the integer lattice every distance is exact and idx must equal the reference bitwise."""
import functools

import numpy as np
import pytest
import torch

import _kmeans_ref as KR

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
IDS = ['f64', 'f32']
CASES = [(n, m, 3) for n in (1, 127, 128, 129, 300) for m in (1, 2, 17, 65)] + [(129, 17, q) for q in (1, 4, 5, 8, 9, 16)] + [(128 * 1024 + 1, 2, 3)]


def _eps(dtype):
    return float(torch.finfo(dtype).eps)


@functools.lru_cache(maxsize=None)
def _case(N, M, Q, rounded):
    """(X, C, idx, d2) in float64 numpy: the operands (as a float32 run sees them, if rounded) and the reference; computed once, never modified"""
    rng = np.random.default_rng(N * 1009 + M * 31 + Q)
    X, C = 2.0 * rng.standard_normal((N, Q)), 2.0 * rng.standard_normal((M, Q))
    if rounded:
        X, C = X.astype(np.float32).astype(np.float64), C.astype(np.float32).astype(np.float64)
    idx, d2 = KR.nearest(X, C)
    for a in (X, C, idx, d2):
        a.setflags(write=False)
    return X, C, idx, d2


def _dev(a, dtype):
    return torch.as_tensor(np.array(a)).to(dtype).cuda().contiguous()


def _check_assignment(X, C, idx, d2_ref, rtol):
    idx = idx.cpu().numpy().astype(np.int64)
    assert idx.min() >= 0 and idx.max() < C.shape[0]
    own = ((X - C[idx]) ** 2).sum(1)
    worst = float(np.max(own / np.where(d2_ref > 0, d2_ref, 1.0) - np.where(d2_ref > 0, 1.0, 0.0)))
    print('assignment: worst excess over the float64 minimum %.3g, bar %.3g' % (worst, 2 * rtol))
    assert np.all(own <= (1 + 2 * rtol) * d2_ref)
    return idx


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('N,M,Q', CASES, ids=['N%d-M%d-Q%d' % c for c in CASES])
def test_nearest_and_step(N, M, Q, dtype):
    from mxfusion_amd import ops
    X, C, _, d2_ref = _case(N, M, Q, dtype == torch.float32)
    rtol = 4 * (Q + 2) * _eps(dtype)
    Xd, Cd = _dev(X, dtype), _dev(C, dtype)
    idx, d2 = ops.nearest(Xd, Cd)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (N,) and d2.dtype == dtype and tuple(d2.shape) == (N,)
    err = np.abs(d2.double().cpu().numpy() - d2_ref)
    print('d2: worst relative error %.3g, bar %.3g' % (float(np.max(err / np.where(d2_ref > 0, d2_ref, 1.0))), rtol))
    assert np.all(err <= rtol * d2_ref)
    _check_assignment(X, C, idx, d2_ref, rtol)
    only, none = ops.nearest(Xd, Cd, want_d2=False)
    assert none is None and torch.equal(only, idx)

    C_new, idx2, counts, inertia = ops.kmeans_step(Xd, Cd)
    torch.cuda.synchronize()
    assert torch.equal(idx2, idx), 'the step assigns as mxf_nearest does'
    assert counts.dtype == torch.int64 and inertia.dtype == torch.float64 and inertia.dim() == 0 and C_new.dtype == dtype
    got_idx = idx2.cpu().numpy().astype(np.int64)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(got_idx, minlength=M))
    means, _ = KR.lloyd_step(X, C, got_idx)
    f = 2.0 ** -23 if dtype == torch.float32 else 1e-12
    cerr = np.abs(C_new.double().cpu().numpy() - means)
    print('C_new: worst error / bar %.3g' % float(np.max(cerr / (f * np.abs(means) + f * np.abs(X).max()))))
    assert np.all(cerr <= f * np.abs(means) + f * np.abs(X).max())
    empty = np.bincount(got_idx, minlength=M) == 0
    assert torch.equal(C_new[torch.as_tensor(empty).cuda()], Cd[torch.as_tensor(empty).cuda()]), 'an empty cluster keeps its centre bitwise'
    total = float(d2_ref.sum())
    print('inertia: relative error %.3g, bar %.3g' % (abs(float(inertia) - total) / total, rtol))
    assert abs(float(inertia) - total) <= rtol * total


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_ties_go_to_the_smallest_index(dtype):
    """the integer lattice: two centres duplicated, rows equidistant from distinct centres; every distance is exact in both dtypes"""
    from mxfusion_amd import ops
    X, C = KR.lattice()
    ref_idx, ref_d2 = KR.nearest(X, C)
    idx, d2 = ops.nearest(_dev(X, dtype), _dev(C, dtype))
    assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(d2.double().cpu().numpy(), ref_d2)
    C_new, idx2, counts, inertia = ops.kmeans_step(_dev(X, dtype), _dev(C, dtype))
    assert np.array_equal(idx2.cpu().numpy(), ref_idx) and float(inertia) == float(ref_d2.sum())
    assert counts[2] == 0 and counts[5] == 0 and torch.equal(C_new[2], _dev(C, dtype)[2])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_far_centre_is_empty_and_returned_bitwise(dtype):
    from mxfusion_amd import ops
    X, C, _, _ = _case(300, 17, 3, dtype == torch.float32)
    C = C.copy()
    C[4] = 1e6 + np.arange(3)
    Cd = _dev(C, dtype)
    C_new, idx, counts, _ = ops.kmeans_step(_dev(X, dtype), Cd)
    assert int(counts[4]) == 0 and int(counts.sum()) == 300 and torch.equal(C_new[4], Cd[4]) and not bool((idx == 4).any())


def _raw(name, Xt, Ct, **over):
    """the raw entry points with every pointer and size replaceable; returns the buffers"""
    from mxfusion_amd import _lib, ops
    N, Q, M = Xt.shape[0], Xt.shape[1], Ct.shape[0]
    b = dict(idx=torch.full((N,), -7, dtype=torch.int32).cuda(), d2=torch.full((N,), -7.0, dtype=Xt.dtype).cuda(),
             C_new=torch.full((M, Q), -7.0, dtype=Xt.dtype).cuda(), counts=torch.full((M,), -7, dtype=torch.int64).cuda(),
             inertia=torch.full((), -7.0, dtype=torch.float64).cuda())
    p = dict(X=Xt.data_ptr(), C=Ct.data_ptr(), N=N, M=M, Q=Q, **{k: v.data_ptr() for k, v in b.items()})
    p.update(over)
    try:
        if name == 'mxf_nearest':
            _lib.call(name, ops._h(Xt), ops._dt(Xt), p['N'], p['M'], p['Q'], p['X'], p['C'], p['idx'], p['d2'], ops._stream())
        else:
            _lib.call(name, ops._h(Xt), ops._dt(Xt), p['N'], p['M'], p['Q'], p['X'], p['C'], p['C_new'], p['idx'], p['counts'], p['inertia'], ops._stream())
    finally:
        torch.cuda.synchronize()
    return b


def test_status_codes_leave_the_buffers_alone():
    """Q = 17 is -3; a null required pointer, N = 0 and C_new == C are -2; nothing is written.  A step without idx and a nearest call without d2 run."""
    from mxfusion_amd import _lib
    X, C = torch.ones(5, 3, dtype=torch.float64).cuda(), torch.zeros(2, 3, dtype=torch.float64).cuda()
    X17, C17 = torch.ones(5, 17, dtype=torch.float64).cuda(), torch.zeros(2, 17, dtype=torch.float64).cuda()
    untouched = lambda b: all(float((v.double() + 7.0).abs().max()) == 0.0 for v in b.values())

    def refused(code, name, Xt, Ct, **over):
        guard = dict(idx=torch.full((Xt.shape[0],), -7, dtype=torch.int32).cuda())
        with pytest.raises(_lib.MXFError, match=r'\(%d\)' % code):
            _raw(name, Xt, Ct, **dict(dict(idx=guard['idx'].data_ptr()), **over))
        assert untouched(guard), 'the guard value in idx was written'
    for name in ('mxf_nearest', 'mxf_kmeans_step'):
        refused(-3, name, X17, C17)
        for over in (dict(X=None), dict(C=None), dict(N=0), dict(M=0), dict(Q=0)):
            refused(-2, name, X, C, **over)
    refused(-2, 'mxf_nearest', X, C, idx=None)
    for over in (dict(counts=None), dict(C_new=None), dict(inertia=None), dict(C_new=C.data_ptr())):
        refused(-2, 'mxf_kmeans_step', X, C, **over)
    assert float(C.abs().max()) == 0.0, 'C was written through the refused alias'
    # the same calls with nothing wrong run: five rows of ones, two coincident centres at the origin
    b = _raw('mxf_nearest', X, C, d2=None)
    assert b['idx'].tolist() == [0] * 5 and float((b['d2'] + 7.0).abs().max()) == 0.0
    b = _raw('mxf_kmeans_step', X, C, idx=None)
    assert b['counts'].tolist() == [5, 0] and float(b['inertia']) == 15.0 and b['C_new'].tolist() == [[1.0] * 3, [0.0] * 3]
    assert b['idx'].tolist() == [-7] * 5


def test_ops_validate_their_operands():
    from mxfusion_amd import ops
    X, C = torch.ones(5, 3).cuda(), torch.ones(2, 3).cuda()
    with pytest.raises(ValueError, match=r'X is \(N, Q\) and C \(M, Q\)'):
        ops.nearest(X, torch.ones(2, 4).cuda())
    with pytest.raises(ValueError, match='contiguous'):
        ops.kmeans_step(torch.ones(3, 5).cuda().t(), C)
    with pytest.raises(TypeError, match='dtype and device'):
        ops.nearest(X, C.double())
    with pytest.raises(ValueError, match='at least 1'):
        ops.nearest(X, torch.ones(0, 3).cuda())


# ---- util.inducing ---------------------------------------------------------------------------------------------------------------------
def _blobs():
    rng = np.random.default_rng(100)
    return np.concatenate([rng.standard_normal((200, 2)) + c for c in ((0, 0), (10, 0), (0, 10))])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_kmeans_finds_three_blobs(dtype):
    from mxfusion_amd.util.inducing import kmeans
    X = _blobs()
    Z, info = kmeans(_dev(X, dtype), 3)
    Z = Z.double().cpu().numpy()
    means = np.stack([X[i * 200:(i + 1) * 200].mean(0) for i in range(3)])
    dist = np.sqrt(((Z[:, None, :] - means[None]) ** 2).sum(-1))
    print('distance of each centre to the nearest blob mean', dist.min(1), 'inertia', info['inertia'])
    assert np.all(dist.min(1) <= 0.3) and sorted(dist.argmin(1).tolist()) == [0, 1, 2]
    slack = 1e-6 if dtype == torch.float32 else 1e-12
    ine = info['inertia']
    assert len(ine) == info['iterations'] and all(b <= a * (1 + slack) for a, b in zip(ine, ine[1:]))
    assert info['converged'] and info['iterations'] < 25 and int(info['counts'].sum()) == 600


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_kmeanspp_picks_the_reference_rows_on_the_lattice(dtype):
    from mxfusion_amd.util.inducing import kmeans, kmeanspp_rows
    X, _ = KR.lattice()
    for seed in (0, 1, 7):
        u = np.random.RandomState(seed).random_sample(6)
        rows = kmeanspp_rows(_dev(X, dtype), 6, seed=seed)
        assert rows.tolist() == KR.kmeanspp_rows(X, u).tolist(), seed
    Z, info = kmeans(_dev(X, dtype), 6, num_iter=0, seed=7)
    assert np.array_equal(Z.double().cpu().numpy(), X[KR.kmeanspp_rows(X, np.random.RandomState(7).random_sample(6))]) and info['iterations'] == 0
    with pytest.raises(ValueError, match='only 3 distinct rows, fewer than M = 4'):
        kmeans(_dev(np.repeat(X[:3], 4, 0), dtype), 4)
    Zr, _ = kmeans(_dev(X, dtype), 5, num_iter=0, init='random', seed=3)
    assert np.array_equal(Zr.double().cpu().numpy(), X[np.random.RandomState(3).permutation(49)[:5]])


def test_an_empty_cluster_is_reseeded_at_the_farthest_row():
    from mxfusion_amd.util.inducing import kmeans
    X = _blobs()
    init = np.array([[0.0, 0.0], [1e4, 1e4], [10.0, 0.0]])
    Z, info = kmeans(_dev(X, torch.float64), 3, num_iter=1, init=_dev(init, torch.float64))
    idx, d2 = KR.nearest(X, init)
    assert int(info['counts'][1]) == 0 and info['iterations'] == 1 and not info['converged']
    assert np.array_equal(Z[1].cpu().numpy(), X[int(np.argmax(d2))])
    means, _ = KR.lloyd_step(X, init, idx)
    assert np.allclose(Z[[0, 2]].cpu().numpy(), means[[0, 2]], rtol=1e-12, atol=1e-12 * np.abs(X).max())


def _greedy_inputs():
    X = np.random.default_rng(4).uniform(-2, 2, (150, 2))
    ls, var = np.array([1.3, 0.9]), 1.2
    d = (X[:, None, :] - X[None]) / ls
    return X, ls, var, var * np.exp(-0.5 * (d * d).sum(-1))


def test_greedy_variance_takes_the_reference_rows():
    """RBF with ARD on 150 points, M = 12, float64.  The first step is an exact tie of 150 identical prior variances (a stationary kernel),
    which both sides resolve to row 0; from the second step on the best and second-best conditional variances of the reference differ by
    more than 1e-6 relative (5.3e-5 at the closest step of these inputs), which rules out ties and near-ties."""
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.util.inducing import greedy_variance
    X, ls, var, K = _greedy_inputs()
    rows, gaps = KR.greedy_variance(K, 12)
    print('smallest gap after the first step', gaps[1:].min())
    assert rows[0] == 0 and gaps[0] == 0 and gaps[1:].min() > 1e-6
    Xd = _dev(X, torch.float64)
    Z, idx = greedy_variance(Xd, RBF(2, ARD=True), 12, rbf_lengthscale=_dev(ls, torch.float64), rbf_variance=_dev([var], torch.float64))
    assert idx.dtype == torch.int64 and idx.tolist() == rows.tolist() and torch.equal(Z, Xd[idx])
    with pytest.raises(ValueError, match='only 3 of the M = 5 rows'):
        greedy_variance(_dev(np.repeat(X[:3], 3, 0), torch.float64), RBF(2, ARD=True), 5, rbf_lengthscale=_dev(ls, torch.float64),
                        rbf_variance=_dev([var], torch.float64))


def _svgp(N, Q, M, sparse=True):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.inference import GradBasedInference, MAP
    from mxfusion_amd.modules.gp_modules import GPRegression, SVGPRegression
    m = Model()
    m.N = Variable()
    m.X = Variable(shape=(m.N, Q))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.05)
    kernel = RBF(input_dim=Q, ARD=True, variance=1.2, lengthscale=1.5, dtype='float64')
    if sparse:
        m.Y = SVGPRegression.define_variable(X=m.X, kernel=kernel, noise_var=m.noise_var, num_inducing=M, shape=(m.N, 1), dtype='float64')
        m.Y.factor.svgp_log_pdf.jitter = 1e-6
    else:
        m.Y = GPRegression.define_variable(X=m.X, kernel=kernel, noise_var=m.noise_var, shape=(m.N, 1), dtype='float64')
    return m, GradBasedInference(MAP(model=m, observed=[m.X, m.Y]), dtype='float64')


def test_initialize_inducing_inputs():
    from mxfusion_amd.util.inducing import initialize_inducing_inputs, kmeans
    N, Q, M = 300, 3, 17
    rng = np.random.default_rng(300)
    X = _dev(3.0 + 2.0 * rng.standard_normal((N, Q)), torch.float64)
    Y = torch.sin(X.sum(1, keepdim=True))
    m, infr = _svgp(N, Q, M)
    with pytest.raises(ValueError, match='not initialised'):
        initialize_inducing_inputs(infr, m.Y, X)
    infr.initialize(X=(N, Q), Y=(N, 1))
    Zvar = m.Y.factor.inducing_inputs
    got = initialize_inducing_inputs(infr, m.Y, X)
    Z, _ = kmeans(X, M)
    # two runs add their rows in a different order: sums of at most 300 doubles, 300 * 2^-53 relative to the largest |x|
    assert tuple(got.shape) == (M, Q) and torch.allclose(got, Z, rtol=0, atol=1e-12 * float(X.abs().max()))
    assert torch.equal(infr.params[Zvar], got)
    with pytest.raises(ValueError, match=r'X is \(N, 3\)'):
        initialize_inducing_inputs(infr, m.Y, X[:, :2].contiguous())
    with pytest.raises(ValueError, match="'kmeans' or 'greedy_variance'"):
        initialize_inducing_inputs(infr, m.Y, X, method='median')
    losses, loop = [], infr._grad_loop
    step0 = loop.step

    def step(*a, **k):
        loss = step0(*a, **k)
        losses.append(float(loss.detach()))
        return loss
    loop.step = step
    infr.run(X=X, Y=Y, max_iter=1, learning_rate=0.01)
    print('loss of the first step', losses)
    assert len(losses) == 1 and np.isfinite(losses[0])
    # the other method reads the kernel's current parameters from infr.params
    from mxfusion_amd.util.inducing import greedy_variance
    got = initialize_inducing_inputs(infr, m.Y, X, method='greedy_variance')
    kp = {n: infr.params[v] for n, v in m.Y.factor.kernel.parameters.items()}
    assert torch.equal(got, greedy_variance(X, m.Y.factor.kernel, M, **kp)[0])
    m2, infr2 = _svgp(N, Q, M, sparse=False)
    infr2.initialize(X=(N, Q), Y=(N, 1))
    with pytest.raises(ValueError, match='has no inducing_inputs'):
        initialize_inducing_inputs(infr2, m2.Y, X)
