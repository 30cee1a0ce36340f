"""mxf_knn, mxf_vecchia_cond / _logpdf / _logpdf_bwd and VecchiaGPRegression on the GPU, in both dtypes, against the float64 restatement
tests/_vecchia_ref.py.

Sizes of the kernels that the shapes are chosen from.  knn.hip: a wavefront is 64 rows, a workgroup KNN_RB = 128 rows, a thread one row; Q is
padded to 4 / 8 / 16 and the register list to 8 / 16 / 32 slots; a causal scan ends at the wavefront's last row.  vecchia.hip: a group of 32
lanes owns a row, a workgroup VECCHIA_ROWS = 2 of them, at most 4096 workgroups that loop over further rows; a lane per column of the P + 1
right-hand sides (P = 32: lane 0 takes two).

The bars.  knn: a returned d2 is a sum of Q squares of rounded differences, each fma exact to one rounding: within 4 (Q + 2) eps relative
of the float64 distance of the returned index (test_gpu_kmeans' derivation), so slot t's true distance is within (1 + 2 rtol) of the
reference's slot t.  logpdf / bwd / cond, against the restatement on the REFERENCE's neighbour sets: the error of a row is the rounding
of the kernel values (eps relative) amplified by the conditioning of its tile, so per-row terms, the value and every gradient -- each
relative to its own magnitude plus the magnitude of its largest summand -- are held to C k cond_max eps, cond_max the largest cond_1(A_i)
of the case and eps the dtype's epsilon.  The form is derived; the constant is measured: over the logpdf / bwd cases below, on one
MI355X, the worst error / (k cond_max eps) was 6.37 (float64, N = 257, k = 1, where cond_max = 1 and the unit is one eps: the rounding of
the arithmetic itself, not an amplified one; 5.16 in float32 there; at most 1.31 at cond_max = 1.25 and at most 0.56, at N = 4097, wherever it is larger), and 0.084
over the cond cases.  C is the next power of two at or above four times the worst, 4 x 6.37 = 25.5: C = 32."""
import functools

import numpy as np
import pytest
import torch

import _kmeans_ref as KR
import _vecchia_ref as VR

pytestmark = pytest.mark.gpu

C_BAR = 32.0        # the module docstring has the measurement it comes from
DTYPES = [torch.float32, torch.float64]
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _round(a, dtype):
    """what the reference of a float32 run sees: the float32-rounded operand"""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if dtype == torch.float32 else a


# ---- knn -----------------------------------------------------------------------------------------------------------------------------------
def _check_knn(X, C, k, causal, dtype):
    from mxfusion_amd import ops
    X = _round(X, dtype)
    C = None if C is None else _round(C, dtype)
    N, Q = X.shape
    cand = X if C is None else C
    idx, d2 = ops.knn(_dev(X, dtype), None if C is None else _dev(C, dtype), k, causal=causal)
    only, none = ops.knn(_dev(X, dtype), None if C is None else _dev(C, dtype), k, causal=causal, want_d2=False)
    assert none is None and torch.equal(only, idx)
    idx, d2 = idx.cpu().numpy(), d2.double().cpu().numpy()
    assert idx.shape == d2.shape == (N, k) and idx.dtype == np.int32
    ref_idx, ref_d2 = VR.knn(X, C, k, causal)
    rtol = 4 * (Q + 2) * EPS[dtype]
    count = np.minimum(np.arange(N) if causal else np.full(N, cand.shape[0]), k)
    for n in range(N):
        m = count[n]
        got = idx[n, :m]
        assert np.all(idx[n, m:] == -1) and np.all(np.isposinf(d2[n, m:])), n
        assert np.all(got >= 0) and np.all(got < (n if causal else cand.shape[0])) and len(set(got.tolist())) == m, n
        assert np.all(np.diff(d2[n, :m]) >= 0), n
        true = ((X[n][None, :] - cand[got]) ** 2).sum(-1)
        assert np.all(np.abs(d2[n, :m] - true) <= rtol * true), n
        assert np.all(true <= ref_d2[n, :m] * (1 + 2 * rtol)) and np.all(true >= ref_d2[n, :m] * (1 - 2 * rtol)), n
    return idx, ref_idx


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 129, 1025])
def test_knn_causal_rows_and_list_sizes(N, dtype):
    rng = np.random.default_rng(N)
    X = rng.uniform(-2, 2, (N, 3))
    for k in (1, 3, 8, 9, 17, 32):
        _check_knn(X, None, k, True, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Nc', [1, 7, 300])
def test_knn_against_other_rows(Nc, dtype):
    rng = np.random.default_rng(Nc)
    C = rng.uniform(-2, 2, (Nc, 3))
    for N in (1, 65, 129):
        for k in (1, 9, 32):
            _check_knn(rng.uniform(-2, 2, (N, 3)), C, k, False, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Q', [1, 4, 5, 8, 9, 16])
def test_knn_input_dimensions(Q, dtype):
    rng = np.random.default_rng(Q)
    X = rng.uniform(-2, 2, (129, Q))
    _check_knn(X, None, 9, True, dtype)
    _check_knn(X, rng.uniform(-2, 2, (300, Q)), 9, False, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_knn_on_the_lattice_is_the_reference_bitwise(dtype):
    """every distance is exact, several rows have exact ties: the (d2, j) rule decides"""
    X, C = KR.lattice()
    ties = 0
    for Cc, causal, k in ((C, False, 5), (C, False, 7), (None, True, 9), (None, True, 32), (X, False, 17)):
        idx, ref = _check_knn(X, Cc, k, causal, dtype)
        assert np.array_equal(idx, ref), (causal, k)
        _, d2 = VR.knn(X, Cc, k, causal)
        ties += int(((d2[:, 1:] == d2[:, :-1]) & np.isfinite(d2[:, 1:])).sum())
    assert ties > 20


def _raw_knn(N, Nc, Q, k, causal, X, C, idx, d2):
    """mxf_knn on float32 buffers, any of them absent"""
    from mxfusion_amd import _lib, ops
    p = lambda t: None if t is None else t.data_ptr()
    rc = _lib.load().mxf_knn(ops._h(idx if X is None else X), 0, N, Nc, Q, k, causal, p(X), p(C), p(idx), p(d2), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_knn_status_codes_leave_the_buffers_alone():
    X = torch.rand(20, 17).cuda()
    idx = torch.full((20, 33), 77, dtype=torch.int32).cuda()
    d2 = torch.full((20, 33), 5.0).cuda()
    C = X.clone()
    assert _raw_knn(20, 20, 17, 3, 1, X, X, idx, d2) == -3
    assert _raw_knn(20, 20, 3, 33, 1, X, X, idx, d2) == -3
    assert _raw_knn(20, 20, 3, 3, 1, None, X, idx, d2) == -2
    assert _raw_knn(20, 20, 3, 3, 1, X, X, None, d2) == -2
    assert _raw_knn(0, 20, 3, 3, 0, X, C, idx, d2) == -2
    assert _raw_knn(20, 20, 3, 3, 1, X, C, idx, d2) == -2, 'causal with C != X'
    assert _raw_knn(20, 19, 3, 3, 1, X, X, idx, d2) == -2, 'causal with Nc != N'
    assert bool((idx == 77).all()) and bool((d2 == 5.0).all())
    assert _raw_knn(20, 20, 3, 3, 1, X, X, idx, None) == 0 and not bool((idx == 77).all())


# ---- logpdf / bwd / cond -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(N, k, Q, P, kind, ard, f32, holes=None):
    """operands (float32-rounded for a float32 run), the reference's neighbour sets and the restatement on them"""
    dtype = torch.float32 if f32 else torch.float64
    rng = np.random.default_rng(1000 * N + 10 * k + Q + P)
    X = rng.uniform(-2, 2, (N, Q))
    Y = np.sin(X.sum(1))[:, None] * np.ones((1, P)) + 0.1 * rng.standard_normal((N, P))
    ls = rng.uniform(0.7, 1.3, Q if ard else 1)
    X, Y, ls = [_round(a, dtype) for a in (X, Y, ls)]
    var, noise = float(_round(1.2, dtype)), float(_round(0.05, dtype))
    nbr, _ = VR.knn(X / ls, None, k, True)
    if holes == 'middle':                   # an empty slot between two neighbours, in every row that has three
        nbr = nbr.copy()
        nbr[3:, 1] = -1
    elif holes == 'all':
        nbr = np.full_like(nbr, -1)
    ref = VR.logpdf(kind, X, Y, nbr, ls, var, noise)
    return dict(X=X, Y=Y, ls=ls, var=var, noise=noise, nbr=nbr, ref=ref, kind=kind, ard=ard, k=k)


def _run(c, dtype, g=1.0, want=(True, True, True, True), want_terms=True):
    from mxfusion_amd import ops
    d = lambda a: _dev(np.atleast_1d(a), dtype)
    args = (c['kind'], d(c['X']), d(c['Y']), torch.as_tensor(c['nbr']).cuda(), d(c['ls']), d(c['var']), d(c['noise']), c['ard'])
    value, terms = ops.vecchia_logpdf(*args, want_terms=want_terms)
    grads = ops.vecchia_logpdf_bwd(*args, d(g), want=want)
    n = lambda t: None if t is None else t.double().cpu().numpy()
    dls, dvar, dnoise, dY = [n(t) for t in grads]
    return dict(value=float(value.cpu()), terms=n(terms), dls=dls, dvar=None if dvar is None else float(dvar[0]),
                dnoise=None if dnoise is None else float(dnoise[0]), dY=dY)


def _ratio(got, c, dtype, what):
    """worst error / (k cond_max eps) over the terms, the value and the gradients; prints each"""
    ref = c['ref']
    unit = c['k'] * ref['cond_max'] * EPS[dtype]
    worst = 0.0
    for key in ('terms', 'value', 'dls', 'dvar', 'dnoise', 'dY'):
        if got[key] is None:
            continue
        err, scale = np.abs(np.asarray(got[key]) - np.asarray(ref[key])), np.asarray(ref['scale'][key], dtype=np.float64)
        r = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale * unit, 1.0), np.where(err == 0, 0.0, np.inf))))      # a zero has no rounding
        assert np.isfinite(r), (what, key)
        worst = max(worst, r)
    print('%s: cond_max %.3g, worst error / (k cond_max eps) = %.3g' % (what, ref['cond_max'], worst))
    return worst


SHAPES = [(N, k, 3, 1, 'rbf', True) for N in (1, 2, 9, 33, 70, 257) for k in (1, 3, 8, 17, 32)]
SHAPES += [(70, 8, 3, P, 'rbf', True) for P in (3, 32)] + [(70, 8, Q, 1, 'rbf', True) for Q in (1, 16)]
SHAPES += [(70, 8, 3, 2, kind, ard) for kind in VR.KINDS for ard in (False, True)]
SHAPES += [(4097, 3, 3, 1, 'matern32', True)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES, ids=['-'.join(map(str, s)) for s in SHAPES])
def test_logpdf_and_gradients_are_the_restatement(shape, dtype):
    c = _case(*shape, dtype == torch.float32)
    assert _ratio(_run(c, dtype), c, dtype, str(shape)) <= C_BAR


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('holes', ['middle', 'all'])
def test_empty_slots_contribute_nothing(holes, dtype):
    c = _case(70, 8, 3, 2, 'rbf', True, dtype == torch.float32, holes)
    got = _run(c, dtype)
    assert _ratio(got, c, dtype, holes) <= C_BAR
    if holes == 'all':       # every row is its marginal
        a = c['var'] + c['noise']
        marg = -0.5 * 2 * np.log(2 * np.pi * a) - (c['Y'] ** 2).sum(1) / (2 * a)
        assert np.allclose(got['terms'], marg, rtol=16 * EPS[dtype], atol=0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_upstream_gradient_and_absent_outputs(dtype):
    """g scales every gradient; terms_out = NULL, each gradient pointer NULL in turn and dY = NULL run and leave the others equal (to the
    last bits: the sums are atomic)"""
    c = _case(70, 8, 3, 2, 'matern52', True, dtype == torch.float32)
    full = _run(c, dtype)
    scaled = _run(c, dtype, g=-2.5)
    tol = 64 * EPS[dtype]
    close = lambda a, b, s=1.0: np.allclose(np.asarray(a), s * np.asarray(b), rtol=tol, atol=tol * np.abs(np.asarray(b)).max())
    for key in ('dls', 'dvar', 'dnoise', 'dY'):
        assert close(scaled[key], full[key], -2.5), key
    assert _run(c, dtype, want_terms=False)['terms'] is None and close(_run(c, dtype, want_terms=False)['value'], full['value'])
    for drop in range(4):
        want = tuple(i != drop for i in range(4))
        part = _run(c, dtype, want=want)
        for i, key in enumerate(('dls', 'dvar', 'dnoise', 'dY')):
            assert (part[key] is None) if i == drop else close(part[key], full[key]), (drop, key)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', VR.KINDS)
def test_cond_is_the_restatement(kind, dtype):
    from mxfusion_amd import ops
    c = _case(70, 8, 3, 2, kind, True, dtype == torch.float32)
    rng = np.random.default_rng(11)
    for Nt, k in ((1, 8), (7, 3), (130, 17), (65, 32)):
        Xt = _round(rng.uniform(-2.2, 2.2, (Nt, 3)), dtype)
        nbr, _ = VR.knn(Xt / c['ls'], c['X'] / c['ls'], k, False)
        if k == 3:
            nbr[:, 1] = -1
        mu_ref, v_ref, cmax = VR.cond(kind, Xt, c['X'], c['Y'], nbr, c['ls'], c['var'], c['noise'])
        d = lambda a: _dev(np.atleast_1d(a), dtype)
        mu, v = ops.vecchia_cond(kind, d(Xt), d(c['X']), d(c['Y']), torch.as_tensor(nbr).cuda(), d(c['ls']), d(c['var']), d(c['noise']), True)
        unit = k * cmax * EPS[dtype]
        e_mu = np.abs(mu.double().cpu().numpy() - mu_ref).max() / ((np.abs(mu_ref).max() + np.abs(c['Y']).max()) * unit)
        e_v = np.abs(v.double().cpu().numpy() - v_ref).max() / (c['var'] * unit)
        print('cond %s Nt %d k %d: cond_max %.3g, error / (k cond_max eps): mean %.3g variance %.3g' % (kind, Nt, k, cmax, e_mu, e_v))
        assert mu.shape == (Nt, 2) and v.shape == (Nt,) and max(e_mu, e_v) <= C_BAR


def test_vecchia_status_codes_leave_the_buffers_alone():
    from mxfusion_amd import _lib, ops
    X, Y = torch.rand(20, 17, dtype=torch.float64).cuda(), torch.rand(20, 33, dtype=torch.float64).cuda()
    nbr = torch.full((20, 33), -1, dtype=torch.int32).cuda()
    one = torch.ones(17, dtype=torch.float64).cuda()
    out = torch.full((20 * 33,), 7.0, dtype=torch.float64).cuda()
    p, st, h, lib = (lambda t: None if t is None else t.data_ptr()), torch.cuda.current_stream().cuda_stream, ops._h(X), _lib.load()
    logpdf = lambda Q, P, k, X_=X, N=20: lib.mxf_vecchia_logpdf(h, 0, 1, N, Q, P, k, 1, p(X_), p(Y), p(nbr), p(one), p(one), p(one), p(out), p(out), st)
    bwd = lambda Q, P, k, g=one: lib.mxf_vecchia_logpdf_bwd(h, 0, 1, 20, Q, P, k, 1, p(X), p(Y), p(nbr), p(one), p(one), p(one), p(g), p(out), p(out), p(out), p(out), st)
    cond = lambda Q, P, k, m=out: lib.mxf_vecchia_cond(h, 0, 1, 20, 20, Q, P, k, 1, p(X), p(X), p(Y), p(nbr), p(one), p(one), p(one), p(m), p(out), st)
    for f in (logpdf, bwd, cond):
        assert (f(17, 1, 3), f(3, 33, 3), f(3, 1, 33)) == (-3, -3, -3)
    assert (logpdf(3, 1, 3, None), logpdf(3, 1, 3, X, 0), bwd(3, 1, 3, None), cond(3, 1, 3, None)) == (-2, -2, -2, -2)
    assert lib.mxf_vecchia_logpdf(h, 4, 1, 20, 3, 1, 3, 1, p(X), p(Y), p(nbr), p(one), p(one), p(one), p(out), p(out), st) == -2, 'a linear kernel'
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the exactness anchor: the dense path ---------------------------------------------------------------------------------------------------
def _model(cls, p, **kw):
    """(module, runtime variables with the sample axis, leaves) in float64: tests/test_gpu_iterative_gp.py's harness"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.util.inference import VariablesDict
    n, q = p['X'].shape
    m = Model()
    m.X = Variable(shape=(n, q))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    m.Y = cls.define_variable(X=m.X, kernel=RBF(q, ARD=True, dtype='float64'), noise_var=m.noise_var, shape=p['Y'].shape, dtype='float64', **kw)
    gp = m.Y.factor
    d = lambda a: torch.as_tensor(np.atleast_1d(a), dtype=torch.float64).cuda()[None]
    leaves = dict(Y=d(p['Y']).requires_grad_(True), noise=d(p['noise']).requires_grad_(True), ls=d(p['ls']).requires_grad_(True),
                  var=d(p['var']).requires_grad_(True))
    vs = VariablesDict({gp._module_graph.X.uuid: d(p['X']), m.noise_var.uuid: leaves['noise'], m.Y.uuid: leaves['Y']})
    for name, v in gp.kernel.parameters.items():
        vs[v.uuid] = leaves['ls' if name.endswith('lengthscale') else 'var']
    leaves['noise_uuid'] = m.noise_var.uuid
    return gp, vs, leaves


def _value_and_grads(alg, vs, leaves):
    logL = alg.compute(None, vs)
    assert tuple(logL.shape) == (1,)
    g = torch.autograd.grad(logL.sum(), [leaves[k] for k in ('ls', 'var', 'noise', 'Y')])
    c = lambda t: t.detach().double().cpu().numpy()
    return dict(value=float(logL.detach().double().cpu()[0]), dls=c(g[0])[0], dvar=float(c(g[1])[0, 0]), dnoise=float(c(g[2])[0, 0]), dY=c(g[3])[0])


def _predict(gp, vs, log_pdf, predict, Xt, mean=None):
    """{noise_free: (mean, variance)} at Xt from the posterior that the log-pdf persists"""
    from mxfusion_amd.inference.inference_alg import SET_PARAMETER_PREFIX
    out = {}
    with torch.no_grad():
        getattr(gp, log_pdf).compute(None, vs)
        for v in gp._extra_graphs[0].get_parameters():
            vs[v.uuid] = vs[SET_PARAMETER_PREFIX + v.uuid][1][None]
        vs[gp._module_graph.X.uuid] = torch.as_tensor(Xt).cuda()[None]
        if mean is not None:
            vs[mean[0].uuid] = torch.full((1, Xt.shape[0], 1), mean[1], dtype=torch.float64).cuda()
        alg = getattr(gp, predict)
        for noise_free in (False, True):
            alg.noise_free = noise_free
            mu, var = alg.compute(None, vs)[gp._module_graph.Y.uuid]
            out[noise_free] = (mu.double().cpu().numpy()[0], var.double().cpu().numpy()[0])
    return out


def test_all_predecessors_give_gp_regression():
    """N = 30, k = 32, ordering='given': value and gradients equal the dense path (mxf_gp_logpdf through GPRegression) to 1e-10 relative, and
    the predictor with all 30 rows as neighbours equals GPRegression's prediction"""
    from mxfusion_amd.modules.gp_modules import VecchiaGPRegression, GPRegression
    c = _case(30, 32, 3, 2, 'rbf', True, False)
    p = dict(X=c['X'], Y=c['Y'], ls=c['ls'], var=c['var'], noise=c['noise'])
    gp, vs, leaves = _model(VecchiaGPRegression, p, num_neighbours=32, ordering='given')
    got = _value_and_grads(gp.vecchia_gp_log_pdf, vs, leaves)
    gp2, vs2, leaves2 = _model(GPRegression, p)
    ref = _value_and_grads(gp2.gp_log_pdf, vs2, leaves2)
    for key in ('value', 'dls', 'dvar', 'dnoise', 'dY'):
        err = np.abs(np.asarray(got[key]) - np.asarray(ref[key])).max() / np.abs(np.asarray(ref[key])).max()
        print('dense anchor', key, 'relative error', err)
        assert err <= 1e-10, key
    Xt = np.random.default_rng(2).uniform(-2.2, 2.2, (40, 3))
    mu, v = _predict(gp, vs, 'vecchia_gp_log_pdf', 'vecchia_gp_predict', Xt)[False]
    mu_ref, v_ref = _predict(gp2, vs2, 'gp_log_pdf', 'gp_predict', Xt)[False]
    e_mu, e_v = np.abs(mu - mu_ref).max() / np.abs(mu_ref).max(), np.abs(v - v_ref).max() / np.abs(v_ref).max()
    print('dense anchor prediction: mean', e_mu, 'variance', e_v)
    assert mu.shape == mu_ref.shape == (40, 2) and v.shape == v_ref.shape == (40,) and e_mu <= 1e-10 and e_v <= 1e-10


# ---- the module ----------------------------------------------------------------------------------------------------------------------------
N_MOD, K_MOD = 300, 10


@functools.lru_cache(maxsize=None)
def _module_data():
    rng = np.random.default_rng(42)
    X = rng.uniform(-2, 2, (N_MOD, 2))
    return dict(X=X, Y=np.sin(X.sum(1))[:, None] + 0.1 * rng.standard_normal((N_MOD, 1)), ls=np.array([0.8, 1.2]), var=1.2, noise=0.05)


def _bar(ref, k):
    return C_BAR * k * ref['cond_max'] * EPS[torch.float64]


def test_module_log_pdf_and_prediction_are_the_restatement_on_its_own_ordering():
    from mxfusion_amd.modules.gp_modules import VecchiaGPRegression
    p = _module_data()
    gp, vs, leaves = _model(VecchiaGPRegression, p, num_neighbours=K_MOD, seed=3)
    got = _value_and_grads(gp.vecchia_gp_log_pdf, vs, leaves)
    perm = gp.vecchia_gp_log_pdf.permutation(N_MOD, 'cpu').numpy()
    assert sorted(perm.tolist()) == list(range(N_MOD)) and not np.array_equal(perm, np.arange(N_MOD))
    Xo, Yo = p['X'][perm], p['Y'][perm]
    nbr, _ = VR.knn(Xo / p['ls'], None, K_MOD, True)
    ref = VR.logpdf('rbf', Xo, Yo, nbr, p['ls'], p['var'], p['noise'])
    ref['dY'] = ref['dY'][np.argsort(perm)]
    ref['scale']['dY'] = ref['scale']['dY'][np.argsort(perm)]
    for key in ('value', 'dls', 'dvar', 'dnoise', 'dY'):
        r = float(np.max(np.abs(np.asarray(got[key]) - np.asarray(ref[key])) / np.asarray(ref['scale'][key]))) / _bar(ref, K_MOD)
        print('module', key, 'error / bar', r)
        assert r <= 1.0, key
    Xt = np.random.default_rng(1).uniform(-2.2, 2.2, (70, 2))
    gp.vecchia_gp_predict.chunk_rows = 33                 # three chunks
    pred = _predict(gp, vs, 'vecchia_gp_log_pdf', 'vecchia_gp_predict', Xt)
    (mu, v), (mu0, v0) = pred[False], pred[True]
    nbt, _ = VR.knn(Xt / p['ls'], Xo / p['ls'], K_MOD, False)
    mu_ref, v_ref, cmax = VR.cond('rbf', Xt, Xo, Yo, nbt, p['ls'], p['var'], p['noise'])
    unit = C_BAR * K_MOD * cmax * EPS[torch.float64]
    assert np.abs(mu - mu_ref).max() <= unit * (np.abs(mu_ref).max() + np.abs(Yo).max()) and np.abs(v - (v_ref + p['noise'])).max() <= unit * p['var']
    assert np.array_equal(mu0, mu) and np.allclose(v0 + p['noise'], v, rtol=1e-14)


def test_module_orderings_and_the_neighbour_cache():
    from mxfusion_amd.modules.gp_modules import VecchiaGPRegression
    p = _module_data()
    value = {}
    for ordering in ('given', 'random'):
        for k in (K_MOD, 32):
            q = p if k == K_MOD else {key: (v[:30] if key in ('X', 'Y') else v) for key, v in p.items()}       # k >= N - 1 at N = 30
            gp, vs, _ = _model(VecchiaGPRegression, q, num_neighbours=k, ordering=ordering)
            with torch.no_grad():
                value[ordering, k] = float(gp.vecchia_gp_log_pdf.compute(None, vs)[0])
    print(value)
    assert abs(value['given', K_MOD] - value['random', K_MOD]) > 1e-6 * abs(value['given', K_MOD])
    assert abs(value['given', 32] - value['random', 32]) <= 1e-10 * abs(value['given', 32])
    # the cache: the same sets while only the parameters move; new ones after refresh_neighbours() or for another X
    gp, vs, leaves = _model(VecchiaGPRegression, p, num_neighbours=K_MOD)
    alg = gp.vecchia_gp_log_pdf
    with torch.no_grad():
        alg.compute(None, vs)
        first = alg._cache.nbr
        leaves['ls'].data.copy_(torch.tensor([[3.0, 0.3]]))
        alg.compute(None, vs)
        assert alg._cache.nbr is first
        gp.refresh_neighbours()
        alg.compute(None, vs)
        assert alg._cache.nbr is not first and not torch.equal(alg._cache.nbr, first)
        second = alg._cache.nbr
        vs[gp._module_graph.X.uuid] = vs[gp._module_graph.X.uuid].clone()
        alg.compute(None, vs)
        assert alg._cache.nbr is not second and torch.equal(alg._cache.nbr, second)


def test_module_mean_function_and_noise_samples():
    from mxfusion_amd import Variable
    from mxfusion_amd.modules.gp_modules import VecchiaGPRegression
    p = _module_data()
    gp, vs, leaves = _model(VecchiaGPRegression, p, num_neighbours=K_MOD)
    mean = Variable(shape=(N_MOD, 1))
    gpm, vsm, _ = _model(VecchiaGPRegression, dict(p, Y=p['Y'] + 0.7), num_neighbours=K_MOD, mean=mean)
    vsm[mean.uuid] = torch.full((1, N_MOD, 1), 0.7, dtype=torch.float64).cuda()
    with torch.no_grad():
        plain, shifted = gp.vecchia_gp_log_pdf.compute(None, vs), gpm.vecchia_gp_log_pdf.compute(None, vsm)
        assert abs(float(plain[0]) - float(shifted[0])) <= 1e-9 * abs(float(plain[0]))
        vs[leaves['noise_uuid']] = torch.tensor([[0.05], [0.2]], dtype=torch.float64).cuda()
        two = gp.vecchia_gp_log_pdf.compute(None, vs)
    assert tuple(two.shape) == (2,) and abs(float(two[0]) - float(plain[0])) <= 1e-12 * abs(float(plain[0])) and float(two[1]) != float(two[0])
    Xt = np.random.default_rng(1).uniform(-2, 2, (9, 2))
    gp0, vs0, _ = _model(VecchiaGPRegression, p, num_neighbours=K_MOD)
    mu0, _ = _predict(gp0, vs0, 'vecchia_gp_log_pdf', 'vecchia_gp_predict', Xt)[True]
    vsm[mean.uuid] = torch.full((1, N_MOD, 1), 0.7, dtype=torch.float64).cuda()
    mu1, _ = _predict(gpm, vsm, 'vecchia_gp_log_pdf', 'vecchia_gp_predict', Xt, mean=(mean, 0.7))[True]
    assert np.allclose(mu1, mu0 + 0.7, rtol=0, atol=1e-9)


def test_five_adam_steps_lower_the_loss():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.inference import GradBasedInference, MAP
    from mxfusion_amd.modules.gp_modules import VecchiaGPRegression
    p = _module_data()
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64).cuda()
    m = Model()
    m.X = Variable(shape=(N_MOD, 2))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.5)
    m.Y = VecchiaGPRegression.define_variable(X=m.X, kernel=RBF(2, ARD=True, lengthscale=0.5, dtype='float64'), noise_var=m.noise_var, shape=(N_MOD, 1),
                                              num_neighbours=K_MOD, dtype='float64')
    infr = GradBasedInference(MAP(model=m, observed=[m.X, m.Y]), dtype='float64')
    infr.initialize(X=(N_MOD, 2), Y=(N_MOD, 1))
    kern = m.Y.factor.kernel

    def loss():
        q = dict(p, noise=infr.params[m.noise_var].double().cpu().numpy().reshape(1), ls=infr.params[kern.lengthscale].double().cpu().numpy().reshape(2),
                 var=infr.params[kern.variance].double().cpu().numpy().reshape(1))
        gp2, vs2, _ = _model(VecchiaGPRegression, q, num_neighbours=K_MOD)
        with torch.no_grad():
            return -float(gp2.vecchia_gp_log_pdf.compute(None, vs2)[0])
    before = loss()
    infr.run(X=t(p['X']), Y=t(p['Y']), learning_rate=0.05, max_iter=5)
    after = loss()
    print('negative Vecchia log-pdf before', before, 'after', after)
    assert np.isfinite(after) and after < before


def test_module_refusals():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Linear
    from mxfusion_amd.modules.gp_modules import VecchiaGPRegression
    m = Model()
    m.X = Variable(shape=(30, 3))
    m.noise_var = Variable(shape=(1,), initial_value=0.1)
    for kernel in (Linear(3), RBF(2, active_dims=[0, 1]), RBF(3) + RBF(3, name='rbf2'), RBF(17)):
        with pytest.raises(ModelSpecificationError, match='single stationary kernel'):
            VecchiaGPRegression.define_variable(X=m.X, kernel=kernel, noise_var=m.noise_var, shape=(30, 1))
    p = _module_data()
    gp, vs, _ = _model(VecchiaGPRegression, p, num_neighbours=K_MOD)
    vs[gp._module_graph.X.uuid].requires_grad_(True)
    with pytest.raises(NotImplementedError, match='no reverse mode in X'):
        gp.vecchia_gp_log_pdf.compute(None, vs)
