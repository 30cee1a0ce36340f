"""Categorical, Dirichlet and Bernoulli on the MI355X: the row-wise kernels (mxf_categorical_*, mxf_dirichlet_*, simplex.hip), the Bernoulli
kind of the univariate kernels, the classes through the API, their draws, and one MAP run.

Expected values and gradients are float64 torch on the CPU -- log_softmax with gather / sum, torch.distributions.Dirichlet.log_prob on the
normalised x (plus the closed form for an un-normalised one), Bernoulli.log_prob -- with autograd under a random cotangent; never the code
under test.  Inputs are rounded to the dtype under test before either side sees them.  Errors are normwise per output,
|got - want| / max(|want|, tiny).  float64: 1e-9.  float32, per case: max(4 x the worst error of torch's own float32 CPU evaluation of the
same formula on the same inputs, 8 * 2^-24 * M / |want|) with M the norm of the per-output sums of absolute term magnitudes (the floor:
with normalization off torch's float32 pick is exact and its bar would be zero).  float64 has the same floor with 2^-53: it is below 1e-9
unless M / |want| exceeds 5.6e5, which happens in one place -- the Dirichlet's dx at K = 1 with normalization, where x / |x| = 1 whatever x
is, the true gradient is exactly zero, and the float64 reference itself returns rounding noise (1.1e-16 against terms of magnitude 15):
a relative error against that noise is undefined, and this code returns exactly zero there."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 16, 17, 64, 65, 130)          # every group width, its upper edge, the edge + 1, two and more trips of the lane loop
BATCHES = ((1, 1), (1, 7), (3, 5), (2, 33))
P_LAYOUTS = ('own', 'samples', 'batch', 'both')   # the parameter: (S, B, K), shared over samples, over the batch, over both
X_LAYOUTS = ('own', 'samples')
MODES = ((False, True), (False, False), (True, True), (True, False))        # (one_hot, normalize)
F64_BAR = 1e-9
EPS32 = 2.0 ** -24
PREFILL = 0.75
WORST = {}          # (family, dtype) -> (worst error, widest bar): printed for the record of a run


def _tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def _round(a, dtype):
    return np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64)


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=_tdt(dtype)).cuda()


def _np(t):
    return t.detach().double().cpu().numpy()


def nerr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), np.finfo(np.float64).tiny))


def nerr_rows(got, want, keep):
    """nerr over the rows `keep` (S, B) alone"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm((got - want)[keep]) / np.linalg.norm(want[keep]))


def _p_shape(layout, S, B, K):
    return {'own': (S, B, K), 'samples': (1, B, K), 'batch': (S, 1, K), 'both': (1, 1, K)}[layout]


def _sum_to(a, shape):
    """a (S, B, K) summed over the axes where `shape` has extent 1 and a has not"""
    for d, n in enumerate(shape):
        if n == 1 and a.shape[d] != 1:
            a = a.sum(axis=d, keepdims=True)
    return a


def _record(family, dtype, what, names, got, want, bars):
    errs = [nerr(g, w) for g, w in zip(got, want)]
    worst = WORST.get((family, dtype), (0.0, 0.0))
    kept = [(e, b) for e, b in zip(errs, bars) if b < 1.0] or [worst]       # (a reference of zero or of rounding noise: asserted, not tabled)
    WORST[(family, dtype)] = (max(worst[0], max(e for e, _ in kept)), max(worst[1], max(b for _, b in kept)))
    print('%s %s %s: %s; worst so far %.3g, widest bar %.3g'
          % (family, dtype, what, ', '.join('%s %.3g (bar %.3g)' % t for t in zip(names, errs, bars)), *WORST[(family, dtype)]))
    for name, g, w, e, bar in zip(names, got, want, errs, bars):
        assert np.asarray(g).shape == np.asarray(w).shape, (name, np.asarray(g).shape, np.asarray(w).shape)
        assert e <= bar, (what, name, e, bar)


def _bars(dtype, want, own32, mags):
    """per output: 1e-9, or max(4 x torch's float32 error, the floor of the float32 terms); either no lower than 8 ulp of the terms"""
    if dtype == 'float64':
        return [max(F64_BAR, 8 * 2.0 ** -53 * float(np.linalg.norm(m)) / max(float(np.linalg.norm(w)), np.finfo(np.float64).tiny))
                for w, m in zip(want, mags)]
    return [max(4 * nerr(o, w), 8 * EPS32 * float(np.linalg.norm(m)) / max(float(np.linalg.norm(w)), np.finfo(np.float64).tiny))
            for o, w, m in zip(own32, want, mags)]


# ----------------------------------------------------------------------------------------------------------------------------------
# Categorical

def _clip(x, K):
    return np.clip(np.trunc(x), 0, K - 1).astype(np.int64)


def cat_reference(logp, x, cot, one_hot, normalize, dtype):
    """[value (S, B), dlogp like logp, (one_hot) dx like x] in torch `dtype` on the CPU"""
    S, B = cot.shape
    K = logp.shape[-1]
    lp = torch.as_tensor(logp, dtype=dtype).requires_grad_(True)
    xt = torch.as_tensor(x, dtype=dtype).requires_grad_(bool(one_hot))
    l = (torch.log_softmax(lp, -1) if normalize else lp).expand(S, B, K)
    if one_hot:
        v = (xt * l).sum(-1)
    else:
        v = l.gather(-1, torch.as_tensor(_clip(x, K)).expand(S, B).unsqueeze(-1)).squeeze(-1)
    g = torch.autograd.grad((v * torch.as_tensor(cot, dtype=dtype)).sum(), [lp] + ([xt] if one_hot else []), allow_unused=True)
    return [_np(v)] + [np.zeros(t.shape) if gi is None else _np(gi) for gi, t in zip(g, [lp, xt])]


def cat_magnitudes(logp, x, cot, one_hot, normalize):
    """sums of the absolute values of the terms each output is formed from"""
    S, B = cot.shape
    K = logp.shape[-1]
    lpb = np.broadcast_to(logp, (S, B, K))
    m = lpb.max(-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        lse = m + np.log(np.exp(lpb - m).sum(-1, keepdims=True))
        p = np.exp(lpb - lse)
    t = np.broadcast_to(x, (S, B, K)) if one_hot else (np.arange(K) == np.broadcast_to(_clip(x, K), (S, B))[..., None]).astype(np.float64)
    mag_l = np.abs(lpb) + (np.abs(lse) if normalize else 0.0)
    w = np.abs(cot)[..., None]
    mags = [(np.abs(t) * mag_l).sum(-1), _sum_to(w * (np.abs(t) + (p * np.abs(t).sum(-1, keepdims=True) if normalize else 0.0)), logp.shape)]
    if one_hot:
        mags.append(_sum_to(w * mag_l, x.shape))
    return mags


@functools.lru_cache(maxsize=None)
def cat_case(dtype, K, S, B, p_layout, x_layout, one_hot, normalize, spread=1.0, edge_labels=False):
    r = np.random.RandomState(7 * K + 100 * S + B + 1000 * len(p_layout) + len(x_layout) + 2 * one_hot + normalize)
    logp = _round(spread * r.uniform(-1.0, 1.0, _p_shape(p_layout, S, B, K)), dtype)
    Sx = 1 if x_layout == 'samples' else S
    labels = r.randint(0, K, size=(Sx, B))
    labels.flat[0], labels.flat[-1] = 0, K - 1                                  # both ends in every case
    if B == 1 and Sx == 1:
        labels.flat[0] = K - 1
    x = labels.astype(np.float64)
    if edge_labels:
        x = np.where(labels == 0, -1.0, np.where(labels == K - 1, float(K), x))
    if one_hot:
        x = _round(np.eye(K)[labels] * r.uniform(0.5, 1.5, (Sx, B, 1)) + 0.1 * r.uniform(0, 1, (Sx, B, K)), dtype)       # soft rows: dx and sum_j t_j are exercised
    cot = _round(r.uniform(0.5, 1.5, (S, B)), dtype)
    want = cat_reference(logp, x, cot, one_hot, normalize, torch.float64)
    own32 = cat_reference(logp, x, cot, one_hot, normalize, torch.float32) if dtype == 'float32' else None
    return (logp, x, cot), want, _bars(dtype, want, own32, cat_magnitudes(logp, x, cot, one_hot, normalize))


def cat_run(dtype, logp, x, cot, one_hot, normalize, scale=1.0):
    from mxfusion_amd import ops
    lp, xd, c = _dev(logp, dtype), _dev(x, dtype), _dev(cot, dtype)
    out = ops.categorical_logpdf(lp, xd.expand((cot.shape[0],) + xd.shape[1:]), one_hot, normalize, scale)       # (a view: S rows even where all is shared)
    dlp = torch.zeros_like(lp)
    dx = torch.zeros_like(xd) if one_hot else None
    ops.categorical_logpdf_bwd_(lp, xd, c, one_hot, normalize, scale, dlp, dx)
    torch.cuda.synchronize()
    return [_np(out), _np(dlp)] + ([_np(dx)] if one_hot else [])


def cat_check(dtype, K, S, B, p_layout='own', x_layout='own', modes=MODES, **kw):
    for one_hot, normalize in modes:
        (logp, x, cot), want, bars = cat_case(dtype, K, S, B, p_layout, x_layout, one_hot, normalize, **kw)
        got = cat_run(dtype, logp, x, cot, one_hot, normalize)
        n = 3 if one_hot else 2
        _record('categorical', dtype, 'K=%d (S, B)=(%d, %d) p %s x %s one_hot=%d normalize=%d' % (K, S, B, p_layout, x_layout, one_hot, normalize),
                ('value', 'dlogp', 'dx')[:n], got, want[:n], bars[:n])


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('K', KS)
def test_categorical_class_counts(K, dtype):
    cat_check(dtype, K, 3, 5)
    cat_check(dtype, K, 2, 33, 'both', 'samples')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('S,B', BATCHES)
def test_categorical_batches(S, B, dtype):
    for K in (3, 16, 65):
        cat_check(dtype, K, S, B)
        cat_check(dtype, K, S, B, 'batch', 'own', modes=MODES[:1] + MODES[2:3])


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('x_layout', X_LAYOUTS)
@pytest.mark.parametrize('p_layout', P_LAYOUTS)
def test_categorical_sharing_layouts(p_layout, x_layout, dtype):
    cat_check(dtype, 5, 3, 5, p_layout, x_layout)
    cat_check(dtype, 17, 2, 33, p_layout, x_layout)
    cat_check(dtype, 130, 3, 5, p_layout, x_layout, modes=MODES[2:3])


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_categorical_labels_are_clipped(dtype):
    """-1 and K give what 0 and K - 1 give (MXNet's pick, mode 'clip'); a fractional label is truncated toward zero"""
    for K in (3, 17):
        (logp, x, cot), want, bars = cat_case(dtype, K, 3, 5, 'own', 'own', False, True, edge_labels=True)
        assert x.min() == -1 and x.max() == K
        inside = _clip(x, K).astype(np.float64)
        got, ref = cat_run(dtype, logp, x, cot, False, True), cat_run(dtype, logp, inside, cot, False, True)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))
        assert all(np.array_equal(g, r) for g, r in zip(cat_run(dtype, logp, inside + 0.75 * (inside < K - 1), cot, False, True), ref))
        _record('categorical', dtype, 'K=%d clipped labels' % K, ('value', 'dlogp'), got, want[:2], bars[:2])


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_categorical_wide_spread_and_an_impossible_row(dtype):
    """log_prob within +-80: exp overflows float32 unless the row maximum is subtracted first.  A row of all -inf is NaN, alone."""
    cat_check(dtype, 17, 3, 5, spread=80.0, modes=MODES[:1] + MODES[2:3])
    (logp, x, cot), want, bars = cat_case(dtype, 5, 3, 5, 'own', 'own', False, True)
    logp = logp.copy()
    logp[1, 2] = -np.inf
    value, dlp = cat_run(dtype, logp, x, cot, False, True)
    bad = np.zeros((3, 5), dtype=bool)
    bad[1, 2] = True
    assert np.isnan(value[bad]).all() and np.isfinite(value[~bad]).all() and np.isfinite(dlp[~bad]).all()
    assert nerr_rows(value, want[0], ~bad) <= bars[0] and nerr_rows(dlp, want[1], ~bad) <= bars[1]


# ----------------------------------------------------------------------------------------------------------------------------------
# Dirichlet

def dir_reference(x, alpha, cot, normalize, dtype):
    """[value (S, B), dx like x, dalpha like alpha]: torch.distributions on the normalised x; for an un-normalised one the closed form"""
    xt, at = torch.as_tensor(x, dtype=dtype).requires_grad_(True), torch.as_tensor(alpha, dtype=dtype).requires_grad_(True)
    if normalize:
        v = torch.distributions.Dirichlet(at, validate_args=False).log_prob(xt / xt.abs().sum(-1, keepdim=True))
    else:
        v = ((at - 1) * torch.log(xt)).sum(-1) + torch.lgamma(at.sum(-1)) - torch.lgamma(at).sum(-1)
    v = v.expand(cot.shape)
    g = torch.autograd.grad((v * torch.as_tensor(cot, dtype=dtype)).sum(), [xt, at])
    return [_np(v), _np(g[0]), _np(g[1])]


def dir_magnitudes(x, alpha, cot, normalize):
    from scipy.special import digamma, gammaln
    S, B = cot.shape
    K = x.shape[-1]
    xb, ab = np.broadcast_to(x, (S, B, K)), np.broadcast_to(alpha, (S, B, K))
    n1 = np.abs(xb).sum(-1, keepdims=True) if normalize else 1.0
    lx, sa = np.abs(np.log(xb / n1)), ab.sum(-1, keepdims=True)
    w = np.abs(cot)[..., None]
    return [(np.abs(ab - 1) * lx).sum(-1) + np.abs(gammaln(sa[..., 0])) + np.abs(gammaln(ab)).sum(-1),
            _sum_to(w * (np.abs(ab - 1) / xb + (np.abs(ab - 1).sum(-1, keepdims=True) / n1 if normalize else 0.0)), x.shape),
            _sum_to(w * (lx + np.abs(digamma(sa)) + np.abs(digamma(ab))), alpha.shape)]


@functools.lru_cache(maxsize=None)
def dir_case(dtype, K, S, B, p_layout, x_layout, normalize, alpha_value=None):
    r = np.random.RandomState(11 * K + 100 * S + B + 1000 * len(p_layout) + len(x_layout) + normalize)
    alpha = _round(r.uniform(0.3, 5.0, _p_shape(p_layout, S, B, K)) if alpha_value is None else np.full(_p_shape(p_layout, S, B, K), alpha_value), dtype)
    x = r.uniform(0.2, 3.0, (1 if x_layout == 'samples' else S, B, K))
    if not normalize:
        x = x / x.sum(-1, keepdims=True)                 # on the simplex (up to the rounding to dtype)
    x, cot = _round(x, dtype), _round(r.uniform(0.5, 1.5, (S, B)), dtype)
    want = dir_reference(x, alpha, cot, normalize, torch.float64)
    own32 = dir_reference(x, alpha, cot, normalize, torch.float32) if dtype == 'float32' else None
    return (x, alpha, cot), want, _bars(dtype, want, own32, dir_magnitudes(x, alpha, cot, normalize))


def dir_run(dtype, x, alpha, cot, normalize, scale=1.0, grads=True):
    from mxfusion_amd import ops
    xd, ad, c = _dev(x, dtype), _dev(alpha, dtype), _dev(cot, dtype)
    out = ops.dirichlet_logpdf(xd.expand((cot.shape[0],) + xd.shape[1:]), ad, normalize, scale)       # (a view: S rows even where all is shared)
    dx, da = torch.zeros_like(xd), torch.zeros_like(ad)
    if grads:
        ops.dirichlet_logpdf_bwd_(xd, ad, c, normalize, scale, dx, da)
    torch.cuda.synchronize()
    return [_np(out), _np(dx), _np(da)]


def dir_check(dtype, K, S, B, p_layout='own', x_layout='own', **kw):
    for normalize in (True, False):
        (x, alpha, cot), want, bars = dir_case(dtype, K, S, B, p_layout, x_layout, normalize, **kw)
        _record('dirichlet', dtype, 'K=%d (S, B)=(%d, %d) alpha %s x %s normalize=%d' % (K, S, B, p_layout, x_layout, normalize),
                ('value', 'dx', 'dalpha'), dir_run(dtype, x, alpha, cot, normalize), want, bars)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('K', KS)
def test_dirichlet_class_counts(K, dtype):
    dir_check(dtype, K, 3, 5)
    dir_check(dtype, K, 2, 33, 'both', 'samples')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('S,B', BATCHES)
def test_dirichlet_batches(S, B, dtype):
    for K in (3, 16, 65):
        dir_check(dtype, K, S, B)
        dir_check(dtype, K, S, B, 'batch', 'own')


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('x_layout', X_LAYOUTS)
@pytest.mark.parametrize('p_layout', P_LAYOUTS)
def test_dirichlet_sharing_layouts(p_layout, x_layout, dtype):
    dir_check(dtype, 5, 3, 5, p_layout, x_layout)
    dir_check(dtype, 17, 2, 33, p_layout, x_layout)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_dirichlet_large_alpha_and_scipy(dtype):
    """alpha = 200 at K = 3: Gamma(200) overflows a double, lgamma does not.  Values also against SciPy where it is importable."""
    dir_check(dtype, 3, 3, 5, alpha_value=200.0)
    try:
        from scipy.stats import dirichlet as sp
    except ImportError:
        return
    for K, alpha_value in ((3, 200.0), (5, None)):
        (x, alpha, cot), want, bars = dir_case(dtype, K, 3, 5, 'own', 'own', True, alpha_value)
        xn = x / np.abs(x).sum(-1, keepdims=True)
        ref = np.array([[sp.logpdf(xn[s, b] / xn[s, b].sum(), alpha[s, b]) for b in range(5)] for s in range(3)])
        assert nerr(want[0], ref) <= 1e-12
        assert nerr(dir_run(dtype, x, alpha, cot, True, grads=False)[0], ref) <= bars[0]


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_dirichlet_failed_rows_are_nan_alone(dtype):
    (x, alpha, cot), want, bars = dir_case(dtype, 5, 3, 5, 'own', 'own', True)
    x, alpha = x.copy(), alpha.copy()
    x[0, 1, 2] = 0.0
    alpha[2, 3, 4] = -1.0
    value, dx, da = dir_run(dtype, x, alpha, cot, True)
    bad = np.zeros((3, 5), dtype=bool)
    bad[0, 1] = bad[2, 3] = True
    assert np.isnan(value[bad]).all() and np.isnan(dx[bad]).all() and np.isnan(da[bad]).all()
    for g, w, bar in zip((value, dx, da), want, bars):
        assert np.isfinite(g[~bad]).all() and nerr_rows(g, w, ~bad) <= bar


# ----------------------------------------------------------------------------------------------------------------------------------
# contracts of the wrappers and of the C ABI

def test_expanded_operands_are_passed_without_a_copy():
    from mxfusion_amd import ops
    S, B, K = 3, 5, 6
    (logp, x, cot), _, _ = cat_case('float64', K, S, B, 'both', 'samples', True, True)
    lp, xd, c = _dev(logp, 'float64'), _dev(x, 'float64'), _dev(cot, 'float64')
    for t, axes in ((lp, (0, 1)), (xd, (0,))):
        e = t.expand((S, B, K))
        got, ss, sb = ops._simplex_operand(e, axes)
        assert got.data_ptr() == t.data_ptr() and ss == 0 and (sb == 0 if axes == (0, 1) else sb == K)
    dense, ss, sb = ops._simplex_operand(lp.expand(S, B, K).contiguous(), (0, 1))
    assert (ss, sb) == (B * K, K)
    padded = torch.zeros(S, B, K + 2, dtype=torch.float64).cuda()[..., :K]
    assert ops._simplex_operand(padded, (0, 1))[0].is_contiguous()
    want = ops.categorical_logpdf(lp.expand(S, B, K).contiguous(), xd.expand(S, B, K).contiguous(), True, True)
    assert torch.equal(ops.categorical_logpdf(lp.expand(S, B, K), xd.expand(S, B, K), True, True), want)
    assert torch.equal(ops.categorical_logpdf(lp, xd, True, True), want[:1])         # nothing has a sample axis: one row of samples
    d1, d2 = torch.zeros_like(lp), torch.zeros_like(xd)
    ops.categorical_logpdf_bwd_(lp.expand(S, B, K), xd.expand(S, B, K), c, True, True, 1.0, d1, d2)
    full = [torch.zeros(S, B, K, dtype=torch.float64).cuda() for _ in range(2)]
    ops.categorical_logpdf_bwd_(lp.expand(S, B, K).contiguous(), xd.expand(S, B, K).contiguous(), c, True, True, 1.0, *full)
    assert nerr(_np(d1), _np(full[0].sum((0, 1), keepdim=True))) < 1e-14 and nerr(_np(d2), _np(full[1].sum(0, keepdim=True))) < 1e-14
    (x, alpha, cot), _, _ = dir_case('float64', K, S, B, 'samples', 'samples', True)
    xd, ad = _dev(x, 'float64'), _dev(alpha, 'float64')
    assert torch.equal(ops.dirichlet_logpdf(xd.expand(S, B, K), ad.expand(S, B, K)), ops.dirichlet_logpdf(xd, ad).expand(S, B))


def test_wrappers_refuse_mixed_dtypes_and_strided_buffers():
    from mxfusion_amd import ops
    lp, x = torch.zeros(2, 3, 4, dtype=torch.float64).cuda(), torch.zeros(2, 3, dtype=torch.float64).cuda()
    with pytest.raises(TypeError):
        ops.categorical_logpdf(lp, x.float())
    with pytest.raises(TypeError):
        ops.categorical_logpdf(lp, x.long())
    with pytest.raises(TypeError):
        ops.dirichlet_logpdf(lp.float(), lp)
    with pytest.raises(TypeError):
        ops.dirichlet_logpdf(lp.half(), lp.half())
    with pytest.raises(ValueError):
        ops.categorical_logpdf_bwd_(lp, x, torch.zeros(3, 2, dtype=torch.float64).cuda().t(), dlogp_acc=torch.zeros_like(lp))
    with pytest.raises(ValueError):
        ops.dirichlet_logpdf_bwd_(lp, lp, torch.zeros(2, 3, dtype=torch.float64).cuda(), dx_acc=torch.zeros(2, 3, 8, dtype=torch.float64).cuda()[..., ::2])
    with pytest.raises(ValueError):
        ops.dirichlet_logpdf_bwd_(lp, lp, torch.zeros(2, 3, dtype=torch.float64).cuda(), dx_acc=torch.zeros(1, 3, 4, dtype=torch.float64).cuda())


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_accumulation_contract(dtype):
    """gradients are added to what the buffers hold, out is written, and a null output leaves the others as they were"""
    from mxfusion_amd import ops
    for p_layout in ('own', 'both'):
        (logp, x, cot), want, bars = cat_case(dtype, 5, 3, 5, p_layout, 'samples', True, True)
        lp, xd, c = _dev(logp, dtype), _dev(x, dtype), _dev(cot, dtype)
        both = [torch.full_like(lp, PREFILL), torch.full_like(xd, PREFILL)]
        ops.categorical_logpdf_bwd_(lp, xd, c, True, True, 1.0, *both)
        only = [torch.full_like(lp, PREFILL), torch.full_like(xd, PREFILL)]
        ops.categorical_logpdf_bwd_(lp, xd, c, True, True, 1.0, only[0], None)
        ops.categorical_logpdf_bwd_(lp, xd, c, True, True, 1.0, None, only[1])
        for b, o, w, bar in zip(both, only, want[1:], bars[1:]):
            assert nerr(_np(b) - PREFILL, w) <= bar + 4 * (EPS32 if dtype == 'float32' else 2.0 ** -53) * PREFILL * np.sqrt(w.size) / np.linalg.norm(w)
            assert nerr(_np(b), _np(o)) <= 4 * (EPS32 if dtype == 'float32' else 2.0 ** -53)      # (sums over the batch axis: atomics, any order)
        (x, alpha, cot), want, bars = dir_case(dtype, 5, 3, 5, p_layout, 'samples', True)
        xd, ad, c = _dev(x, dtype), _dev(alpha, dtype), _dev(cot, dtype)
        both = [torch.full_like(xd, PREFILL), torch.full_like(ad, PREFILL)]
        ops.dirichlet_logpdf_bwd_(xd, ad, c, True, 1.0, *both)
        only = [torch.full_like(xd, PREFILL), torch.full_like(ad, PREFILL)]
        ops.dirichlet_logpdf_bwd_(xd, ad, c, True, 1.0, only[0], None)
        ops.dirichlet_logpdf_bwd_(xd, ad, c, True, 1.0, None, only[1])
        for b, o, w, bar in zip(both, only, want[1:], bars[1:]):
            assert nerr(_np(b) - PREFILL, w) <= bar + 4 * (EPS32 if dtype == 'float32' else 2.0 ** -53) * PREFILL * np.sqrt(w.size) / np.linalg.norm(w)
            assert nerr(_np(b), _np(o)) <= 4 * (EPS32 if dtype == 'float32' else 2.0 ** -53)      # (sums over the batch axis: atomics, any order)
        # out is written: two calls give the same values, and scale multiplies them
        assert torch.equal(ops.dirichlet_logpdf(xd, ad), ops.dirichlet_logpdf(xd, ad))
        assert nerr(_np(ops.dirichlet_logpdf(xd, ad, True, 2.0)), 2 * _np(ops.dirichlet_logpdf(xd, ad))) < 1e-6


def test_status_codes():
    from mxfusion_amd import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    dt = torch.float64
    S, B, K = 2, 3, 4
    lp, x1, xk = torch.zeros(S, B, K, dtype=dt).cuda(), torch.zeros(S, B, dtype=dt).cuda(), torch.full((S, B, K), 0.25, dtype=dt).cuda()
    cot, out = torch.ones(S, B, dtype=dt).cuda(), torch.full((S, B), 7.0, dtype=dt).cuda()
    g, g2 = torch.zeros(S, B, K, dtype=dt).cuda(), torch.zeros(S, B, K, dtype=dt).cuda()
    h = _lib.handle(0)
    P = lambda t: None if t is None else t.data_ptr()

    def cat(dtype=_lib.F64, S=S, B=B, K=K, logp=lp, ss=B * K, sb=K, x=x1, ssx=B, one_hot=0, out=out, h=h):
        return lib.mxf_categorical_logpdf(h, dtype, S, B, K, P(logp), ss, sb, P(x), ssx, one_hot, 1, 1.0, P(out), st)

    def cat_bwd(dtype=_lib.F64, K=K, logp=lp, ss=B * K, x=x1, ssx=B, one_hot=0, cot=cot, dlp=g, dx=None, h=h):
        return lib.mxf_categorical_logpdf_bwd(h, dtype, S, B, K, P(logp), ss, K, P(x), ssx, one_hot, 1, P(cot), 1.0, P(dlp), P(dx), st)

    def dirichlet(dtype=_lib.F64, S=S, K=K, x=xk, ssx=B * K, alpha=xk, ss=B * K, sb=K, out=out, h=h):
        return lib.mxf_dirichlet_logpdf(h, dtype, S, B, K, P(x), ssx, P(alpha), ss, sb, 1, 1.0, P(out), st)

    def dirichlet_bwd(dtype=_lib.F64, K=K, x=xk, ssx=B * K, alpha=xk, ss=B * K, cot=cot, dx=g, h=h):
        return lib.mxf_dirichlet_logpdf_bwd(h, dtype, S, B, K, P(x), ssx, P(alpha), ss, K, 1, P(cot), 1.0, P(dx), None, st)

    def refused(name, rc):
        assert rc == -2, (name, rc)
        assert name + ':' in lib.mxf_last_error(h).decode(), lib.mxf_last_error(h)

    assert cat(h=None) == -1 and cat_bwd(h=None) == -1 and dirichlet(h=None) == -1 and dirichlet_bwd(h=None) == -1
    for name, fn in (('mxf_categorical_logpdf', cat), ('mxf_categorical_logpdf_bwd', cat_bwd), ('mxf_dirichlet_logpdf', dirichlet),
                     ('mxf_dirichlet_logpdf_bwd', dirichlet_bwd)):
        refused(name, fn(dtype=7))
        refused(name, fn(K=0))
        refused(name, fn(x=None))
        refused(name, fn(ss=B * K + 1))
        refused(name, fn(ssx=1))
    refused('mxf_categorical_logpdf', cat(logp=None))
    refused('mxf_categorical_logpdf', cat(out=None))
    refused('mxf_categorical_logpdf', cat(sb=K + 1))
    refused('mxf_categorical_logpdf', cat(ssx=B * K))                        # the labels' dense stride is B
    refused('mxf_categorical_logpdf', cat(x=xk, ssx=B, one_hot=1))            # the one-hot rows' is B * K
    refused('mxf_categorical_logpdf_bwd', cat_bwd(cot=None))
    refused('mxf_categorical_logpdf_bwd', cat_bwd(dx=g))                      # a class index has no gradient
    assert cat_bwd(x=xk, ssx=B * K, one_hot=1, dx=g2) == 0
    refused('mxf_dirichlet_logpdf', dirichlet(alpha=None))
    refused('mxf_dirichlet_logpdf', dirichlet(out=None))
    refused('mxf_dirichlet_logpdf', dirichlet(sb=1))
    refused('mxf_dirichlet_logpdf_bwd', dirichlet_bwd(cot=None))
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0              # no refused call wrote
    assert cat(S=0) == 0 and dirichlet(S=0) == 0 and cat(B=0) == 0
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    assert cat() == 0 and dirichlet() == 0


# ----------------------------------------------------------------------------------------------------------------------------------
# Bernoulli on the univariate kernels

@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('S', [1, 4])
@pytest.mark.parametrize('n', [1, 5, 300])
def test_bernoulli_kernels(n, S, dtype):
    from mxfusion_amd import ops
    r = np.random.RandomState(13 * n + S)
    x = (r.uniform(size=(S, n)) < 0.5).astype(np.float64)
    x.flat[0], x.flat[-1] = 1.0, 0.0
    if n > 1:
        x[0, 1] = 0.25                                                           # a fractional observation: the formula is linear in x
    cot = _round(r.uniform(0.5, 1.5, (S, n)), dtype)
    for p_shape in ((1,), (n,), (S, n)):
        p = _round(r.uniform(0.05, 0.95, p_shape), dtype)

        def ref(tdt, c):
            xt, pt = torch.as_tensor(x, dtype=tdt).requires_grad_(True), torch.as_tensor(p, dtype=tdt).requires_grad_(True)
            v = torch.distributions.Bernoulli(probs=pt, validate_args=False).log_prob(xt).expand(S, n)
            g = torch.autograd.grad((v * torch.as_tensor(c, dtype=tdt)).sum(), [xt, pt])
            return [_np(v), _np(g[0]), _np(g[1])]

        def mags(w):
            pb = np.broadcast_to(p, (S, n))
            la, l1 = np.abs(np.log(pb)), np.abs(np.log1p(-pb))
            mp = w * (x / pb + np.abs(1 - x) / (1 - pb))
            return [x * la + np.abs(1 - x) * l1, w * (la + l1), mp if p.shape == (S, n) else (mp.sum(0) if p.shape == (n,) else mp.sum().reshape(1))]
        want = ref(torch.float64, cot)
        bars = _bars(dtype, want, ref(torch.float32, cot) if dtype == 'float32' else None, mags(np.abs(cot)))
        xd, pd, c = _dev(x, dtype), _dev(p, dtype), _dev(cot, dtype)
        out = ops.univariate_logpdf_elem('bernoulli', xd, pd, pd, 1.0)
        dx, dp, db = torch.zeros_like(xd), torch.zeros_like(pd), torch.full_like(pd, PREFILL)
        ops.univariate_logpdf_bwd_('bernoulli', xd, pd, pd, c, 1.0, dx, dp, db)
        assert float(db.min()) == PREFILL and float(db.max()) == PREFILL          # gb = 0: the buffer is as it was
        _record('bernoulli', dtype, 'n=%d S=%d p%s' % (n, S, p_shape), ('value', 'dx', 'dp'), [_np(out), _np(dx), _np(dp)], want, bars)
        if p.shape != (S, n):                                                     # the reduced kernel: parameters without a sample axis
            half = np.full((S, n), 0.5)

            def reduced(tdt):
                v, gx, gp = ref(tdt, half)
                return [0.5 * v.sum().reshape(1), gx, gp]
            m = mags(half)
            want2 = reduced(torch.float64)
            bars2 = _bars(dtype, want2, reduced(torch.float32) if dtype == 'float32' else None, [0.5 * m[0].sum().reshape(1), m[1], m[2]])
            acc, dx2, dp2 = torch.zeros(1, dtype=_tdt(dtype)).cuda(), torch.zeros_like(xd), torch.zeros_like(pd)
            ops.univariate_logpdf_('bernoulli', xd, pd, pd, 0.5, acc, dx2, dp2, None)
            _record('bernoulli', dtype, 'n=%d S=%d p%s reduced' % (n, S, p_shape), ('sum', 'dx', 'dp'), [_np(acc), _np(dx2), _np(dp2)], want2, bars2)


# ----------------------------------------------------------------------------------------------------------------------------------
# through the API

def _add_sample_axis(a, is_samples):
    return a if is_samples else a[None]


# (log_prob shape, has samples, rv shape, has samples, num_samples, one_hot, normalization): categorical_test.py::test_log_pdf
CAT_API = (((5, 4, 3), True, (5, 4, 1), True, 5, False, True), ((4, 3), False, (4, 1), False, 1, False, False),
           ((5, 4, 3), True, (4, 1), False, 5, False, True), ((4, 3), False, (5, 4, 1), True, 5, False, False),
           ((5, 4, 3), True, (4,), False, 5, True, True), ((4, 3), False, (5, 4), True, 5, True, False))
# (alpha shape, has samples, rv shape, has samples, num_samples): dirichlet_test.py::test_log_pdf_with_broadcast
DIR_API = (((3, 2), False, (5, 3, 2), True, 5), ((10, 3, 2), True, (10, 3, 2), True, 10), ((3, 2), False, (3, 2), False, 5))


@pytest.mark.parametrize('case', range(len(CAT_API)))
def test_categorical_log_pdf_through_the_api(case):
    from mxfusion_amd.components.distributions import Categorical
    lp_shape, lp_s, rv_shape, rv_s, S, one_hot, normalization = CAT_API[case]
    r = np.random.RandomState(40 + case)
    logp = _add_sample_axis(r.rand(*lp_shape) + 1e-2, lp_s)
    labels = r.randint(0, 3, size=rv_shape)
    rv = _add_sample_axis(np.eye(3)[labels] if one_hot else labels.astype(np.float64), rv_s)
    lead = rv.shape[1:-1]
    cot = r.uniform(0.5, 1.5, (S,) + lead)
    lt = torch.as_tensor(logp).requires_grad_(True)
    l = (torch.log_softmax(lt, -1) if normalization else lt).expand((S,) + lead + (3,))
    rt = torch.as_tensor(np.broadcast_to(rv, (S,) + rv.shape[1:]).copy())
    want = (rt * l).sum(-1) if one_hot else l.gather(-1, rt.long()).squeeze(-1)
    want_g, = torch.autograd.grad((want * torch.as_tensor(cot)).sum(), [lt])
    for scaling in (1, 3):
        cat = Categorical.define_variable(0, num_classes=3, one_hot_encoding=one_hot, normalization=normalization, shape=rv.shape[1:],
                                          dtype='float64').factor
        cat.log_pdf_scaling = scaling
        ld = _dev(logp, 'float64').requires_grad_(True)
        rd = torch.as_tensor(rv).cuda() if one_hot else torch.as_tensor(rv).long().cuda()      # integer labels are cast
        got = cat.log_pdf(F=None, variables={cat.log_prob.uuid: ld, cat.random_variable.uuid: rd})
        assert got.dtype == torch.float64 and tuple(got.shape) == (S,) + lead
        g, = torch.autograd.grad((got * _dev(cot, 'float64')).sum(), [ld])
        assert nerr(_np(got), scaling * _np(want)) <= F64_BAR and nerr(_np(g), scaling * _np(want_g)) <= F64_BAR


@pytest.mark.parametrize('case', range(len(DIR_API)))
def test_dirichlet_log_pdf_through_the_api(case):
    from mxfusion_amd.components.distributions import Dirichlet
    a_shape, a_s, rv_shape, rv_s, S = DIR_API[case]
    r = np.random.RandomState(50 + case)
    alpha, rv = _add_sample_axis(r.rand(*a_shape) + 0.1, a_s), _add_sample_axis(r.rand(*rv_shape) + 0.05, rv_s)
    S = max(alpha.shape[0], rv.shape[0])                                         # (the third case has no sample axis anywhere)
    cot = r.uniform(0.5, 1.5, (S, 3))
    want = dir_reference(np.broadcast_to(rv, (S, 3, 2)).copy(), alpha, cot, True, torch.float64)
    d = Dirichlet.define_variable(alpha=0, shape=(3, 2), dtype='float64').factor
    d.log_pdf_scaling = 3                                                        # dirichlet.py:64 does not apply it
    ad, xd = _dev(alpha, 'float64').requires_grad_(True), _dev(rv, 'float64').requires_grad_(True)
    got = d.log_pdf(F=None, variables={d.alpha.uuid: ad, d.random_variable.uuid: xd})
    assert got.dtype == torch.float64 and tuple(got.shape) == (S, 3)
    gx, ga = torch.autograd.grad((got * _dev(cot, 'float64')).sum(), [xd, ad])
    assert nerr(_np(got), want[0]) <= F64_BAR and nerr(_np(ga), want[2]) <= F64_BAR
    assert nerr(_np(gx), _sum_to(want[1], rv.shape)) <= F64_BAR


@pytest.mark.parametrize('p_shape,rv_shape,S', [((5, 3, 2), (5, 3, 2), 5), ((3, 2), (5, 3, 2), 5), ((5, 3, 2), (3, 2), 5), ((1,), (3, 2), 1)])
def test_bernoulli_log_pdf_through_the_api(p_shape, rv_shape, S):
    from mxfusion_amd.components.distributions import Bernoulli
    r = np.random.RandomState(60 + len(p_shape) + len(rv_shape))
    p = _add_sample_axis(r.uniform(0.05, 0.95, p_shape), len(p_shape) == 3)
    if p_shape == (1,):
        p = p.reshape(1, 1, 1)
    rv = _add_sample_axis((r.rand(*rv_shape) < 0.5), len(rv_shape) == 3)
    cot = r.uniform(0.5, 1.5, (S, 3, 2))
    pt = torch.as_tensor(p).requires_grad_(True)
    want = torch.distributions.Bernoulli(probs=pt).log_prob(torch.as_tensor(rv).double()).expand(S, 3, 2)
    want_g, = torch.autograd.grad((want * torch.as_tensor(cot)).sum(), [pt], retain_graph=True)
    b = Bernoulli.define_variable(prob_true=0, shape=(3, 2), dtype='float64').factor
    b.log_pdf_scaling = 3
    pd = _dev(p, 'float64').requires_grad_(True)
    variables = {b.prob_true.uuid: pd, b.random_variable.uuid: torch.as_tensor(rv).cuda()}      # boolean observations are cast
    got = b.log_pdf(F=None, variables=variables)
    assert got.dtype == torch.float64 and tuple(got.shape) == (S, 3, 2)
    g, = torch.autograd.grad((got * _dev(cot, 'float64')).sum(), [pd], retain_graph=True)
    assert nerr(_np(got), 3 * _np(want)) <= F64_BAR and nerr(_np(g), 3 * _np(want_g)) <= F64_BAR
    total = b.log_pdf_sum(None, variables)                                     # what FactorGraph.log_pdf adds
    g2, = torch.autograd.grad(total, [pd])
    assert abs(float(total) - 3 * float(want.mean(0).sum())) <= F64_BAR * abs(3 * float(want.mean(0).sum()))
    assert nerr(_np(g2), 3 * _np(torch.autograd.grad(want.mean(0).sum(), [pt])[0])) <= F64_BAR


def test_mock_draws_on_the_device():
    from mxfusion_amd.components.distributions import Bernoulli, Categorical, Dirichlet, MockRandomGenerator
    S = 5
    r = np.random.RandomState(70)
    labels = torch.as_tensor(r.randint(0, 3, size=S * 4).astype(np.float64)).cuda()
    logp = _dev(r.rand(1, 4, 3), 'float64')
    for one_hot in (False, True):
        shape = (4, 3) if one_hot else (4, 1)
        cat = Categorical.define_variable(0, num_classes=3, one_hot_encoding=one_hot, shape=shape, rand_gen=MockRandomGenerator(labels),
                                          dtype='float64').factor
        draw = cat.draw_samples(F=None, variables={cat.log_prob.uuid: logp}, num_samples=S)
        want = labels.reshape(S, 4)
        assert draw.is_cuda and draw.dtype == torch.float64
        assert torch.equal(draw, torch.nn.functional.one_hot(want.long(), 3).double() if one_hot else want.reshape(S, 4, 1))
    gam = _dev(r.rand(S * 6) + 0.1, 'float64')
    d = Dirichlet.define_variable(alpha=0, shape=(3, 2), rand_gen=MockRandomGenerator(gam), dtype='float64').factor
    draw = d.draw_samples(F=None, variables={d.alpha.uuid: _dev(r.rand(1, 3, 2) + 0.5, 'float64')}, num_samples=S)
    assert torch.equal(draw, gam.reshape(S, 3, 2) / gam.reshape(S, 3, 2).sum(-1, keepdim=True))
    bits = _dev((r.rand(S * 6) < 0.5).astype(np.float64), 'float64')
    b = Bernoulli.define_variable(prob_true=0, shape=(3, 2), rand_gen=MockRandomGenerator(bits), dtype='float64').factor
    draw = b.draw_samples(F=None, variables={b.prob_true.uuid: torch.full((1, 3, 2), 0.5, dtype=torch.float64).cuda()}, num_samples=S)
    assert torch.equal(draw, bits.reshape(S, 3, 2))


def test_device_draws_follow_their_distributions():
    """20 000 draws: class frequencies within 5 standard errors of softmax(log_prob) (exp(log_prob) without normalization) and of p; Dirichlet
    draws sum to 1 along the class axis"""
    from mxfusion_amd.components.distributions import Bernoulli, Categorical, Dirichlet
    torch.manual_seed(5)
    N = 20000
    logp = np.log(np.array([[0.1, 0.6, 0.3], [0.5, 0.25, 0.25]]))
    for normalization, shift in ((True, 1.5), (False, 0.0)):
        for one_hot in (False, True):
            cat = Categorical.define_variable(0, num_classes=3, one_hot_encoding=one_hot, normalization=normalization,
                                              shape=(2, 3) if one_hot else (2, 1), dtype='float64').factor
            draw = cat.draw_samples(F=None, variables={cat.log_prob.uuid: _dev(logp[None] + shift, 'float64')}, num_samples=N)
            assert tuple(draw.shape) == ((N, 2, 3) if one_hot else (N, 2, 1))
            onehot = draw if one_hot else torch.nn.functional.one_hot(draw.long()[..., 0], 3).double()
            freq, p = _np(onehot.mean(0)), np.exp(logp)
            assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N)).all(), (freq, p)
    p = np.array([0.1, 0.5, 0.8])
    b = Bernoulli.define_variable(prob_true=0, shape=(3,), dtype='float64').factor
    draw = b.draw_samples(F=None, variables={b.prob_true.uuid: _dev(p[None], 'float64')}, num_samples=N)
    assert tuple(draw.shape) == (N, 3) and draw.dtype == torch.float64 and set(np.unique(_np(draw))) <= {0.0, 1.0}
    assert (np.abs(_np(draw.mean(0)) - p) <= 5 * np.sqrt(p * (1 - p) / N)).all()
    d = Dirichlet.define_variable(alpha=0, shape=(3, 4), dtype='float64').factor
    alpha = np.random.RandomState(1).uniform(0.5, 3.0, (1, 3, 4))
    draw = d.draw_samples(F=None, variables={d.alpha.uuid: _dev(alpha, 'float64')}, num_samples=N)
    assert tuple(draw.shape) == (N, 3, 4) and float((draw.sum(-1) - 1).abs().max()) < 1e-12 and float(draw.min()) >= 0
    mean = alpha[0] / alpha[0].sum(-1, keepdims=True)
    var = mean * (1 - mean) / (alpha[0].sum(-1, keepdims=True) + 1)
    assert (np.abs(_np(draw.mean(0)) - mean) <= 5 * np.sqrt(var / N)).all()


def test_map_classification_end_to_end():
    """logits (3,) under Normal(0, 10), 40 fixed labels under Categorical(logits): the log_prob is shared by every row, so its gradient is
    the batch-shared path (atomics into double) inside a real step."""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Categorical, Normal
    from mxfusion_amd.inference import GradBasedInference, MAP
    y = np.random.RandomState(80).choice(3, size=(40, 1), p=[0.2, 0.5, 0.3]).astype(np.float64)
    m = Model()
    m.logits = Normal.define_variable(mean=0., variance=10., shape=(3,), dtype='float64')
    m.y = Categorical.define_variable(log_prob=m.logits, num_classes=3, shape=(40, 1), dtype='float64')
    alg = MAP(model=m, observed=[m.y])
    infr = GradBasedInference(inference_algorithm=alg, dtype='float64')
    yd = _dev(y, 'float64')
    infr.initialize(y=yd)
    loc = alg.posterior[m.logits].factor.location

    def closed_form(z):
        prior = torch.distributions.Normal(0.0, float(np.sqrt(10.0))).log_prob(z).sum()
        return -(prior + torch.log_softmax(z, -1)[torch.as_tensor(y[:, 0]).long()].sum())
    z = infr.params.raw(loc).detach().double().cpu().reshape(3).clone().requires_grad_(True)
    want = closed_form(z)
    want.backward()
    loss, loss_for_gradient = infr.create_executor()(yd)
    assert abs(float(loss) - float(want)) <= 1e-9 * abs(float(want)), (float(loss), float(want))
    loss_for_gradient.backward()
    assert nerr(_np(infr.params.grad(loc)).reshape(3), _np(z.grad)) <= 1e-9
    infr.params.zero_grad()
    infr.run(y=yd, max_iter=50, learning_rate=0.05)
    with torch.no_grad():
        after, _ = infr.create_executor()(yd)
    assert float(after) < float(want)


def test_worst_errors_are_printed():
    """the record of a run: worst error and widest bar per family and dtype (the tests above fill the table)"""
    for key in sorted(WORST):
        print('%s %s: worst error %.3g, widest bar %.3g' % (key + WORST[key]))
