"""GPU tests of the difference-form Gram pass and its reverse mode (mxf_gram_diff / mxf_gram_diff_bwd; csrc/gram_diff.hip) against the
float64 restatement tests/_gram_diff_ref.py on the dtype-rounded operands.

Shapes come from the kernels' own tiles (csrc/gram_diff_plan.h): a workgroup owns 256 columns (one per lane) and a band of 64 rows (the
reverse pass: a multiple of 64, which the plan brings down to 64 at these sizes), so the extents are 1, one below / at / above a row tile
(63, 64, 65) and a column tile (255, 256, 257), and 300 = the most the issue allows (two column tiles, five bands); Q runs over the
coordinate tiles' ends 1, 3 (tile 4), 16 (8 for SpectralMixture) and A over 1, 3, 8.

Bars: |error| <= C eps amp T with T the output's own sum of absolute terms from the restatement (forward: the sum over the mixture
components of |w_a k_a|, which is |k| for Periodic and RQ), amp = 1 + the case's largest phase or exponent argument
(_gram_diff_ref.amplification), eps = 2^-24 / 2^-53, and C the next power of two at or above four times the worst ratio measured on an
MI355X over the cases of this file:
    worst ratio      periodic   rq      sm      4 x worst   C
    float32 forward  4.01       2.41    7.78    31.1        32
    float64 forward  4.49       2.56    5.49    22.0        32
    float32 reverse  4.67       4.86    2.63    19.4        32
    float64 reverse  6.53       3.20    2.45    26.1        32
T is the ENVELOPE of the terms where they carry a sine or cosine (_gram_diff_ref.gram, majorant): a phase rounded by eps |phase| moves a
sine or cosine by that much absolutely, however close to zero it is.  With the terms themselves as T the outputs that are one pair, or a
short sum of pairs, next to such a zero measured 2e4 (forward SpectralMixture) and 185 to 927 (reverse Periodic and SpectralMixture at
1 x 300, 300 x 1 and Q = 8, A = 1) in float32 and float64 alike -- far beyond "a few hundred", i.e. the form was wrong, not the constant.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import _gram_diff_ref as R

pytestmark = pytest.mark.gpu

C_FWD = {torch.float32: 32.0, torch.float64: 32.0}
C_BWD = {torch.float32: 32.0, torch.float64: 32.0}
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
OPS = ('X', 'X2', 'p0', 'p1', 'p2')


def _params(kind, rng, Q, A, ard):
    n = Q if ard else 1
    if kind == 'sm':
        return rng.uniform(0.3, 1.0, A), rng.uniform(0.05, 0.6, (A, Q)), rng.uniform(0.05, 0.4, (A, Q))
    return rng.uniform(0.5, 1.5, 1), rng.uniform(0.8, 1.8, n), (rng.uniform(0.7, 2.5, n) if kind == 'periodic' else rng.uniform(0.5, 3.0, 1))


@functools.lru_cache(maxsize=None)
def make(kind, N, N2, Q, A, ard, S, shared, f32, offset=0.0, seed=0):
    """float64 CPU operands (already rounded to the run's dtype) of one call: {name: (S|1, ...)}, and dK (S, N, N2).  `shared`: the operands
    with a unit sample axis; N2 None: square."""
    rng = np.random.default_rng(seed + 1000 * N + (N2 or 0))
    rnd = (lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32).astype(np.float64))) if f32 else (lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)))
    n = lambda name: 1 if name in shared else S
    ops = {'X': rnd(rng.uniform(-2, 2, (n('X'), N, Q)) + offset), 'X2': None if N2 is None else rnd(rng.uniform(-2, 2, (n('X2'), N2, Q)) + offset)}
    for i, name in enumerate(('p0', 'p1', 'p2')):
        ops[name] = rnd(np.stack([_params(kind, rng, Q, A, ard)[i] for _ in range(n(name))]))
    return ops, rnd(rng.standard_normal((S, N, N2 or N)))


@functools.lru_cache(maxsize=None)
def reference(*key):
    """per call: K (S, N, N2), its T, {name: (gradient, T)} shaped like the operands (summed over the samples where shared), amp"""
    kind, S = key[0], key[6]
    ops, dK = make(*key)
    at = lambda t, s: None if t is None else t[s if t.shape[0] > 1 else 0]
    Ks, Ts, amp = [], [], 1.0
    grads = {n: [torch.zeros_like(t), torch.zeros_like(t)] for n, t in ops.items() if t is not None}
    for s in range(S):
        a = [at(ops[n], s) for n in OPS]
        K, T = R.gram(kind, *a)
        Ks.append(K), Ts.append(T)
        amp = max(amp, R.amplification(kind, *a))
        for n, (g, t) in R.grads(kind, *a, dK[s]).items():
            i = s if ops[n].shape[0] > 1 else 0
            grads[n][0][i] += g
            grads[n][1][i] += t
    return torch.stack(Ks), torch.stack(Ts), grads, amp


def dev(t, dtype):
    return None if t is None else t.to(dtype).cuda()


def ratio(got, ref, T, eps, amp):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all())
    err, bar = (got - ref).abs(), eps * amp * T
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(r.max())


def note(what, kind, dtype, r):
    print('ratio', what, kind, str(dtype).split('.')[-1], '%.3f' % r)


SHAPES = [(1, 1), (63, 255), (64, 256), (65, 257), (1, 300), (300, 1), (130, None), (65, None), (1, None)]
CASES = [(k, N, N2, 3, 3 if k == 'sm' else 1, True, 1, frozenset()) for k in R.KINDS for N, N2 in SHAPES]
CASES += [(k, 65, 257, Q, 1, ard, 1, frozenset()) for k in ('periodic', 'rq') for Q in (1, 16) for ard in (True, False)]
CASES += [(k, 65, None, 3, 1, False, 1, frozenset()) for k in ('periodic', 'rq')]
CASES += [('sm', 65, 257, Q, A, True, 1, frozenset()) for Q, A in ((1, 1), (1, 8), (8, 1), (8, 8), (3, 8))]
CASES += [(k, 65, N2, 3, 3 if k == 'sm' else 1, True, 3, frozenset(sh)) for k in R.KINDS for N2 in (70, None)
          for sh in ((), ('X',), ('X2',), ('p0',), ('p1',), ('p2',), ('X', 'X2'), ('p0', 'p1', 'p2')) if N2 is not None or 'X2' not in sh]
DTYPES = (torch.float32, torch.float64)
cid = lambda c: '%s-%dx%s-Q%d-A%d-%s-S%d-%s' % (c[0], c[1], c[2], c[3], c[4], 'ard' if c[5] else 'iso', c[6], '+'.join(sorted(c[7])) or 'none')


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
@pytest.mark.parametrize('case', CASES, ids=cid)
def test_forward(case, dtype):
    from mxfusion_amd import ops as mops
    kind, N, N2, Q, A, ard, S, shared = case
    key = case + (dtype == torch.float32,)
    o, _ = make(*key)
    Kref, T, _, amp = reference(*key)
    K = mops.gram_diff(kind, *(dev(o[n], dtype) for n in OPS), ard)
    assert K.shape == (S, N, N2 or N)
    r = ratio(K, Kref, T, EPS[dtype], amp)
    note('fwd', kind, dtype, r)
    assert r <= C_FWD[dtype]
    if N2 is None:
        assert torch.equal(K, K.transpose(-1, -2))
        p0 = dev(o['p0'], dtype)
        kd = p0[..., 0]
        for a in range(1, p0.shape[-1]):
            kd = kd + p0[..., a]
        assert torch.equal(torch.diagonal(K, dim1=-2, dim2=-1), kd[:, None].expand(S, N))


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
@pytest.mark.parametrize('case', CASES, ids=cid)
def test_reverse(case, dtype):
    from mxfusion_amd import ops as mops
    kind, N, N2, Q, A, ard, S, shared = case
    key = case + (dtype == torch.float32,)
    o, dK = make(*key)
    _, _, gref, amp = reference(*key)
    got = dict(zip(OPS, mops.gram_diff_bwd(kind, *(dev(o[n], dtype) for n in OPS), ard, dev(dK, dtype))))
    assert (got['X2'] is None) == (N2 is None)
    for n, (g, T) in gref.items():
        assert got[n].shape == o[n].shape
        r = ratio(got[n], g, T, EPS[dtype], amp)
        note('bwd', kind, dtype, r)
        assert r <= C_BWD[dtype], n


# ---- the output contract ---------------------------------------------------------------------------------------------------------------------
SMALL = {k: (k, 65, 70, 3, 3 if k == 'sm' else 1, True, 1, frozenset()) for k in R.KINDS}


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
@pytest.mark.parametrize('kind', R.KINDS)
def test_diagonal_terms_and_padded_output(kind, dtype):
    from mxfusion_amd import ops as mops
    c = (kind, 65, None, 3, 3 if kind == 'sm' else 1, True, 3, frozenset(('p0', 'p1', 'p2'))) + (dtype == torch.float32,)
    o, _ = make(*c)
    a = [dev(o[n], dtype) for n in OPS]
    K0 = mops.gram_diff(kind, *a, True)
    diag = torch.tensor([[0.25], [0.5], [0.125]], dtype=dtype, device='cuda')
    K1 = mops.gram_diff(kind, *a, True, diag_add=diag, jitter=1e-3)
    eye = torch.eye(65, dtype=torch.bool, device='cuda')
    assert torch.equal(K1[:, ~eye], K0[:, ~eye])
    d0, d1 = torch.diagonal(K0, dim1=-2, dim2=-1), torch.diagonal(K1, dim1=-2, dim2=-1)
    want = d0.double() + diag.double() + 1e-3
    assert float(((d1.double() - want).abs() / want).max()) <= 2 * EPS[dtype]            # one rounding of diag + jitter, one of the sum
    buf = torch.full((3, 65, 80), -7.0, dtype=dtype, device='cuda')
    out = mops.gram_diff(kind, *a, True, out=buf[:, :, :65])
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf[:, :, :65], K0) and bool((buf[:, :, 65:] == -7.0).all())


def _raw_bwd(kind, a, ard, dK, bufs, A):
    from mxfusion_amd import _lib, ops as mops
    X, X2, p0, p1, p2 = a
    N2 = X.shape[-2] if X2 is None else X2.shape[-2]
    p, ss = mops._p, mops._ss
    return _lib.load().mxf_gram_diff_bwd(mops._h(X), mops.KIND_DIFF[kind], mops._dt(X), dK.shape[0], X.shape[-2], N2, X.shape[-1], A, p(X), ss(X), p(X2), ss(X2),
                                         p(p0), ss(p0), p(p1), ss(p1), p(p2), ss(p2), int(ard), p(dK), dK.stride(-2), dK.stride(0), *(p(b) for b in bufs), mops._stream())


@pytest.mark.parametrize('kind', R.KINDS)
def test_every_subset_of_need_and_accumulate_into(kind):
    """an absent output changes no other output (to the reordering of the atomic sums: 64 eps of the output's absolute sum); pre-filled
    buffers receive their pre-fill plus the gradient"""
    from mxfusion_amd import ops as mops
    dtype = torch.float64
    c = SMALL[kind] + (False,)
    o, dK = make(*c)
    _, _, gref, _ = reference(*c)
    a, g = [dev(o[n], dtype) for n in OPS], dev(dK, dtype)
    full = dict(zip(OPS, mops.gram_diff_bwd(kind, *a, True, g)))
    for k in range(len(OPS) + 1):
        for need in itertools.combinations(OPS, k):
            got = dict(zip(OPS, mops.gram_diff_bwd(kind, *a, True, g, need=need)))
            for n in OPS:
                assert (got[n] is None) == (n not in need), (need, n)
                if n in need:
                    assert bool(((got[n] - full[n]).abs().cpu() <= 64 * EPS[dtype] * gref[n][1]).all()), (need, n)
    bufs = [torch.full_like(t, 3.0) for t in a]
    assert _raw_bwd(kind, a, True, g, bufs, c[4]) == 0
    for n, b in zip(OPS, bufs):
        assert bool(((b - 3.0 - full[n]).abs().cpu() <= 64 * EPS[dtype] * (gref[n][1] + 3.0)).all()), n


@pytest.mark.parametrize('dtype', DTYPES, ids=('f32', 'f64'))
@pytest.mark.parametrize('kind', R.KINDS)
def test_duplicated_rows_and_offset_inputs(kind, dtype):
    """coincident rows (tau = 0 exactly) give finite gradients; inputs 1000 units away give the errors of centred inputs, within the same
    bars: the differences are taken first"""
    from mxfusion_amd import ops as mops
    f32 = dtype == torch.float32
    base = (kind, 65, None, 3, 3 if kind == 'sm' else 1, True, 1, frozenset())
    o, dK = make(*base, f32)
    X = o['X'].clone()
    X[:, 1::2] = X[:, 0::2][:, :X[:, 1::2].shape[1]]
    got = mops.gram_diff_bwd(kind, dev(X, dtype), None, *(dev(o[n], dtype) for n in OPS[2:]), True, dev(dK, dtype))
    assert all(t is None or bool(torch.isfinite(t).all()) for t in got)
    for off in (0.0, 1000.0):
        key = (kind, 65, 70, 3, base[4], True, 1, frozenset(), f32, off)
        o, dK = make(*key)
        Kref, T, gref, amp = reference(*key)
        a = [dev(o[n], dtype) for n in OPS]
        r = ratio(mops.gram_diff(kind, *a, True), Kref, T, EPS[dtype], amp)
        note('fwd@%g' % off, kind, dtype, r)
        assert r <= C_FWD[dtype]
        for n, t in zip(OPS, mops.gram_diff_bwd(kind, *a, True, dev(dK, dtype))):
            r = ratio(t, gref[n][0], gref[n][1], EPS[dtype], amp)
            note('bwd@%g' % off, kind, dtype, r)
            assert r <= C_BWD[dtype], (off, n)


def test_status_codes_leave_the_buffers_alone():
    from mxfusion_amd import _lib, ops as mops
    dt = torch.float32
    for kind, Q, A, code in (('periodic', 17, 1, -3), ('rq', 17, 1, -3), ('sm', 9, 2, -3), ('sm', 2, 9, -3)):
        X = torch.zeros(1, 5, Q, dtype=dt, device='cuda')
        shp = ((1, A), (1, A, Q), (1, A, Q)) if kind == 'sm' else ((1, 1), (1, Q), (1, Q if kind == 'periodic' else 1))
        ps = [torch.ones(s, dtype=dt, device='cuda') for s in shp]
        out = torch.full((1, 5, 5), -7.0, dtype=dt, device='cuda')
        with pytest.raises(_lib.MXFError, match=r'\(%d\).*limit' % code):
            mops.gram_diff(kind, X, None, *ps, True, out=out)
        bufs = [torch.full_like(t, -7.0) for t in (X, X, *ps)]
        assert _raw_bwd(kind, (X, None, *ps), True, torch.ones(1, 5, 5, dtype=dt, device='cuda'), bufs, A) == code
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and all(bool((b == -7.0).all()) for b in bufs)
    X, one = torch.zeros(1, 5, 2, dtype=dt, device='cuda'), torch.ones(1, 1, dtype=dt, device='cuda')
    out = torch.full((1, 5, 5), -7.0, dtype=dt, device='cuda')
    h, st = mops._h(X), mops._stream()
    rc = _lib.load().mxf_gram_diff(h, 0, 0, 1, 5, 5, 2, 1, None, 0, None, 0, one.data_ptr(), 0, one.data_ptr(), 0, one.data_ptr(), 0, 0, None, 0, 0.0,
                                   out.data_ptr(), 5, 25, st)
    assert rc == -2 and bool((out == -7.0).all())
    assert _raw_bwd('rq', (X, None, one, one, one), False, torch.ones(1, 5, 5, dtype=dt, device='cuda'), [None] * 5, 1) == 0      # nothing asked for
