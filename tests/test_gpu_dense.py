"""The fused dense layer on the MI355X: mxf_dense_fwd / mxf_dense_bwd (dense.hip) through ops.dense / ops.dense_bwd_.

Expected values are float64 torch on the CPU -- torch.nn.functional.linear plus the activation, autograd under a random cotangent -- never
the code under test.  Inputs are rounded to the dtype under test before either side sees them.  The reverse mode takes Y as an operand: it
is given the reference's Y rounded to the dtype under test.  Errors are normwise per output, |got - want| / max(|want|, tiny).
float64: 1e-9.  float32, per case: max(4 x the error of torch's own float32 CPU evaluation of the same formula on the same inputs,
8 * 2^-24 * M / |want|) with M the norm of the per-element sums of absolute term magnitudes:
  Y      sum_i |x_i w_oi| + |b_o| + |y|   (|act'| <= 1 for all four activations: an error of the sum passes through at most unchanged; the
         activation rounds its own result, |y|)
  G      |dY| t(y) with t the absolute terms of act'(y): 1 (identity), 1 + y^2 (tanh), [y > 0] (relu), |y| + y^2 (sigmoid); the y^2 also
         covers the rounding of the given Y (for tanh d act' = 2 y dy = 2 y^2 ulp)
  dX     sum_o G_o |w_oi|,   dW   sum_n(,s) G_o |x_i|,   db   sum_n(,s) G_o."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64_BAR = 1e-9
EPS32 = 2.0 ** -24
PREFILL = 0.75
WORST = {}          # dtype -> (worst error, widest bar): printed for the record of a run

ACTS = {'identity': lambda z: z, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}

# I, O, N, S, activation, bias (None / 'shared' / 'own'), W ('shared' / 'own'), X ('shared' / 'own' / 'padded': own with a padded leading dimension)
# Widths: the edges of a 16-, 32- and 64-wide tiling, the notebook's 50 and the limit; N: one row, a ragged tile, more than one tile of
# either dtype (16 and 32 rows), many workgroups adding into dW and db.
CASES = (
    (1, 16, 1, 1, 'tanh', 'own', 'own', 'own'),
    (2, 17, 7, 3, 'relu', 'shared', 'shared', 'shared'),
    (3, 50, 33, 3, 'sigmoid', None, 'own', 'padded'),
    (16, 64, 257, 3, 'identity', 'own', 'own', 'shared'),
    (17, 65, 7, 3, 'tanh', 'shared', 'own', 'own'),
    (50, 128, 33, 3, 'relu', 'own', 'shared', 'padded'),
    (64, 1, 257, 1, 'sigmoid', None, 'own', 'own'),
    (65, 2, 1, 3, 'identity', 'own', 'shared', 'shared'),
    (128, 3, 33, 3, 'tanh', 'shared', 'own', 'own'),
    (50, 50, 257, 3, 'tanh', 'own', 'own', 'shared'),
    (128, 128, 33, 3, 'sigmoid', 'own', 'own', 'own'),
    (128, 128, 257, 1, 'relu', 'shared', 'shared', 'padded'),
    (1, 1, 257, 3, 'identity', None, 'shared', 'own'),
    (50, 1, 33, 3, 'identity', 'own', 'own', 'own'),
    (1, 50, 257, 3, 'tanh', 'own', 'own', 'shared'),
)


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


def _sum_to(a, shape):
    for d, n in enumerate(shape):
        if n == 1 and a.shape[d] != 1:
            a = a.sum(axis=d, keepdims=True)
    return a


def reference(X, W, b, act, cot, dtype):
    """[Y (S, N, O), dX like X, dW like W, db like b or None] in torch `dtype` on the CPU"""
    ts = [torch.as_tensor(a, dtype=dtype).requires_grad_(True) for a in (X, W)] + ([torch.as_tensor(b, dtype=dtype).requires_grad_(True)] if b is not None else [])
    S = cot.shape[0]
    pick = lambda t, s: t[s if t.shape[0] > 1 else 0]
    Y = torch.stack([ACTS[act](torch.nn.functional.linear(pick(ts[0], s), pick(ts[1], s), pick(ts[2], s) if b is not None else None)) for s in range(S)], 0)
    g = torch.autograd.grad((Y * torch.as_tensor(cot, dtype=dtype)).sum(), ts)
    return [_np(Y)] + [_np(t) for t in g] + ([None] if b is None else [])


def magnitudes(X, W, b, act, cot, Y):
    S = cot.shape[0]
    Xb, Wb = np.broadcast_to(np.abs(X), (S,) + X.shape[1:]), np.broadcast_to(np.abs(W), (S,) + W.shape[1:])
    mY = np.einsum('sni,soi->sno', Xb, Wb) + (np.abs(b)[:, None, :] if b is not None else 0.0) + np.abs(Y)
    t = {'identity': np.ones_like(Y), 'tanh': 1 + Y * Y, 'relu': (Y > 0).astype(np.float64), 'sigmoid': np.abs(Y) + Y * Y}[act]
    G = np.abs(cot) * t
    mags = [mY, _sum_to(np.einsum('sno,soi->sni', G, Wb), X.shape), _sum_to(np.einsum('sno,sni->soi', G, Xb), W.shape)]
    return mags + [_sum_to(G.sum(1), b.shape) if b is not None else None]


def _bars(dtype, want, own32, mags):
    tiny = np.finfo(np.float64).tiny
    floor = lambda w, m, eps: 8 * eps * float(np.linalg.norm(m)) / max(float(np.linalg.norm(w)), tiny)
    if dtype == 'float64':
        return [None if w is None else max(F64_BAR, floor(w, m, 2.0 ** -53)) for w, m in zip(want, mags)]
    return [None if w is None else max(4 * nerr(o, w), floor(w, m, EPS32)) for o, w, m in zip(own32, want, mags)]


@functools.lru_cache(maxsize=None)
def case(dtype, I, O, N, S, act, bias, w, x, scale=1.0):
    r = np.random.RandomState(I + 131 * O + 17 * N + S + len(act))
    X = _round(r.uniform(-1.0, 1.0, (1 if x == 'shared' else S, N, I)), dtype)
    W = _round(scale * r.uniform(-1.0, 1.0, (1 if w == 'shared' else S, O, I)) / np.sqrt(I), dtype)
    b = None if bias is None else _round(r.uniform(-0.5, 0.5, (1 if bias == 'shared' else S, O)), dtype)
    cot = _round(r.uniform(-1.0, 1.0, (S, N, O)), dtype)
    want = reference(X, W, b, act, cot, torch.float64)
    own32 = reference(X, W, b, act, cot, torch.float32) if dtype == 'float32' else None
    return (X, W, b, cot), want, _bars(dtype, want, own32, magnitudes(X, W, b, act, cot, want[0]))


def _x_dev(X, x, dtype):
    if x != 'padded':
        return _dev(X, dtype)
    buf = torch.full(X.shape[:2] + (X.shape[2] + 5,), float('nan'), dtype=_tdt(dtype), device='cuda')
    buf[:, :, :X.shape[2]] = _dev(X, dtype)
    return buf[:, :, :X.shape[2]]


def _record(dtype, what, names, got, want, bars):
    trip = [(n, g, w, b) for n, g, w, b in zip(names, got, want, bars) if w is not None]
    errs = [nerr(g, w) for _, g, w, _ in trip]
    worst = WORST.get(dtype, (0.0, 0.0))
    WORST[dtype] = (max([worst[0]] + errs), max([worst[1]] + [b for _, _, _, b in trip]))
    print('dense %s %s: %s; worst so far %.3g, widest bar %.3g'
          % (dtype, what, ', '.join('%s %.3g (bar %.3g)' % (t[0], e, t[3]) for t, e in zip(trip, errs)), *WORST[dtype]))
    for (name, g, w, bar), e in zip(trip, errs):
        assert np.asarray(g).shape == np.asarray(w).shape, (name, np.asarray(g).shape, np.asarray(w).shape)
        assert e <= bar, (what, name, e, bar)


def run_case(dtype, I, O, N, S, act, bias, w, x, prefill=0.0, skip=(), scale=1.0):
    """forward through ops.dense, reverse through ops.dense_bwd_ on accumulators prefilled with `prefill`; outputs in `skip` are passed null"""
    from mxfusion_amd import ops
    (X, W, b, cot), want, bars = case(dtype, I, O, N, S, act, bias, w, x, scale)
    Xd, Wd, bd = _x_dev(X, x, dtype), _dev(W, dtype), None if b is None else _dev(b, dtype)
    Y = ops.dense(Xd, Wd, bd, act)
    acc = lambda a, name: None if a is None or name in skip else torch.full(a.shape, prefill, dtype=_tdt(dtype), device='cuda')
    dX, dW, db = acc(X, 'dX'), acc(W, 'dW'), acc(b, 'db')
    ops.dense_bwd_(Xd, Wd, _dev(_round(want[0], dtype), dtype), _dev(cot, dtype), act, dX, dW, db)
    torch.cuda.synchronize()
    Yg = _np(Y)
    if all(t is None or t.shape[0] == 1 for t in (X, W, b)):      # nothing carries the sample axis: one block stands for all S
        assert Yg.shape == (1, N, O)
        Yg = np.broadcast_to(Yg, (S, N, O))
    got = [Yg] + [None if g is None else _np(g) - prefill for g in (dX, dW, db)]
    keep = [True] + [g is not None for g in got[1:]]
    _record(dtype, 'I=%d O=%d N=%d S=%d %s b=%s W=%s X=%s' % (I, O, N, S, act, bias, w, x), ('Y', 'dX', 'dW', 'db'),
            got, [wv if k else None for wv, k in zip(want, keep)], bars)
    return got


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('I,O,N,S,act,bias,w,x', CASES)
def test_dense_forward_and_reverse(dtype, I, O, N, S, act, bias, w, x):
    run_case(dtype, I, O, N, S, act, bias, w, x)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_dense_writes_y_and_accumulates_gradients(dtype):
    """Y is written over a prefilled buffer (the raw entry point on the caller's buffer); the gradients are added to prefilled ones"""
    from mxfusion_amd import _lib, ops
    I, O, N, S, act = 17, 50, 33, 3, 'tanh'
    run_case(dtype, I, O, N, S, act, 'own', 'own', 'own', prefill=PREFILL)
    run_case(dtype, I, O, N, S, act, 'shared', 'shared', 'shared', prefill=PREFILL)
    (X, W, b, cot), want, bars = case(dtype, I, O, N, S, act, 'own', 'own', 'own')
    Xd, Wd, bd = _dev(X, dtype), _dev(W, dtype), _dev(b, dtype)
    Y = torch.full((S, N, O), PREFILL, dtype=_tdt(dtype), device='cuda')
    _lib.call('mxf_dense_fwd', ops._h(Xd), ops._dt(Xd), S, N, I, O, _lib.ACT_TANH, Xd.data_ptr(), I, N * I, Wd.data_ptr(), O * I,
              bd.data_ptr(), O, Y.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    _record(dtype, 'prefilled Y', ('Y',), [_np(Y)], want[:1], bars[:1])


@pytest.mark.parametrize('skip', [('dX',), ('dW',), ('db',), ('dX', 'db'), ('dW', 'db')])
def test_dense_null_output_is_skipped(skip):
    for dtype in ('float64', 'float32'):
        run_case(dtype, 17, 50, 33, 3, 'tanh', 'own', 'shared', 'shared', skip=skip)


def test_dense_width_129_is_status_minus_3():
    from mxfusion_amd import _lib, ops
    x = torch.zeros(1, 2, 129, dtype=torch.float32, device='cuda')
    w = torch.zeros(1, 3, 129, dtype=torch.float32, device='cuda')
    y = torch.zeros(1, 2, 3, dtype=torch.float32, device='cuda')
    lib, h = _lib.load(), ops._h(x)
    vp = ctypes.c_void_p
    assert lib.mxf_dense_fwd(h, _lib.F32, 1, 2, 129, 3, 0, vp(x.data_ptr()), 129, 0, vp(w.data_ptr()), 0, None, 0, vp(y.data_ptr()), None) == -3
    assert lib.mxf_dense_fwd(h, _lib.F32, 1, 2, 3, 129, 0, vp(x.data_ptr()), 129, 0, vp(w.data_ptr()), 0, None, 0, vp(y.data_ptr()), None) == -3
    assert lib.mxf_dense_bwd(h, _lib.F32, 1, 2, 129, 3, 0, vp(x.data_ptr()), 129, 0, vp(w.data_ptr()), 0, 0, vp(y.data_ptr()), vp(y.data_ptr()),
                             None, vp(w.data_ptr()), None, None) == -3
    assert b'129' in lib.mxf_last_error(h)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('I,O,w,x', [(129, 3, 'own', 'shared'), (5, 130, 'shared', 'own')])
def test_dense_fallback_beyond_the_widths(dtype, I, O, w, x):
    """the wrapper's route through gemm and elementwise torch, to the same bars"""
    run_case(dtype, I, O, 33, 3, 'tanh', 'shared', w, x)


def test_dense_rejects_bad_operands():
    from mxfusion_amd import _lib, ops
    x = torch.zeros(1, 2, 4, dtype=torch.float32, device='cuda')
    w = torch.zeros(1, 3, 4, dtype=torch.float32, device='cuda')
    y = torch.zeros(1, 2, 3, dtype=torch.float32, device='cuda')
    lib, h = _lib.load(), ops._h(x)
    vp = ctypes.c_void_p
    assert lib.mxf_dense_fwd(h, _lib.F32, 1, 2, 4, 3, 7, vp(x.data_ptr()), 4, 0, vp(w.data_ptr()), 0, None, 0, vp(y.data_ptr()), None) == -2      # activation
    assert lib.mxf_dense_fwd(h, _lib.F32, 1, 2, 4, 3, 0, vp(x.data_ptr()), 3, 0, vp(w.data_ptr()), 0, None, 0, vp(y.data_ptr()), None) == -2      # ldx < I
    assert lib.mxf_dense_fwd(h, _lib.F32, 2, 2, 4, 3, 0, vp(x.data_ptr()), 4, 0, vp(w.data_ptr()), 5, None, 0, vp(y.data_ptr()), None) == -2      # W's stride
    assert lib.mxf_dense_fwd(h, 9, 1, 2, 4, 3, 0, vp(x.data_ptr()), 4, 0, vp(w.data_ptr()), 0, None, 0, vp(y.data_ptr()), None) == -2             # dtype
    assert lib.mxf_dense_fwd(h, _lib.F32, 0, 2, 4, 3, 0, None, 4, 0, None, 0, None, 0, None, None) == 0                                           # nothing to do
    with pytest.raises(ValueError):
        ops.dense(x, torch.zeros(1, 3, 5, dtype=torch.float32, device='cuda'))
    with pytest.raises(TypeError):
        ops.dense(x, w.double())
