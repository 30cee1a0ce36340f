"""The model operators on the MI355X: the broadcast map (ops.ewise / ops.ewise_bwd_), the reductions (ops.reduce / ops.reduce_bwd_), the raw
ABI's refusals, the sixteen operators through factor.eval, and a model written with them under stochastic variational inference.

Expected values are float64 torch / numpy on the CPU, never the code under test; inputs are rounded to the dtype under test before either
side sees them; errors are normwise per output.  float64: 1e-9.  float32: max(4 x the error of torch's own float32 CPU evaluation of the
same formula on the same inputs, 8 * 2^-24 * |M| / |want|), M the per-element sum of the absolute magnitudes of the terms that make up the
element:
  map, forward      |x| + |y| for add and subtract, |z| for the others (one term);
  map, reverse      the buffers are prefilled with 0.75 and the output is prefill + gradient: M = 0.75 + the sum over the operand's shared
                    axes of |t|, t the term of the table -- dz; dz y and dz x; dz / y and dz x / y^2; dz y x^(y-1) and dz x^y log x; 2 x dz;
                    dz exp x; dz / x.  For the dy of multiply under a one-element y that is 0.75 + the sum of |dz| |x| over all 25 443 terms;
  sum, mean         the sum over the reduced axes of |x| (mean: / R);   prod: |prod| (one term);
  reductions, reverse   0.75 + |gradient| (one term per element).
Each test prints its worst error against its bar, and the widest bar, for the record."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64_BAR = 1e-9
EPS32 = 2.0 ** -24
PREFILL = 0.75
OPS = ['add', 'subtract', 'multiply', 'divide', 'power', 'square', 'exp', 'log']
BINARY = OPS[:5]


def _tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def _round(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64))


def _norm(a):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64)))


def nerr(got, want):
    return _norm(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / max(_norm(want), np.finfo(np.float64).tiny)


def bar(dtype, want, cpu32, M):
    if dtype == 'float64':
        return F64_BAR
    return max(4 * nerr(cpu32, want), 8 * EPS32 * _norm(M) / max(_norm(want), np.finfo(np.float64).tiny))


class Record(object):
    """the worst error relative to its bar, and the widest bar, of one test"""

    def __init__(self, what):
        self.what, self.worst, self.widest = what, (0.0, 0.0, 1.0, ''), 0.0

    def check(self, label, dtype, got, want, cpu32, M):
        got = got.detach().double().cpu().numpy()
        want = want.detach().numpy()
        assert got.shape == want.shape, (self.what, label, got.shape, want.shape)
        e, b = nerr(got, want), bar(dtype, want, None if cpu32 is None else cpu32.detach().double().numpy(), M.detach().numpy())
        if e / b >= self.worst[0]:
            self.worst = (e / b, e, b, label)
        self.widest = max(self.widest, b)
        assert e <= b, (self.what, label, e, b)

    def done(self):
        print('%s: worst error %.3g (bar %.3g) at %s; widest bar %.3g' % (self.what, self.worst[1], self.worst[2], self.worst[3], self.widest))


def sum_to(t, shape):
    return t.sum_to_size(tuple(shape)) if tuple(t.shape) != tuple(shape) else t


def map_inputs(op, xs, ys, dtype, seed=0):
    """x, y (None for the elementwise ops) and the cotangent, float64 CPU tensors holding values of `dtype`, in the tested domains"""
    r = np.random.RandomState(seed + 31 * OPS.index(op))
    pos = lambda s: r.uniform(0.5, 2.0, s)
    x = pos(xs) if op in ('power', 'log') else r.randn(*xs)
    y = None if op not in BINARY else pos(ys) if op == 'divide' else r.uniform(-2, 2, ys) if op == 'power' else r.randn(*ys)
    shape = np.broadcast_shapes(xs, ys) if y is not None else xs
    return _round(x, dtype), None if y is None else _round(y, dtype), _round(r.randn(*shape), dtype)


def map_formulas(op, x, y, dz):
    """z and the terms of dx and dy over the full output shape, in the dtype of the arguments (torch on the CPU)"""
    z = {'add': lambda: x + y, 'subtract': lambda: x - y, 'multiply': lambda: x * y, 'divide': lambda: x / y, 'power': lambda: torch.pow(x, y),
         'square': lambda: x * x, 'exp': lambda: torch.exp(x), 'log': lambda: torch.log(x)}[op]()
    tx, ty = {'add': lambda: (dz, dz), 'subtract': lambda: (dz, -dz), 'multiply': lambda: (dz * y, dz * x),
              'divide': lambda: (dz / y, -dz * x / (y * y)),
              'power': lambda: (dz * y * torch.pow(x, y - 1), dz * torch.pow(x, y) * torch.log(x)),
              'square': lambda: (2 * x * dz, None), 'exp': lambda: (dz * torch.exp(x), None), 'log': lambda: (dz / x, None)}[op]()
    full = lambda t: None if t is None else t.expand(dz.shape)
    return z, full(tx), full(ty)


def check_map(rec, label, op, dtype, xd, yd, x, y, dz, want_dx=True, want_dy=True):
    """ops.ewise and ops.ewise_bwd_ on the device operands xd, yd (views of any layout holding the values of x, y) against the formulas"""
    from mxfusion_amd import ops
    f32 = lambda t: None if t is None else t.float()
    z, tx, ty = map_formulas(op, x, y, dz)
    z32, tx32, ty32 = map_formulas(op, f32(x), f32(y), f32(dz))
    got = ops.ewise(op, xd, yd)
    Mz = x.abs() + y.abs() if op in ('add', 'subtract') else z.abs()
    rec.check('%s %s z' % (label, op), dtype, got, z, z32, Mz.expand(z.shape))
    dzd = dz.to(_tdt(dtype)).cuda()
    xo, yo = ops.ewise_operands(xd, yd)
    accs = [torch.full(tuple(t.shape), PREFILL, dtype=_tdt(dtype), device='cuda') if t is not None and w else None
            for t, w in ((xo, want_dx), (yo, want_dy))]
    ops.ewise_bwd_(op, xd, yd, dzd, *accs)
    torch.cuda.synchronize()
    for name, acc, t, t32 in (('dx', accs[0], tx, tx32), ('dy', accs[1], ty, ty32)):
        if acc is None:
            continue
        want = PREFILL + sum_to(t, acc.shape)
        rec.check('%s %s %s' % (label, op, name), dtype, acc, want, (PREFILL + sum_to(t32, acc.shape)), PREFILL + sum_to(t.abs(), acc.shape))
    return got, accs


def dev(t, dtype):
    return None if t is None else t.to(_tdt(dtype)).cuda()


CASES = {
    'inner 1': ((2, 3, 1), (1, 3, 1)), 'inner 3': ((2, 3, 3), (1, 1, 3)), 'inner 4': ((2, 3, 4), (1, 1, 4)), 'inner 5': ((2, 3, 5), (1, 1, 5)),
    'inner 8 + 3': ((2, 3, 11), (1, 1, 11)), 'inner 8 + 3, columns': ((2, 3, 11), (2, 3, 1)),
    'same shape': ((3, 7, 5), (3, 7, 5)),
    'x shared over samples': ((1, 7, 5), (3, 7, 5)),
    'one-element operand': ((3, 257, 33), (1, 1, 1)),
    'row vector': ((3, 33, 5), (1, 1, 5)),
    'column vector': ((3, 33, 5), (3, 33, 1)),
    'outer product': ((3, 33, 1), (1, 1, 5)),
    'rank 5 after merging': ((2, 3, 1, 4, 1, 5), (1, 1, 2, 1, 3, 5)),
    'lower rank': ((3, 33, 5), (1, 5)),
    # a per-row operand: shared over the samples AND over the innermost axis, dense between -- its destinations repeat with the samples,
    # so one destination comes back in several separate runs of lanes within a wave (float32: 2, 3 chunks a row; float64: 4, 5)
    'per-row scale, 4 rows of 8': ((1, 4, 1), (3, 4, 8)),
    'per-row scale, 5 rows of 9': ((1, 5, 1), (3, 5, 9)),
    'per-row scale, 5 rows of 12': ((3, 5, 12), (1, 5, 1)),
    'per-row scale, four axes': ((1, 1, 3, 1), (2, 3, 3, 5)),
    'per-row scale, four axes, many samples': ((7, 5, 2, 6), (1, 1, 2, 1)),
}


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_map_forward_and_reverse(case, dtype):
    from mxfusion_amd import ops
    xs, ys = CASES[case]
    rec = Record('map, %s, %s' % (case, dtype))
    for op in OPS:
        x, y, dz = map_inputs(op, xs, ys, dtype)
        yy = y if y is None or y.dim() == x.dim() else y.reshape((y.shape[0],) + (1,) * (x.dim() - y.dim()) + tuple(y.shape[1:]))
        assert ops.ewise_fits(dev(x, dtype), dev(y, dtype))
        check_map(rec, case, op, dtype, dev(x, dtype), dev(y, dtype), x, yy, dz)
    rec.done()


def test_rank_five_is_what_the_merged_case_reaches_the_kernel_with(monkeypatch):
    """(2, 3, 1, 4, 1, 5) op (1, 1, 2, 1, 3, 5): the two leading axes merge (x dense, y shared over the run), nothing else does: five
    axes, the most the kernel takes, and it takes them"""
    from mxfusion_amd import ops, _lib
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, h, *a: (seen.append((name, a)), real(name, h, *a))[1])
    xs, ys = CASES['rank 5 after merging']
    ops.ewise('add', torch.zeros(xs, device='cuda'), torch.zeros(ys, device='cuda'))
    (name, a), = seen
    assert name == 'mxf_ewise_fwd' and a[2] == 5 and list(a[3]) == [6, 2, 4, 3, 5] and list(a[5]) == [20, 0, 5, 0, 1] and list(a[7]) == [0, 15, 0, 5, 1]


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_more_than_five_axes_go_through_torch(dtype, monkeypatch):
    """six axes that do not merge: mxf_ewise_* would answer -3 (test_raw_abi_refusals), so the wrapper routes the map to the torch expression"""
    from mxfusion_amd import ops, _lib
    xs, ys = (2, 1, 2, 1, 2, 3), (1, 2, 1, 2, 1, 3)
    rec = Record('map routed to torch, %s' % dtype)
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, h, *a: pytest.fail('the kernel was called') if name.startswith('mxf_ewise') else real(name, h, *a))
    for op in OPS:
        x, y, dz = map_inputs(op, xs, ys, dtype)
        if y is not None:
            assert not ops.ewise_fits(dev(x, dtype), dev(y, dtype))
            check_map(rec, 'six axes', op, dtype, dev(x, dtype), dev(y, dtype), x, y, dz)
    rec.done()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_operand_layouts_reach_the_kernel_as_they_are(dtype, monkeypatch):
    """an expanded view out of broadcast_to, a transposed view and an operand that starts off a 16-byte boundary: no copy is made -- the
    address the kernel receives is the view's own -- and the values are right"""
    from mxfusion_amd import ops, _lib, Variable
    from mxfusion_amd.components.functions.operators import broadcast_to
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, h, *a: (seen.append((name, a)), real(name, h, *a))[1])
    rec = Record('map, operand layouts, %s' % dtype)
    for op in OPS:
        x, y, dz = map_inputs(op, (3, 33, 5), (1, 1, 5), dtype)
        # y through broadcast_to: (1, 1, 5) -> (1, 33, 5), stride 0 along the rows
        src = Variable(shape=(1, 5))
        base = dev(y if y is not None else x[:1, :1], dtype)
        yd = broadcast_to(src, (33, 5)).factor.eval(torch, {src.uuid: base})
        assert tuple(yd.shape) == (1, 33, 5) and yd.stride(1) == 0 and yd.data_ptr() == base.data_ptr()
        # x as a transposed view of a (3, 5, 33) array, starting one element into its buffer
        buf = torch.zeros(3 * 5 * 33 + 1, dtype=_tdt(dtype), device='cuda')
        xd = buf[1:].view(3, 5, 33).transpose(1, 2)
        xd.copy_(dev(x, dtype))
        assert not xd.is_contiguous() and xd.data_ptr() % 16 == buf.element_size()
        del seen[:]
        if y is None:
            check_map(rec, 'views', op, dtype, xd, None, x, None, dz)
        else:
            check_map(rec, 'views', op, dtype, xd, yd, x, y, dz)
        calls = [(n, a) for n, a in seen if n.startswith('mxf_ewise')]
        assert [n for n, _ in calls] == ['mxf_ewise_fwd', 'mxf_ewise_bwd']
        for n, a in calls:
            assert a[4] == xd.data_ptr() and list(a[5])[-2:] == [1, 33], (n, list(a[5]))
            if y is not None:
                assert a[6] == base.data_ptr() and list(a[3]) == [3, 33, 5] and list(a[7]) == [0, 0, 1], (n, list(a[3]), list(a[7]))
        # the odd start alone, on contiguous operands of one shape: the whole map is one row that begins 4 (8) bytes off
        x, y, dz = map_inputs(op, (3, 7, 5), (3, 7, 5), dtype, seed=5)
        buf = torch.zeros(3 * 7 * 5 + 1, dtype=_tdt(dtype), device='cuda')
        xd = buf[1:].view(3, 7, 5)
        xd.copy_(dev(x, dtype))
        check_map(rec, 'odd start', op, dtype, xd, dev(y, dtype), x, y, dz)
    rec.done()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_null_outputs_leave_the_other_right(dtype):
    rec = Record('map, null outputs, %s' % dtype)
    for case in ('row vector', 'one-element operand', 'x shared over samples'):
        xs, ys = CASES[case]
        for op in BINARY:
            x, y, dz = map_inputs(op, xs, ys, dtype, seed=9)
            _, accs = check_map(rec, case + ', no dx', op, dtype, dev(x, dtype), dev(y, dtype), x, y, dz, want_dx=False)
            assert accs[0] is None and accs[1] is not None
            _, accs = check_map(rec, case + ', no dy', op, dtype, dev(x, dtype), dev(y, dtype), x, y, dz, want_dy=False)
            assert accs[1] is None and accs[0] is not None
    rec.done()


def test_cpu_tensors_are_refused():
    from mxfusion_amd import ops, _lib
    x = torch.rand(2, 3, dtype=torch.float64)
    for call in (lambda: ops.ewise('add', x, x), lambda: ops.ewise('exp', x), lambda: ops.reduce('sum', x, None),
                 lambda: ops.ewise_bwd_('add', x, x, x, x.clone(), None), lambda: ops.reduce_bwd_('sum', x, None, x[:, :1], x.clone())):
        with pytest.raises(_lib.MXFError):
            call()


# ---- reductions ---------------------------------------------------------------------------------------------------------------------------

# (outer, R, inner): both regimes (inner == 1: a wave per row up to R = 512, a workgroup beyond; inner > 1: a loop over R), R around the
# wave's 64 lanes and the workgroup's 256 threads, inner around the wave
EXTENTS = [(1, 1, 1), (3, 63, 1), (3, 64, 1), (1, 65, 1), (3, 257, 1), (3, 1025, 1), (1, 1025, 3), (3, 63, 3), (1, 64, 64), (3, 65, 65),
           (3, 1, 65), (1, 257, 64)]


def reduce_want(kind, x, dims, dy, dtype_t):
    """the result and its gradient under dy by torch autograd on the CPU in dtype_t; dims: axes of the full array, descending"""
    xt = x.to(dtype_t).requires_grad_(True)
    out = xt
    for d in dims:
        out = getattr(torch, kind)(out, d)
    g, = torch.autograd.grad(out, xt, dy.to(dtype_t).reshape(out.shape))
    return out.detach(), g


def check_reduce(rec, label, kind, dtype, x, axes, dims, out_shape):
    from mxfusion_amd import ops
    r = np.random.RandomState(3)
    dy = _round(r.randn(*out_shape), dtype)
    want, gwant = reduce_want(kind, x, dims, dy, torch.float64)
    c32, g32 = reduce_want(kind, x, dims, dy, torch.float32)
    M = x.abs()
    for d in dims:
        M = M.sum(d)
    M = want.abs() if kind == 'prod' else M / (x.numel() / want.numel()) if kind == 'mean' else M
    xd = dev(x, dtype)
    got = ops.reduce(kind, xd, axes)
    assert tuple(got.shape) == tuple(out_shape), (label, kind, tuple(got.shape), out_shape)
    rec.check('%s %s' % (label, kind), dtype, got.reshape(want.shape), want, c32, M)
    acc = torch.full(tuple(x.shape), PREFILL, dtype=_tdt(dtype), device='cuda')
    ops.reduce_bwd_(kind, xd, axes, dev(dy, dtype), acc)
    torch.cuda.synchronize()
    rec.check('%s %s dx' % (label, kind), dtype, acc, PREFILL + gwant, PREFILL + g32, PREFILL + gwant.abs())


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', ['sum', 'mean', 'prod'])
def test_reductions_over_one_axis(kind, dtype):
    rec = Record('reduce %s over one axis, %s' % (kind, dtype))
    for outer, R, inner in EXTENTS:
        r = np.random.RandomState(outer + 7 * R + 13 * inner)
        shape = (outer, R) + ((inner,) if inner > 1 else ())
        x = _round(2.0 ** r.uniform(-1, 1, shape) * r.choice([-1.0, 1.0], shape) if kind == 'prod' else r.randn(*shape), dtype)
        check_reduce(rec, str((outer, R, inner)), kind, dtype, x, 0, (1,), (outer,) + ((inner,) if inner > 1 else ()))
    rec.done()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', ['sum', 'mean', 'prod'])
def test_reductions_axis_forms(kind, dtype):
    """axis=None gives (S, 1); an axis or a tuple drops the axes; a tuple that is not adjacent takes the permuted path; negative axes count
    from the end of the per-sample array"""
    rec = Record('reduce %s, axis forms, %s' % (kind, dtype))
    r = np.random.RandomState(17)
    shape = (3, 4, 5, 6)
    x = _round(2.0 ** r.uniform(-1, 1, shape) * r.choice([-1.0, 1.0], shape), dtype)
    for axes, dims, out_shape in ((None, (3, 2, 1), (3, 1)), (1, (2,), (3, 4, 6)), (-1, (3,), (3, 4, 5)), ((0, 1), (2, 1), (3, 6)),
                                  ((1, 2), (3, 2), (3, 4)), ((0, 2), (3, 1), (3, 5)), ((2, 0), (3, 1), (3, 5)), ((0, 1, 2), (3, 2, 1), (3,))):
        check_reduce(rec, 'axes %s' % (axes,), kind, dtype, x, axes, dims, out_shape)
    rec.done()


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('inner', [1, 3])
def test_prod_rows_with_zeros(inner, dtype):
    """a row with exactly one zero has one non-zero gradient entry, the product of the others; a row with two zeros has none: prefix and
    suffix products, no division"""
    rec = Record('prod with zeros, inner %d, %s' % (inner, dtype))
    r = np.random.RandomState(23)
    shape = (3, 65) + ((inner,) if inner > 1 else ())
    x = r.uniform(0.5, 2.0, shape)
    x[0, 17] = 0.0
    x[1, 3] = 0.0
    x[1, 64] = 0.0
    x = _round(x, dtype)
    check_reduce(rec, 'zeros', 'prod', dtype, x, 0, (1,), (3,) + ((inner,) if inner > 1 else ()))
    from mxfusion_amd import ops
    acc = torch.zeros(shape, dtype=_tdt(dtype), device='cuda')
    ops.reduce_bwd_('prod', dev(x, dtype), 0, torch.ones((3,) + ((inner,) if inner > 1 else ()), dtype=_tdt(dtype), device='cuda'), acc)
    acc = acc.cpu()
    assert torch.isfinite(acc).all() and (acc[1] == 0).all() and int((acc[0] != 0).sum()) == inner and (acc[0, 17] != 0).all()
    rec.done()


def test_float32_sum_of_1025_mixed_sign_terms_is_held_to_the_bar():
    """what accumulating in double buys: the sum of 1025 float32 terms of both signs, which cancel to a small total, within
    max(4 x torch's float32 error, 8 * 2^-24 * sum|x| / |sum|) -- for every row, one by one, not only normwise over the rows"""
    from mxfusion_amd import ops
    r = np.random.RandomState(29)
    x = _round(r.randn(3, 1025) * 10.0 ** r.uniform(-2, 2, (3, 1025)), 'float32')
    got = ops.reduce('sum', x.float().cuda(), 0).double().cpu()
    want, c32, M = x.sum(1), x.float().sum(1).double(), x.abs().sum(1)
    for i in range(3):
        e, b = nerr(got[i], want[i]), bar('float32', want[i].numpy(), c32[i].numpy(), M[i].numpy())
        print('float32 sum of 1025 terms, row %d: error %.3g, bar %.3g (sum|x| / |sum| = %.3g); one rounding of the exact sum is %.3g'
              % (i, e, b, float(M[i] / want[i].abs()), EPS32))
        assert e <= b
        assert e <= 2 * EPS32          # the double accumulator leaves the final rounding alone


# ---- the raw ABI ---------------------------------------------------------------------------------------------------------------------------

def test_raw_abi_refusals():
    from mxfusion_amd import _lib
    lib, h = _lib.load(), _lib.handle(torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    arr = lambda v: (ctypes.c_int64 * len(v))(*v)
    x = torch.ones(64, dtype=torch.float64, device='cuda')
    z = torch.full((64,), 7.5, dtype=torch.float64, device='cuda')
    g = torch.full((64,), 7.5, dtype=torch.float64, device='cuda')
    ext6, s6 = arr([2, 2, 2, 2, 2, 2]), arr([32, 16, 8, 4, 2, 1])
    assert lib.mxf_ewise_fwd(h, 0, _lib.F64, 6, ext6, x.data_ptr(), s6, x.data_ptr(), s6, z.data_ptr(), st) == -3
    assert lib.mxf_ewise_bwd(h, 0, _lib.F64, 6, ext6, x.data_ptr(), s6, x.data_ptr(), s6, x.data_ptr(), g.data_ptr(), None, st) == -3
    ext1, s1 = arr([64]), arr([1])
    assert lib.mxf_ewise_fwd(h, 0, _lib.F64, 1, ext1, None, s1, x.data_ptr(), s1, z.data_ptr(), st) == -2
    assert b'null' in lib.mxf_last_error(h)
    assert lib.mxf_ewise_bwd(h, 0, _lib.F64, 1, ext1, None, s1, x.data_ptr(), s1, x.data_ptr(), g.data_ptr(), None, st) == -2
    assert lib.mxf_ewise_fwd(h, 8, _lib.F64, 1, ext1, x.data_ptr(), s1, x.data_ptr(), s1, z.data_ptr(), st) == -2
    assert lib.mxf_ewise_fwd(h, 0, _lib.F64, 1, ext1, x.data_ptr(), arr([-1]), x.data_ptr(), s1, z.data_ptr(), st) == -2
    assert lib.mxf_reduce_fwd(h, 3, _lib.F64, 1, 64, 1, x.data_ptr(), z.data_ptr(), st) == -2
    assert lib.mxf_reduce_fwd(h, 0, _lib.F64, 1, 64, 1, None, z.data_ptr(), st) == -2
    torch.cuda.synchronize()
    assert bool((z == 7.5).all()) and bool((g == 7.5).all())          # a refused call touches no buffer
    assert lib.mxf_ewise_fwd(h, 0, _lib.F64, 1, ext1, x.data_ptr(), s1, x.data_ptr(), s1, z.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((z == 2.0).all())


# ---- the operators through the graph ---------------------------------------------------------------------------------------------------------

def _graph_cases():
    from mxfusion_amd.components.functions import operators as O
    bin_np = {'add': np.add, 'subtract': np.subtract, 'multiply': np.multiply, 'divide': np.divide, 'power': np.power}
    cases = [(name, lambda a, b, f=getattr(O, name): f(a, b), [(4, 5), (4, 5)], fn, 'pos') for name, fn in bin_np.items()]
    cases += [('add, lower rank', lambda a, b: O.add(a, b), [(4, 5), (5,)], np.add, 'pos'),
              ('square', lambda a: O.square(a), [(4, 5)], np.square, 'any'), ('exp', lambda a: O.exp(a), [(4, 5)], np.exp, 'any'),
              ('log', lambda a: O.log(a), [(4, 5)], np.log, 'pos'),
              ('dot', lambda a, b: O.dot(a, b), [(4, 5), (5, 2)], np.dot, 'any'),
              ('diag of a vector', lambda a: O.diag(a), [(5,)], np.diag, 'any'), ('diag of a matrix', lambda a: O.diag(a, k=0), [(5, 5)], np.diag, 'any'),
              ('reshape', lambda a: O.reshape(a, (10, -1)), [(4, 5)], lambda s: s.reshape(10, -1), 'any'),
              ('transpose', lambda a: O.transpose(a), [(4, 5, 2)], np.transpose, 'any'),
              ('transpose, axes', lambda a: O.transpose(a, axes=(1, 0, 2)), [(4, 5, 2)], lambda s: s.transpose(1, 0, 2), 'any'),
              ('broadcast_to', lambda a: O.broadcast_to(a, (4, 3, 5)), [(1, 5)], lambda s: np.broadcast_to(s, (4, 3, 5)), 'any')]
    for name, fn in (('sum', np.sum), ('mean', np.mean), ('prod', np.prod)):
        f = getattr(O, name)
        cases += [(name + ', axis=None', lambda a, f=f: f(a), [(4, 5, 2)], lambda s, fn=fn: fn(s).reshape(1), 'pos'),
                  (name + ', axis=1', lambda a, f=f: f(a, axis=1), [(4, 5, 2)], lambda s, fn=fn: fn(s, axis=1), 'pos'),
                  (name + ', axis=(0, 2)', lambda a, f=f: f(a, axis=(0, 2)), [(4, 5, 2)], lambda s, fn=fn: fn(s, axis=(0, 2)), 'pos')]
    return cases


@pytest.mark.parametrize('S', [1, 3])
def test_operators_through_factor_eval(S, monkeypatch):
    """each of the sixteen operators on (S, ...) inputs, the last input shared over the samples where there are two: the per-sample numpy
    result, stacked; sum / mean / prod give (S, 1) for axis=None and drop the axes otherwise.  With FUSED_OPERATORS set, so that the
    arithmetic runs through the HIP entry points whatever the default is."""
    from mxfusion_amd import Variable
    from mxfusion_amd.components.functions.operators import operators as impl
    monkeypatch.setattr(impl, 'FUSED_OPERATORS', True)
    seen = set()
    worst = 0.0
    for label, make, shapes, fn, domain in _graph_cases():
        r = np.random.RandomState(len(label))
        vs = [Variable(shape=s) for s in shapes]
        arrays = [(r.uniform(0.5, 2.0, ((S if i == 0 or len(shapes) == 1 else 1),) + s) if domain == 'pos' else r.randn(*(((S if i == 0 else 1),) + s)))
                  for i, s in enumerate(shapes)]
        out = make(*vs)
        f = out.factor
        seen.add(f.operator_name)
        got = f.eval(torch, {v.uuid: torch.as_tensor(a).cuda() for v, a in zip(vs, arrays)})
        want = np.stack([fn(*[a[s if a.shape[0] > 1 else 0] for a in arrays]) for s in range(S)])
        assert tuple(got.shape) == want.shape, (label, tuple(got.shape), want.shape)
        e = nerr(got.cpu().numpy(), want)
        worst = max(worst, e)
        assert e <= F64_BAR, (label, e)
    assert len(seen) == 16, seen
    print('operators through factor.eval, S = %d: worst error %.3g' % (S, worst))


def test_fused_and_torch_routes_agree_under_autograd(monkeypatch):
    """the autograd functions over ops.ewise / ops.reduce against the torch route (FUSED_OPERATORS = False) of the same operators, in
    float64: values and the gradients of an operand that is shared over the samples, an expanded one and a lower-rank one"""
    from mxfusion_amd.components.functions.operators import operators as impl
    r = np.random.RandomState(41)
    a0, b0, c0 = (torch.as_tensor(r.uniform(0.5, 2.0, s)) for s in ((3, 33, 5), (1, 5), (1, 1, 1)))

    def run():
        a, b, c = (t.cuda().requires_grad_(True) for t in (a0, b0, c0))
        z = impl._ewise('multiply', impl._ewise('add', a, b), c.expand(1, 33, 5))
        z = impl._ewise('power', z, impl._ewise('exp', b))
        out = impl._reduce('sum', impl._ewise('log', z), (0,)) + impl._reduce('prod', impl._ewise('divide', b, c), None) \
            + impl._reduce('mean', impl._ewise('square', impl._ewise('subtract', a, c)), (0, 1)).reshape(3, 1)
        out.sum().backward()
        return [t.detach().cpu().numpy() for t in (out, a.grad, b.grad, c.grad)]
    monkeypatch.setattr(impl, 'FUSED_OPERATORS', True)
    fused = run()
    monkeypatch.setattr(impl, 'FUSED_OPERATORS', False)
    plain = run()
    for name, g, w in zip(('value', 'da', 'db', 'dc'), fused, plain):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        print('fused against the torch route, %s: %.3g' % (name, nerr(g, w)))
        assert nerr(g, w) <= F64_BAR, (name, nerr(g, w))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------

N, D, S = 33, 5, 3
LOG_S, Q_VAR_RAW = -1.0, -3.0
LATENT = (('w', (D, 1)), ('b', (1,)))


@functools.lru_cache(maxsize=None)
def e2e_data(dtype):
    r = np.random.RandomState(7)
    x = r.randn(N, D)
    y = x @ r.randn(D, 1) + 0.3 + 0.2 * r.randn(N, 1)
    eps = {k: _round(r.randn(S, *s), dtype) for k, s in LATENT}
    init = {k: _round(0.3 * r.randn(*s), dtype) for k, s in LATENT}
    return _round(x, dtype), _round(y, dtype), eps, init


def _logn(x, mean, var):
    return -0.5 * np.log(2 * np.pi) - 0.5 * torch.log(var) - (x - mean) ** 2 / (2 * var)


def e2e_restatement(dtype_in, dtype):
    """the negative Monte-Carlo ELBO of the model below and its gradients in torch `dtype` on the CPU, with their magnitudes; the leaves are
    the stored (unconstrained) values"""
    x, y, eps, init = e2e_data(dtype_in)
    tt = lambda t: t.to(dtype)
    leaves = {'log_s': torch.full((1,), LOG_S, dtype=dtype).requires_grad_(True)}
    for k, s in LATENT:
        leaves[k + '_mean'] = tt(init[k]).clone().requires_grad_(True)
        leaves[k + '_var_raw'] = torch.full(s, Q_VAR_RAW, dtype=dtype).requires_grad_(True)
    sp = torch.nn.functional.softplus
    draws, prior, ent = {}, 0.0, 0.0
    for k, _ in LATENT:
        var = sp(leaves[k + '_var_raw'])
        draws[k] = leaves[k + '_mean'] + torch.sqrt(var) * tt(eps[k])
        prior = prior + _logn(draws[k], torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)).sum() / S
        ent = ent + _logn(draws[k], leaves[k + '_mean'], var).sum() / S
    s_ = torch.exp(leaves['log_s'])
    ll = 0.0
    for i in range(S):
        mean = tt(x) @ draws['w'][i] + draws['b'][i]
        ll = ll + _logn(tt(y), mean, (s_ * s_).expand(N, 1)).sum() / S
    groups = [ll, prior, -ent]
    loss = -sum(groups)
    names = list(leaves)
    g = torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)
    gmag = [np.zeros(tuple(leaves[k].shape)) for k in names]
    for part in groups:
        for i, gi in enumerate(torch.autograd.grad(part, [leaves[k] for k in names], retain_graph=True, allow_unused=True)):
            if gi is not None:
                gmag[i] = gmag[i] + np.abs(gi.detach().double().numpy())
    return (float(loss.detach()), {k: gi.detach().double().numpy() for k, gi in zip(names, g)},
            sum(abs(float(p.detach())) for p in groups), dict(zip(names, gmag)))


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_model_written_with_operators_under_svi(dtype, monkeypatch):
    """m.w, m.b ~ Normal, m.s = exp(m.log_s), m.y ~ Normal(dot(m.x, m.w) + m.b, broadcast_to(m.s * m.s, (N, 1))) with N = 33, D = 5 and 3
    samples, a Gaussian mean field, the noise injected through MockRandomGenerator: the loss and every parameter gradient against the
    float64 CPU restatement that sees the same draws.  float32 bars as in tests/test_gpu_bnn.py: M is, for the loss, the sum of the
    absolute values of the three groups of terms (likelihood, prior, entropy) and, for a gradient, the norm of the sum of the absolute
    gradients of the three groups.  The +, * and exp go through ops.ewise."""
    from mxfusion_amd import Model, Variable, ops
    from mxfusion_amd.components.distributions import Normal
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    from mxfusion_amd.components.functions.operators import broadcast_to, dot, exp, operators as impl
    from mxfusion_amd.inference import GradBasedInference, StochasticVariationalInference, create_Gaussian_meanfield, BatchInferenceLoop
    monkeypatch.setattr(impl, 'FUSED_OPERATORS', True)
    calls = []
    real = ops.ewise
    monkeypatch.setattr(ops, 'ewise', lambda op, x, y=None: (calls.append(op), real(op, x, y))[1])
    x, y, eps, init = e2e_data(dtype)
    m = Model()
    m.N = Variable()
    m.x = Variable(shape=(m.N, D))
    m.w = Normal.define_variable(mean=broadcast_to(torch.tensor([0.]), (D, 1)), variance=broadcast_to(torch.tensor([1.]), (D, 1)), shape=(D, 1))
    m.b = Normal.define_variable(mean=broadcast_to(torch.tensor([0.]), (1,)), variance=broadcast_to(torch.tensor([1.]), (1,)), shape=(1,))
    m.log_s = Variable(shape=(1,), initial_value=torch.tensor([LOG_S], dtype=torch.float64))
    m.s = exp(m.log_s)
    m.y = Normal.define_variable(mean=dot(m.x, m.w) + m.b, variance=broadcast_to(m.s * m.s, (m.N, 1)), shape=(m.N, 1))
    observed = [m.y, m.x]
    q = create_Gaussian_meanfield(model=m, observed=observed)
    alg = StochasticVariationalInference(num_samples=S, model=m, posterior=q, observed=observed)
    infr = GradBasedInference(inference_algorithm=alg, grad_loop=BatchInferenceLoop(), dtype=dtype)
    infr.initialize(y=dev(y, dtype), x=dev(x, dtype))
    infr.params[m.log_s] = torch.tensor([LOG_S], dtype=torch.float64)
    latent = {'w': m.w, 'b': m.b}
    for k, v in latent.items():
        infr.params[q[v].factor.mean] = dev(init[k], dtype)
        infr.params.raw(q[v].factor.variance).fill_(Q_VAR_RAW)
        q[v].factor._rand_gen = MockRandomGenerator(dev(eps[k], dtype))
    infr.params.zero_grad()
    loss, loss_for_gradient = infr.create_executor()(dev(y, dtype), dev(x, dtype))
    loss_for_gradient.backward()
    torch.cuda.synchronize()
    got = {'log_s': infr.params.grad(m.log_s)}
    for k, v in latent.items():
        got[k + '_mean'] = infr.params.grad(q[v].factor.mean)
        got[k + '_var_raw'] = infr.params.grad(q[v].factor.variance)
    got = {k: g.detach().double().cpu().numpy() for k, g in got.items()}
    wloss, wgrads, mloss, mgrads = e2e_restatement(dtype, torch.float64)
    tiny = np.finfo(np.float64).tiny
    if dtype == 'float64':
        bloss, bgrads = F64_BAR, {k: F64_BAR for k in wgrads}
    else:
        loss32, grads32, _, _ = e2e_restatement(dtype, torch.float32)
        floor = lambda w, mm: 8 * EPS32 * _norm(mm) / max(_norm(w), tiny)
        bloss = max(4 * nerr(loss32, wloss), floor(wloss, mloss))
        bgrads = {k: max(4 * nerr(grads32[k], wgrads[k]), floor(wgrads[k], mgrads[k])) for k in wgrads}
    e = nerr(float(loss.detach()), wloss)
    errs = {k: nerr(got[k].reshape(wgrads[k].shape), wgrads[k]) for k in wgrads}
    worst = max(errs, key=lambda k: errs[k] / bgrads[k])
    print('operators end to end %s: loss %.9g (want %.9g) error %.3g (bar %.3g); worst gradient %s %.3g (bar %.3g); widest bar %.3g; ewise calls %s'
          % (dtype, float(loss.detach()), wloss, e, bloss, worst, errs[worst], bgrads[worst], max(bgrads.values()), calls))
    assert e <= bloss, ('loss', e, bloss)
    for k in wgrads:
        assert got[k].size == wgrads[k].size, (k, got[k].shape, wgrads[k].shape)
        assert errs[k] <= bgrads[k], (k, errs[k], bgrads[k])
    assert set(calls) == {'add', 'exp', 'multiply'}, calls          # the +, the * and the exp, each through ops.ewise
