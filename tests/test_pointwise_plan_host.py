"""CPU test of the plans of the pointwise and per-row launchers (mxfusion_amd/csrc/pointwise_plan.h: plain C++, no HIP).
tests/host/pointwise_plan_check.cpp, built with the system C++ compiler, prints the plan of every request it reads.  Checked here: every plan
column over a sweep across each boundary against a transcription of the launchers' arithmetic as it stood before the plans were split out
of them (elementwise.hip, ewise.hip, simplex.hip, dense.hip), the invariants the kernels rely on, and every refusal's code and text in the
order the launchers raised them."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = 0, 1
LIMIT = 1 << 35

REDUCE_IN = 'dtype kind bwd outer R inner has_x has_y has_dx'.split()
REDUCE_OUT = 'rc empty spread rows by_wave items scratch grid'.split()
SIMPLEX_IN = 'dtype bwd dirichlet S B K ss_x ss_p sb_p one_hot labels has_x has_p has_out has_cot has_dp has_dx'.split()
SIMPLEX_OUT = 'rc empty bucket p_atomic by_batch items n_sum grid'.split()
DENSE_IN = 'dtype bwd S N I O act ldx ss_x ss_w ss_b has_X has_W has_Y has_dY has_dX has_dW has_db'.split()
DENSE_OUT = 'rc empty tiles n_dw n_db by_rows grid'.split()
EW_HEAD = 'dtype op rank bwd has_extent has_stride_x has_stride_y has_x has_y has_z has_dx has_dy'.split()
EW_OUT = ('rc empty binary shared_x shared_y total chunks items numel_gx numel_gy wide_index sum_x sum_y inner_shared_x inner_shared_y grid'.split()
          + ['%s%d' % (k, d) for k in ('extent', 'sx', 'sy', 'gx', 'gy') for d in range(5)])
COLS = {'reduce': (REDUCE_IN, REDUCE_OUT), 'simplex': (SIMPLEX_IN, SIMPLEX_OUT), 'dense': (DENSE_IN, DENSE_OUT)}


@pytest.fixture(scope='module')
def check(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('pointwise_plan') / 'pointwise_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'pointwise_plan_check.cpp'), '-o', exe], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    return run


def rows(check, what, reqs, ncol):
    """the printed columns (a list of int lists) of the requests (lists of ints)"""
    out = check('\n'.join(what + ' ' + ' '.join(str(int(x)) for x in r) for r in reqs))
    got = [[int(x) for x in line.split()] for line in out.splitlines()]
    assert len(got) == len(reqs) and all(len(g) == ncol for g in got)
    return got


def plans(check, what, reqs):
    """per request, the plan as a dict; reqs are dicts over the input columns"""
    cin, cout = COLS[what]
    for r in reqs:
        assert set(r) == set(cin), set(r) ^ set(cin)
    return [dict(zip(cout, g)) for g in rows(check, what, [[r[k] for k in cin] for r in reqs], len(cout))]


def refusal(check, what, req):
    line = check('text 1\n%s %s\n' % (what, ' '.join(str(int(x)) for x in req))).rstrip('\n')
    rc, _, why = line.partition(' ')
    return int(rc), why


def cdiv(a, b):
    return -(-a // b)


def grid_for(n, cap=2048):
    return min(max(cdiv(n, 256), 1), cap)


def grid_for_reduce(n):
    return grid_for(n, 512)


# ---- the two grids and mxf_coldot -----------------------------------------------------------------------------------------------------------
def test_grids(check):
    ns = [0, 1, 256, 257, 512 * 256, 512 * 256 + 1, 2048 * 256, 2048 * 256 + 1, 1 << 40]
    got = rows(check, 'grid', [[n] for n in ns], 2)
    assert got == [[grid_for(n), grid_for_reduce(n)] for n in ns]
    assert got[0] == [1, 1] and got[4] == [512, 512] and got[5] == [513, 512] and got[6] == [2048, 512] and got[7] == [2048, 512]


def test_coldot_plan_is_the_parent_launcher(check):
    reqs = [(S, M, N) for S in (1, 2, 64) for M in (1, 63, 64, 1000) for N in (1, 15, 16, 17, 255, 256, 257, 8191, 8192, 16383, 16384, 16385)]
    got = rows(check, 'coldot', reqs, 3)
    seen = set()
    for (S, M, N), g in zip(reqs, got):
        small = S * N < 16384 and M >= 64                                  # mxf_coldot: `if ((int64_t)S * N < 16384 && M >= 64)`
        assert g == [int(small), (N + 15) // 16 if small else (N + 255) // 256, S], (S, M, N)
        assert g[1] >= 1
        seen.add((small, S * N >= 16384, M >= 64))
    assert len(seen) == 4                                                  # both sides of both conditions


# ---- reductions -----------------------------------------------------------------------------------------------------------------------------
def reduce_request(**over):
    r = dict(dtype=F64, kind=0, bwd=0, outer=5, R=7, inner=3, has_x=1, has_y=1, has_dx=1)
    r.update(over)
    return r


def parent_reduce(r):
    """red_launch_fwd / red_launch_bwd of ewise.hip"""
    outer, R, inner, kind = r['outer'], r['R'], r['inner'], r['kind']
    rows_grid = lambda: min(cdiv(outer, 4) if R <= 512 else outer, 65536)
    p = dict(rc=0, empty=0, spread=0, rows=0, by_wave=0, items=0, scratch=0)
    if r['bwd'] and kind != 2:
        p.update(spread=1, items=outer * R * inner, grid=grid_for(outer * R * inner))
        return p
    if r['bwd']:
        p['scratch'] = outer * R * inner
    if inner == 1:
        p.update(rows=1, by_wave=int(R <= 512), grid=rows_grid())
    else:
        p.update(items=outer * inner, grid=grid_for(outer * inner))
    return p


def test_reduce_plan_is_the_parent_launcher(check):
    reqs = [reduce_request(dtype=dt, kind=k, bwd=b, outer=o, R=R, inner=i)
            for dt in (F32, F64) for k in (0, 1, 2) for b in (0, 1) for o in (1, 3, 4, 5, 65537, 65536 * 4, 65536 * 4 + 1)
            for R in (1, 512, 513) for i in (1, 2)]
    got = plans(check, 'reduce', reqs)
    for r, g in zip(reqs, got):
        assert g == parent_reduce(r), (r, g)
        assert g['grid'] >= 1
    by = lambda **kw: [g for r, g in zip(reqs, got) if all(r[k] == v for k, v in kw.items())]
    assert {g['grid'] for g in by(outer=65536 * 4 + 1, R=512, inner=1, kind=2)} == {65536}          # the cap, by wave: 65537 blocks
    assert {g['grid'] for g in by(outer=65536 * 4, R=512, inner=1, kind=2)} == {65536}
    assert {g['grid'] for g in by(outer=65537, R=513, inner=1, kind=2)} == {65536}                  # the cap, a workgroup per row
    assert {g['grid'] for g in by(outer=5, R=512, inner=1, bwd=0)} == {2} and {g['grid'] for g in by(outer=4, R=512, inner=1, bwd=0)} == {1}


# ---- simplex --------------------------------------------------------------------------------------------------------------------------------
def simplex_request(**over):
    r = dict(dtype=F64, bwd=0, dirichlet=0, S=2, B=3, K=4, one_hot=1, labels=0, has_x=1, has_p=1, has_out=1, has_cot=1, has_dp=1, has_dx=1)
    r.update({k: v for k, v in over.items() if not k.startswith('ss_') and k != 'sb_p'})
    r['sb_p'] = over.get('sb_p', r['K'])
    r['ss_x'] = over.get('ss_x', r['B'] * (1 if r['labels'] else r['K']))
    r['ss_p'] = over.get('ss_p', (r['B'] if r['sb_p'] else 1) * r['K'])
    return r


def parent_simplex(r):
    """launch_fwd / launch_bwd and SIMPLEX_LAUNCH of simplex.hip"""
    S, B, K = r['S'], r['B'], r['K']
    bucket = 4 if K <= 4 else (16 if K <= 16 else 64)
    p = dict(rc=0, empty=0, bucket=bucket, p_atomic=0, by_batch=0, items=S * B, n_sum=0)
    if r['bwd']:
        dp, dx = r['has_dp'], r['has_dx']
        shared_over = lambda own_s, own_b: (not own_s and S > 1) or (not own_b and B > 1)
        p_atomic = bool(dp and shared_over(True, r['sb_p']))
        by_batch = bool((dp and not p_atomic and r['ss_p'] == 0 and S > 1) or (dx and r['ss_x'] == 0 and S > 1))
        p.update(p_atomic=int(p_atomic), by_batch=int(by_batch), items=B if by_batch else S * B,
                 n_sum=(S if r['ss_p'] else 1) * 1 * K if p_atomic else 0)                      # shared_numel(ss_p, false, S, B, K)
    p['grid'] = grid_for(p['items'] * bucket)
    return p


def test_simplex_plan_is_the_parent_launcher(check):
    reqs = []
    for K, S, B, dense_x, dense_sp, dense_bp, dp, dx, bwd in itertools.product((1, 4, 5, 16, 17, 64, 65), (1, 2), (1, 3, 70000), (0, 1), (0, 1), (0, 1),
                                                                            (0, 1), (0, 1), (0, 1)):
        if bwd and not dp and not dx:
            continue
        over = dict(K=K, S=S, B=B, bwd=bwd, has_dp=dp, has_dx=dx, dirichlet=K % 2)
        if not dense_x:
            over['ss_x'] = 0
        if not dense_bp:
            over['sb_p'] = 0
        if not dense_sp:
            over['ss_p'] = 0
        reqs.append(simplex_request(**over))
    got = plans(check, 'simplex', reqs)
    for r, g in zip(reqs, got):
        assert g == parent_simplex(r), (r, g)
        assert g['grid'] >= 1
    assert {g['bucket'] for g in got} == {4, 16, 64} and {(g['p_atomic'], g['by_batch']) for g in got} == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- dense ----------------------------------------------------------------------------------------------------------------------------------
def dense_request(**over):
    r = dict(dtype=F64, bwd=0, S=2, N=5, I=3, O=4, act=1, has_X=1, has_W=1, has_Y=1, has_dY=1, has_dX=1, has_dW=1, has_db=1)
    r.update({k: v for k, v in over.items() if k not in ('ldx', 'ss_x', 'ss_w', 'ss_b')})
    r['ldx'] = over.get('ldx', r['I'])
    r['ss_x'] = over.get('ss_x', r['N'] * r['ldx'])
    r['ss_w'] = over.get('ss_w', r['O'] * r['I'])
    r['ss_b'] = over.get('ss_b', r['O'])
    return r


def parent_dense(r):
    """check_operands, launch_fwd and launch_bwd of dense.hip (DenseTile: 32 rows for float, 16 for double)"""
    tile = 16 if r['dtype'] == F64 else 32
    tiles = (r['N'] + tile - 1) // tile
    by_rows = bool(r['bwd'] and r['has_dX'] and r['ss_x'] == 0 and r['S'] > 1)
    return dict(rc=0, empty=0, tiles=tiles, n_dw=(r['S'] if r['ss_w'] else 1) * r['O'] * r['I'], n_db=(r['S'] if r['ss_b'] else 1) * r['O'],
                by_rows=int(by_rows), grid=tiles if by_rows else tiles * r['S'])


def test_dense_plan_is_the_parent_launcher(check):
    reqs = []
    for dt, N, S, shared_x, shared_w, bwd, dX in itertools.product((F32, F64), (1, 15, 16, 17, 31, 32, 33, 63, 64, 65), (1, 2), (0, 1), (0, 1), (0, 1), (0, 1)):
        over = dict(dtype=dt, N=N, S=S, bwd=bwd, has_dX=dX)
        if shared_x:
            over['ss_x'] = 0
        if shared_w:
            over.update(ss_w=0, ss_b=0)
        reqs.append(dense_request(**over))
    for dt, tile in ((F32, 32), (F64, 16)):                                   # tiles * S at the grid limit, and the largest S on the other side of by_rows
        reqs.append(dense_request(dtype=dt, N=tile * 0x7fffffff, S=1, ss_x=0))
        reqs.append(dense_request(dtype=dt, N=tile * 0x3fffffff, S=2, ss_x=0, bwd=1))
    got = plans(check, 'dense', reqs)
    for r, g in zip(reqs, got):
        assert g == parent_dense(r), (r, g)
        assert 1 <= g['grid'] <= 0x7fffffff
    assert {g['by_rows'] for g in got} == {0, 1}


# ---- the broadcast map ------------------------------------------------------------------------------------------------------------------------
def ewise_request(extent, sx, sy=None, dtype=F64, op=0, bwd=0, rank=None, has=(1, 1, 1, 1, 1, 1, 1, 1)):
    """has: extent, stride_x, stride_y arrays, x, y, z (dz), dx, dy"""
    pad = lambda a: list(a) + [0] * (5 - len(a))
    return [dtype, op, len(extent) if rank is None else rank, bwd] + list(has) + pad(extent) + pad(sx) + pad(sy if sy is not None else sx)


def parent_ewise(req):
    """ew_plan, ew_items, ew_launch_fwd and ew_launch_bwd of ewise.hip; None: nothing to do"""
    dtype, op, rank, bwd = req[:4]
    dx, dy = req[10], req[11]
    extent, stride_x, stride_y = req[12:17], req[17:22], req[22:27]
    binary = op <= 4
    a = dict(extent=[0] * 5, sx=[0] * 5, sy=[0] * 5, gx=[0] * 5, gy=[0] * 5)
    total, shared_x, shared_y = 1, False, False
    for d in range(rank):
        e = extent[d]
        sx, sy = (stride_x[d] if e > 1 else 0), (stride_y[d] if binary and e > 1 else 0)
        a['extent'][d], a['sx'][d], a['sy'][d] = e, sx, sy
        shared_x |= e > 1 and sx == 0
        shared_y |= e > 1 and sy == 0 and binary
        total = 0 if e == 0 else total * e
    if total == 0:
        return None
    if op > 4:
        dy = 0
    if bwd and not dx and not dy:
        return None
    ngx = ngy = 1
    for d in range(rank - 1, -1, -1):
        own_x, own_y = a['extent'][d] > 1 and a['sx'][d] != 0, binary and a['extent'][d] > 1 and a['sy'][d] != 0
        a['gx'][d], a['gy'][d] = (ngx if own_x else 0), (ngy if own_y else 0)
        ngx, ngy = ngx * (a['extent'][d] if own_x else 1), ngy * (a['extent'][d] if own_y else 1)
    V = 2 if dtype == F64 else 4                                              # Vec16<T>::n
    inner = a['extent'][rank - 1]
    chunks = (inner + V - 1) // V
    items = total // inner * chunks
    sum_x, sum_y = bool(bwd and shared_x and dx), bool(bwd and shared_y and dy)                # sums.acc[0], sums.acc[1]
    p = dict(rc=0, empty=0, binary=int(binary), shared_x=int(shared_x), shared_y=int(shared_y), total=total, chunks=chunks, items=items, numel_gx=ngx,
             numel_gy=ngy, wide_index=int(not items < (1 << 31)), sum_x=int(sum_x), sum_y=int(sum_y),
             inner_shared_x=int(inner > 1 and a['sx'][rank - 1] == 0), inner_shared_y=int(inner > 1 and a['sy'][rank - 1] == 0),
             grid=grid_for_reduce(items) if sum_x or sum_y else grid_for(items))
    for k in ('extent', 'sx', 'sy', 'gx', 'gy'):
        p.update({'%s%d' % (k, d): a[k][d] for d in range(5)})
    return p


def dense_strides(extent, shared=()):
    s, out = 1, []
    for d in range(len(extent) - 1, -1, -1):
        out.append(0 if d in shared else s)
        s *= 1 if d in shared else max(extent[d], 1)
    return out[::-1]


def test_ewise_plan_is_the_parent_launcher(check):
    reqs = []
    shapes = [(5,), (1,), (0,), (3, 5), (3, 1), (1, 7), (3, 0), (2, 3, 4), (2, 1, 9), (2, 3, 4, 5), (2, 3, 1, 5, 7), (4, 1, 1, 1, 3), (1, 1, 1, 1, 1)]
    for extent in shapes:
        rank = len(extent)
        for shared_x, shared_y in [((), ()), ((rank - 1,), ()), ((), (rank - 1,)), ((0,), (rank - 1,)), ((0,), (0,)), (tuple(range(rank)), ())]:
            for dtype, op, bwd, dx, dy in itertools.product((F32, F64), (0, 4, 5, 7), (0, 1), (0, 1), (0, 1)):
                reqs.append(ewise_request(extent, dense_strides(extent, shared_x), dense_strides(extent, shared_y), dtype=dtype, op=op, bwd=bwd,
                                          has=(1, 1, 1, 1, 1, 1, dx, dy)))
    for dtype, V in ((F32, 4), (F64, 2)):                                     # the index width: items at 2^31 - 1 and 2^31; and the 2^35 limits
        for items in ((1 << 31) - 1, 1 << 31):
            reqs.append(ewise_request((items, 1), (0, 0), dtype=dtype))                             # one chunk per row: `items` rows
            reqs.append(ewise_request((items, 1), (1, 0), dtype=dtype, bwd=1))
            reqs.append(ewise_request((items * V,), (0,), dtype=dtype) if items * V <= LIMIT else ewise_request((items // 2, V + 1), (0, 0), dtype=dtype))
        reqs.append(ewise_request((1 << 35,), (1,), dtype=dtype))
        reqs.append(ewise_request((1 << 17, 1 << 18), (1 << 18, 1), (0, 1), dtype=dtype, bwd=1))
        reqs.append(ewise_request((2,), (1 << 35,), dtype=dtype))
    got = rows(check, 'ewise', reqs, len(EW_OUT))
    seen = set()
    for r, g in zip(reqs, got):
        g = dict(zip(EW_OUT, g))
        want = parent_ewise(r)
        if want is None:
            assert g['rc'] == 0 and g['empty'] == 1 and not any(v for k, v in g.items() if k != 'empty'), r
            continue
        assert g == want, (r, g, want)
        rank = r[2]
        inner = g['extent%d' % (rank - 1)]
        assert g['grid'] >= 1 and g['items'] == g['total'] // inner * g['chunks']
        for d in range(rank):                                                 # gx, gy are zero exactly on shared (or unit) axes
            assert (g['gx%d' % d] == 0) == (g['extent%d' % d] <= 1 or g['sx%d' % d] == 0)
            assert (g['gy%d' % d] == 0) == (g['extent%d' % d] <= 1 or g['sy%d' % d] == 0 or not g['binary'])
        seen.add((g['wide_index'], g['items'] in ((1 << 31) - 1, 1 << 31)))
    assert (0, True) in seen and (1, True) in seen


# ---- refusals: code, text and order ---------------------------------------------------------------------------------------------------------
def _req(cols, r):
    return [r[k] for k in cols]


REFUSALS = [
    # (what, request, rc, text); each later request of a family also trips nothing that an earlier one of the same call tests
    ('reduce', reduce_request(dtype=7, kind=9, outer=-1), -2, 'bad dtype 7'),
    ('reduce', reduce_request(kind=3, outer=-1), -2, 'kind 3 (0 sum, 1 mean, 2 prod)'),
    ('reduce', reduce_request(outer=-1, R=0, inner=2, has_x=0), -2, 'extents (-1, 0, 2)'),
    ('reduce', reduce_request(outer=1 << 20, R=2, inner=1 << 15, has_x=0), -3, 'more than 2^35 elements'),
    ('reduce', reduce_request(has_x=0), -2, 'null x or y'),
    ('reduce', reduce_request(has_y=0), -2, 'null x or y'),
    ('reduce', reduce_request(bwd=1, has_y=0), -2, 'null x or dy'),
    ('reduce', reduce_request(bwd=1, kind=2, has_x=0), -2, 'null x or dy'),
    ('simplex', simplex_request(dtype=7, K=0), -2, 'bad dtype 7'),
    ('simplex', simplex_request(K=0, bwd=1, one_hot=0, labels=1), -2, 'K = 0 classes, at least 1 is needed'),
    ('simplex', simplex_request(bwd=1, one_hot=0, labels=1, S=0, has_x=0), -2, 'dx_acc must be null without one-hot encoding (a label has no gradient)'),
    ('simplex', simplex_request(has_p=0, ss_x=5), -2, 'null operand'),
    ('simplex', simplex_request(ss_x=5, sb_p=3), -2, 'the sample stride of x is 0 or 12 (dense), got 5'),
    ('simplex', simplex_request(one_hot=0, labels=1, ss_x=12), -2, 'the sample stride of x is 0 or 3 (dense), got 12'),
    ('simplex', simplex_request(sb_p=3, ss_p=5), -2, 'the batch stride of the parameter is 0 or K = 4, got 3'),
    ('simplex', simplex_request(sb_p=0, ss_p=12, has_out=0), -2, 'the sample stride of the parameter is 0 or 4 (dense), got 12'),
    ('simplex', simplex_request(has_out=0), -2, 'null out'),
    ('simplex', simplex_request(bwd=1, has_cot=0, has_dp=0, has_dx=0), -2, 'null cotangent'),
    ('dense', dense_request(dtype=7, I=0), -2, 'bad dtype 7'),
    ('dense', dense_request(I=0, act=4), -3, 'widths I = 0, O = 4; 1 .. 128 are supported'),
    ('dense', dense_request(O=129, act=4), -3, 'widths I = 3, O = 129; 1 .. 128 are supported'),
    ('dense', dense_request(act=4, has_Y=0), -2, 'activation 4 (0 identity, 1 tanh, 2 relu, 3 sigmoid)'),
    ('dense', dense_request(has_Y=0, has_X=0), -2, 'null Y'),
    ('dense', dense_request(bwd=1, has_dY=0, has_X=0), -2, 'null Y or dY'),
    ('dense', dense_request(has_W=0, ldx=2), -2, 'null operand'),
    ('dense', dense_request(ldx=2, ss_x=1), -2, 'ldx = 2 < I = 3'),
    ('dense', dense_request(ldx=4, ss_x=18, ss_w=5), -2, 'the sample stride of X is 0 or at least (N - 1) ldx + I = 19, got 18'),
    ('dense', dense_request(ss_w=5, ss_b=3), -2, 'the sample stride of W is 0 or O I = 12 (dense), got 5'),
    ('dense', dense_request(ss_b=3), -2, 'the sample stride of b is 0 or O = 4, got 3'),
    ('dense', dense_request(dtype=F32, N=32 * 0x7fffffff + 1, S=1, ss_x=0), -2, '2147483648 row tiles x 1 samples exceed the grid'),
    ('dense', dense_request(dtype=F64, N=16 * 0x40000000, S=2, ss_x=0, bwd=1), -2, '1073741824 row tiles x 2 samples exceed the grid'),
]
EW_REFUSALS = [
    (ewise_request((3,), (1,), dtype=7, op=9), -2, 'bad dtype 7'),
    (ewise_request((3,), (1,), op=8, rank=0), -2, 'op 8 (0 add .. 7 log)'),
    (ewise_request((3,), (1,), op=-1), -2, 'op -1 (0 add .. 7 log)'),
    (ewise_request((3,), (1,), rank=0, has=(0,) * 8), -2, 'rank 0'),
    (ewise_request((3,), (1,), rank=6, has=(0,) * 8), -3, 'rank 6 after merging; up to 5 axes are supported'),
    (ewise_request((-3,), (1,), has=(0, 1, 1, 1, 1, 1, 1, 1)), -2, 'null operand, extent or stride array'),
    (ewise_request((-3,), (1,), has=(1, 1, 0, 1, 1, 1, 1, 1)), -2, 'null operand, extent or stride array'),
    (ewise_request((-3,), (1,), has=(1, 1, 1, 1, 0, 1, 1, 1)), -2, 'null operand, extent or stride array'),
    (ewise_request((3, -3), (1, 1), (1, 1), op=5, has=(1, 1, 0, 1, 0, 0, 1, 1)), -2, 'axis 1 has extent -3, strides 0, 0'),
    (ewise_request((3, 4), (-2, 1), (1, -1), has=(1, 1, 1, 1, 1, 0, 1, 1)), -2, 'axis 0 has extent 3, strides -2, 1'),
    (ewise_request((3, 4), (1, 1), (1, -1), op=5, has=(1, 1, 1, 1, 1, 0, 1, 1)), -2, 'null z'),           # (a unary op never reads stride_y)
    (ewise_request((2, (1 << 35) + 1), (1, 1), has=(1, 1, 1, 1, 1, 0, 1, 1)), -3, 'axis 1 is beyond 2^35 elements'),
    (ewise_request((2, 2), (1, (1 << 35) + 1), has=(1, 1, 1, 1, 1, 0, 1, 1)), -3, 'axis 1 is beyond 2^35 elements'),
    (ewise_request((1 << 20, 1 << 16), (0, 0), has=(1, 1, 1, 1, 1, 0, 1, 1)), -3, 'more than 2^35 elements'),
    (ewise_request((3, 2), (1 << 34, 1 << 35), (0, 0), has=(1, 1, 1, 1, 1, 0, 1, 1)), -3, 'an operand spans more than 2^35 elements'),
    (ewise_request((3,), (1,), has=(1, 1, 1, 1, 1, 0, 1, 1)), -2, 'null z'),
    (ewise_request((3,), (1,), bwd=1, has=(1, 1, 1, 1, 1, 0, 0, 0)), -2, 'null dz'),
]


def test_refusals(check):
    for what, r, rc, why in REFUSALS:
        assert refusal(check, what, _req(COLS[what][0], r)) == (rc, why), (what, r)
    for r, rc, why in EW_REFUSALS:
        assert refusal(check, 'ewise', r) == (rc, why), r


def test_empty_calls_come_between_the_refusals_as_in_the_launchers(check):
    """nothing to do: after the checks that do not read the operands, before those that do"""
    empty = lambda what, r: plans(check, what, [r])[0]
    for r in (reduce_request(outer=0, has_x=0), reduce_request(inner=0, has_y=0), reduce_request(bwd=1, has_dx=0, has_y=0)):
        assert empty('reduce', r) == dict(zip(REDUCE_OUT, [0, 1] + [0] * 6)), r
    for r in (simplex_request(S=0, has_x=0, ss_x=5), simplex_request(B=0, has_out=0), simplex_request(bwd=1, has_dp=0, has_dx=0)):
        assert empty('simplex', r) == dict(zip(SIMPLEX_OUT, [0, 1] + [0] * 6)), r
    for r in (dense_request(S=0, has_Y=0), dense_request(N=0, has_X=0), dense_request(bwd=1, has_dX=0, has_dW=0, has_db=0, has_X=0, ldx=1)):
        assert empty('dense', r) == dict(zip(DENSE_OUT, [0, 1] + [0] * 5)), r
    for r in (ewise_request((3, 0), (1, 1), has=(1, 1, 1, 1, 1, 0, 0, 0)), ewise_request((3,), (1,), bwd=1, has=(1, 1, 1, 1, 1, 1, 0, 0)),
              ewise_request((3,), (1,), op=6, bwd=1, has=(1, 1, 0, 1, 0, 1, 0, 1))):
        g = rows(check, 'ewise', [r], len(EW_OUT))[0]
        assert g[:2] == [0, 1] and not any(g[2:]), r
    assert refusal(check, 'simplex', _req(SIMPLEX_IN, simplex_request(S=0, K=0)))[0] == -2          # K is checked before the empty return
    assert refusal(check, 'ewise', ewise_request((0, -1), (1, 1)))[0] == -2                      # every axis is checked before the empty return
