"""CPU test of the SVGP composite's plan (mxfusion_amd/csrc/svgp_plan.h: plain C++, no HIP).  tests/host/svgp_plan_check.cpp, built with the
system C++ compiler, prints the plan, the Psi2 / Phi / V schedule and the scratch byte count of every request it reads; what SvgpCall's stages
rely on is asserted here, mxf_svgp_whitened_ok is compared with the formula it had before it became a question to the plan, and the
workload's own calls are pinned to what the launcher computed before the plan was split out of it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLS = ('rc use_mat ysamp het_stream het fused use_split whiten bt_path bt_wh het_split SS SYc lsn SB pl_big pl_h0 gp_scr t_blocked '
        'KA reserve_a reserve_b few reserve_v reserve_phi bytes whitened_ok').split()
# the axes of the sweep, in the checker's order (sX? / sY?: shared or the contiguous stride; noise: (1,1) (B,1) (1,P) (B,P) bad)
AXES = dict(esize=(4, 8), kind=(0,), S=(1, 2, 4), sx=(0, 1), sy=(0, 1), B=(16, 48, 256, 272, 4096, 65536), M=(16, 64, 128, 144, 256, 384, 1024, 2048, 2304),
            Q=(1, 8, 9, 16, 17), P=(1, 2, 8, 9), noise=(0, 1, 2, 3, 4), grad=(0, 1), form=(0, 1), mat=(0, 1), x16=(1,))
# every kind and both alignments of X (they enter het_stream and t_blocked only) over the shapes around those two decisions
AXES_KIND = dict(AXES, kind=tuple(range(7)), x16=(0, 1), S=(1, 2), sx=(1,), sy=(0,), B=(16, 256, 272), M=(64, 128, 256), Q=(8, 9, 17), P=(1, 2), grad=(1,), mat=(0,))


@pytest.fixture(scope='module')
def check(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('svgp_plan') / 'svgp_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'svgp_plan_check.cpp'), '-o', exe], check=True)

    def run(text, rows):
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
        return np.fromstring(out, dtype=np.int64, sep=' ').reshape(rows, len(COLS))
    return run


def sweep(check, axes):
    """(request columns, plan columns) of the cross product, as dicts of int64 arrays"""
    text = 'sweep ' + ' '.join('%d %s' % (len(v), ' '.join(map(str, v))) for v in axes.values())
    grid = np.meshgrid(*[np.array(v, dtype=np.int64) for v in axes.values()], indexing='ij')
    r = {k: g.ravel() for k, g in zip(axes, grid)}
    out = check(text, r['B'].size)
    return r, {k: out[:, i] for i, k in enumerate(COLS)}


def parent_rules(r):
    """The launcher's plan() as it stood before svgp_plan.h, line for line on arrays: (rc, flags)."""
    f32, B, M, Q, P, S, grad = r['esize'] == 4, r['B'], r['M'], r['Q'], r['P'], r['S'], r['grad'] == 1
    sX, sY = r['sx'] * B * Q, r['sy'] * B * P
    nrows = np.where(r['noise'] == 4, B + 1, np.where(r['noise'] % 2 == 1, B, 1))
    ncols = np.where((r['noise'] == 2) | (r['noise'] == 3), P, 1)
    use_mat = r['mat'] == 1
    ysamp = (S > 1) & (sX == 0) & (sY != 0)
    SB = np.where(sX == 0, 1, S) * B
    bt_ok = (M % 256 == 0) & (SB % 256 == 0) & (M % 16 == 0) & (M >= 48)
    is_mfma = (r['kind'] == 0) & f32 & (P == 1) & (Q <= 8) & (SB % 4 == 0) & (SB >= 16) & (B % 16 == 0) & (r['x16'] == 1)
    het_stream = (f32 & grad & (nrows == B) & (nrows > 1) & (ncols == 1) & (P == 1) & ~use_mat & ~ysamp & (Q <= 8) & (B % 16 == 0) & (M % 16 == 0) & (M >= 128)
                  & (r['form'] == 0) & is_mfma)
    het = ((nrows > 1) | (ncols > 1) | use_mat | ysamp | (Q > 16)) & ~het_stream
    fused = grad & ~het
    use_split = fused & f32 & (SB % 16 == 0) & (M % 16 == 0) & (M >= 128) & (Q <= 16)
    whiten = f32 & grad & (r['form'] == 1)
    rc = np.zeros_like(B)
    for cond, code in ((whiten & ~(use_split & (M % 128 == 0) & (SB % 256 == 0)), -3), ((S > 1) & (sX == 0) & (sY == 0), -3),
                       (((nrows != 1) & (nrows != B)) | ((ncols != 1) & (ncols != P)), -2), (P > 8, -3)):      # the first check that fires wins: applied last
        rc = np.where(cond, code, rc)
    flags = dict(use_mat=use_mat, ysamp=ysamp, het_stream=het_stream, het=het, fused=fused, use_split=use_split, whiten=whiten,
                 bt_path=use_split & ~whiten & ~het_stream & (P == 1) & (M <= 2048) & bt_ok, bt_wh=whiten & (P == 1) & (M <= 2048) & bt_ok,
                 het_split=het & f32 & grad & bt_ok & (M * SB >= 1 << 24), SB=SB)
    return rc, flags


@pytest.fixture(scope='module')
def swept(check):
    return {'shapes': sweep(check, AXES), 'kinds': sweep(check, AXES_KIND)}


@pytest.mark.parametrize('which', ['shapes', 'kinds'])
def test_plan_invariants_and_parent_rules(swept, which):
    r, p = swept[which]
    want_rc, want = parent_rules(r)
    assert np.array_equal(p['rc'], want_rc), 'refusal codes differ at rows %s' % np.flatnonzero(p['rc'] != want_rc)[:5]
    ok = p['rc'] == 0
    assert ok.any() and (~ok).any()
    f32, grad, M, P, SB = (r['esize'] == 4)[ok], (r['grad'] == 1)[ok], r['M'][ok], r['P'][ok], p['SB'][ok]
    q = {k: v[ok].astype(bool) if k in COLS[1:11] + ['few'] else v[ok] for k, v in p.items()}
    for k, v in want.items():
        assert np.array_equal(q[k], v[ok]), k

    def implies(a, b):
        return bool(np.all(~a | b))
    # the comment above SvgpPlan
    assert implies(q['use_split'], f32 & grad & ~q['het'] & (SB % 16 == 0))
    assert implies(q['whiten'], q['use_split']) and implies(q['bt_path'], q['use_split'] & ~q['whiten']) and implies(q['bt_wh'], q['whiten'])
    assert implies(q['het_stream'], ~q['het'] & f32) and implies(q['het_split'], q['het'] & f32)
    assert np.array_equal(q['fused'], grad & ~q['het'])
    # ... and what the stages rely on besides
    assert not np.any(q['bt_path'] & q['bt_wh'])
    assert implies(q['whiten'], (M % 128 == 0) & (SB % 256 == 0))
    assert implies(q['t_blocked'] == 1, q['use_split'])
    assert np.array_equal(q['pl_big'], (SB + 15) // 16 * M * 16) and np.array_equal(q['pl_h0'], (M + 15) // 16 * M * 16)
    KA = q['KA']
    assert np.all((0 <= KA) & (KA <= SB) & ((KA % 32 == 0) | (KA == SB)))
    for k in ('reserve_a', 'reserve_b', 'reserve_v', 'reserve_phi'):
        assert np.all((0 <= q[k]) & (q[k] <= 256)), k
    assert np.all(q['bytes'] % 256 == 0) and np.all(q['bytes'] > 0)
    if which == 'shapes':      # the sweep reaches every flag
        for k in COLS[1:11]:
            assert q[k].any() and not q[k].all(), k


def test_whitened_ok_is_the_old_formula(swept):
    r, p = swept['shapes']
    S, B, M, Q, P = r['S'], r['B'], r['M'], r['Q'], r['P']
    SB = np.where(r['sx'] == 0, 1, S) * B
    old = ((r['esize'] == 4) & (S > 0) & (B > 0) & (M % 128 == 0) & (M >= 128) & (SB % 256 == 0) & (Q <= 16) & (P <= 8) & ~((S > 1) & (r['sx'] == 0)))
    assert np.array_equal(p['whitened_ok'].astype(bool), old)
    # ... and it is the call's own verdict: a whitened training call with (1,1) noise and per-sample Y is accepted exactly there
    ask = (r['form'] == 1) & (r['grad'] == 1) & (r['noise'] == 0) & (r['sy'] == 1) & (r['mat'] == 0) & (r['esize'] == 4)
    assert np.array_equal((p['rc'] == 0)[ask], old[ask])


def req(esize, S, B, M, Q, P, sX, sY=0, nrows=1, ncols=1, ard=1, grad=1, mat=0, form=0, x16=1, kind=0, ka=-1, ra=148, ra_set=0, rb=16, rb_set=0):
    return 'plan ' + ' '.join(str(v) for v in (esize, kind, S, B, M, Q, P, sX, sY, nrows, ncols, ard, grad, mat, form, x16, ka, ra, ra_set, rb, rb_set))


N = 65536
# (request, the parent's row: its plan(), carve(), scratch() and kuf_psi2() / whiten_v_phi() arithmetic pasted into a stand-alone program).
# Columns as COLS without whitened_ok.
PINNED = [
    (req(4, 32, N, 1024, 8, 1, N * 8), '0 0 0 0 0 1 1 0 1 0 0 32 1 8 2097152 2147483648 1048576 134217728 1 0 214 32 0 0 0 34802428416'),             # the bench step
    (req(4, 32, N, 1024, 8, 1, N * 8, form=1), '0 0 0 0 0 1 1 1 0 1 0 32 1 8 2097152 2147483648 1048576 134217728 1 0 0 0 0 0 16 34873744128'),      # ... whitened
    (req(4, 4, N, 1024, 8, 1, N * 8), '0 0 0 0 0 1 1 0 1 0 0 4 1 8 262144 268435456 1048576 16777216 1 262144 214 32 0 0 0 4480755968'),               # 4 samples per rank
    (req(4, 4, N, 1024, 8, 1, N * 8, form=1), '0 0 0 0 0 1 1 1 0 1 0 4 1 8 262144 268435456 1048576 16777216 1 0 0 0 1 40 202 4493351424'),
    (req(4, 1, 131072, 512, 1, 2, 0, ard=0, mat=1), '0 1 0 0 1 0 0 0 0 0 1 1 1 1 131072 67108864 262144 0 0 0 0 0 0 0 0 1381558528'),                  # deep GP, first layer
    (req(4, 4, 8192, 1024, 8, 1, 8192 * 8, nrows=8192), '0 0 0 1 0 1 1 0 0 0 0 4 1 8 32768 33554432 1048576 2097152 1 32768 202 16 0 0 0 690641664'),  # (B,1) noise, streaming
    (req(4, 4, 8192, 1024, 8, 1, 8192 * 8, nrows=8192, x16=0), '0 0 0 0 1 0 0 0 0 0 1 4 1 8 32768 33554432 1048576 0 0 0 0 0 0 0 0 818469120'),       # ... X not 16-byte aligned
    (req(8, 4, N, 1024, 8, 1, N * 8), '0 0 0 0 0 1 0 0 0 0 0 4 1 8 262144 268435456 1048576 0 0 131072 148 16 0 0 0 6599936000'),                      # float64
]


def test_pinned_rows(check):
    got = check('\n'.join(r for r, _ in PINNED), len(PINNED))
    for (r, want), g in zip(PINNED, got):
        assert ' '.join(str(v) for v in g[:-1]) == want, (r, g)


def test_knobs_change_only_their_own_numbers(check):
    """MXF_SVGP_PSI2_KA moves KA alone; _RA the first launch's reserve alone (split forms: only when SET; dense form: always); _RB the second
    launch's (one-planes form: only when set) and the unset whitened Phi reserve at many samples."""
    shapes = dict(split=dict(esize=4, S=4, B=8192, M=1024, Q=8, P=2, sX=8192 * 8), planes1=dict(esize=4, S=32, B=N, M=1024, Q=8, P=1, sX=N * 8),
                  dense=dict(esize=8, S=4, B=N, M=1024, Q=8, P=1, sX=N * 8), white=dict(esize=4, S=32, B=N, M=1024, Q=8, P=1, sX=N * 8, form=1),
                  white_few=dict(esize=4, S=4, B=N, M=1024, Q=8, P=1, sX=N * 8, form=1))
    knobs = [dict(), dict(ka=4100), dict(ka=0), dict(ra=100), dict(ra=100, ra_set=1), dict(rb=24), dict(rb=24, rb_set=1)]
    got = check('\n'.join(req(**s, **k) for s in shapes.values() for k in knobs), len(shapes) * len(knobs)).reshape(len(shapes), len(knobs), -1)
    sched = slice(COLS.index('KA'), COLS.index('bytes'))
    for name, rows in zip(shapes, got):
        assert all(np.array_equal(rows[0, :sched.start], x[:sched.start]) and rows[0, -2] == x[-2] for x in rows), name      # the plan and the scratch never move
        base = dict(zip(COLS[sched], rows[0, sched]))
        for k, x in zip(knobs, rows):
            want = dict(base)
            if name in ('white', 'white_few'):
                if 'rb' in k and name == 'white': want['reserve_phi'] = 24
            else:
                if 'ka' in k: want['KA'] = {4100: 4096, 0: 0}[k['ka']]
                if 'ra' in k and (name == 'dense' or k.get('ra_set')): want['reserve_a'] = 100
                if 'rb' in k and (name != 'planes1' or k.get('rb_set')): want['reserve_b'] = 24
            assert dict(zip(COLS[sched], x[sched])) == want, (name, k)
    assert [dict(zip(COLS, g[0]))['reserve_a'] for g in got[:3]] == [202, 214, 148] and [dict(zip(COLS, g[0]))['reserve_b'] for g in got[:3]] == [16, 32, 16]
