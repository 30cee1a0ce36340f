"""CPU test of the Cholesky family's plans (mxfusion_amd/csrc/chol_plan.h: plain C++, no HIP).  tests/host/chol_plan_check.cpp, built with the
system C++ compiler, prints the plan of every request it reads; what PotrfCall's stages and trtri's merge loop rely on is asserted here, and the
workload's own factorisations are pinned to what the launcher computed before the plan was split out of it."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NB, NBO, TRI_MIN = 64, 512, 1024
NS = (1, 5, 63, 64, 65, 128, 192, 512, 513, 576, 1024, 1100, 1536, 2048, 2100, 4608, 8192, 8256, 16384)


def req(esize, S, n, ncu=256, capturing=0, aux=0, inverse=0, zero_upper=1, one_max=512, split_rows=64, eager_panels=2):
    return ('potrf', esize, S, n, ncu, capturing, aux, inverse, zero_upper, one_max, split_rows, eager_panels)


SWEEP = [req(esize, S, n, ncu, cap, aux, inv, 1, one_max, split_rows, eager_panels)
         for n, S, esize, ncu, cap, aux, inv, split_rows, eager_panels, one_max
         in itertools.product(NS, (1, 2, 3, 64, 65), (4, 8), (64, 256, 304), (0, 1), (0, 1), (0, 1), (0, 2, 64), (0, 1, 2, 4), (0, 512))]

# (request as the launcher gathers it -- it asks about the capture and the streams only at n >= 2048 --, the parent's row: chol_plan_check.cpp)
P8192 = '512 1 1024 1 1536 1 2048 1 2560 1 3072 1 3584 1 4096 1 4608 0 5120 0 5632 0 6144 0 6656 0 7168 0 7680 0 8192 0'      # panel_end split
PINNED = [
    (req(8, 1, 1024, zero_upper=0), '- 0 1 0 0 0 64 1024 2 512 0 1024 0'),                    # the SVGP's Kuu: two tile launches, no streams asked for
    (req(8, 1, 8192, aux=1, inverse=1),                                                        # exact GP: eager, row blocks of 1024, eight panels split
     '- 1 1 0 1 1 64 1024 16 ' + P8192 + ' 0 0 1024 1 0 2048 0 1024 2048 1 1024 3072 0 2048 3072 1 2048 4096 0 3072 4096 1 3072 5120 0 4096 5120 1 4096 6144 '
     '0 5120 6144 1 5120 7168 0 6144 7168 1 6144 8192 0 7168 8192 1 7168 0'),
    (req(8, 1, 8192, capturing=1, inverse=1), '- 1 1 0 0 0 64 1024 16 ' + P8192),              # ... while capturing: no look-ahead, no eager inverse
    (req(8, 1, 4608, aux=1), '- 1 1 0 1 0 64 1024 9 512 1 1024 0 1536 0 2048 0 2560 0 3072 0 3584 0 4096 0 4608 0'),
    (req(8, 2, 2048, aux=1), '- 1 1 0 1 0 64 1024 4 512 0 1024 0 1536 0 2048 0'),
    (req(8, 2, 513), '- 0 0 0 0 0 64 1024 2 512 0 513 0'),                                     # ragged: the column form
    (req(4, 1, 1024), '- 0 0 0 0 0 64 1024 2 512 0 1024 0'),                                   # float32: the column form
    (req(8, 1, 8192, ncu=64, aux=1, inverse=1),                                                # 128 block rows on 64 CUs: the column form, look-ahead only
     '- 1 0 0 1 0 64 1024 16 512 0 1024 0 1536 0 2048 0 2560 0 3072 0 3584 0 4096 0 4608 0 5120 0 5632 0 6144 0 6656 0 7168 0 7680 0 8192 0'),
]


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('chol_plan') / 'chol_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'chol_plan_check.cpp'), '-o', exe], check=True)

    def run(rows):
        text = '\n'.join(' '.join(str(v) for v in r) for r in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split('\n')
        assert len(out) == len(rows)
        return out
    return run


def test_potrf_plan_invariants(plans):
    seen = set()
    for r, line in zip(SWEEP, plans(SWEEP)):
        _, esize, S, n, ncu, cap, aux, inv, _, one_max, split_rows, eager_panels = r
        t = line.split()
        what = '%r: %s' % (r, line)
        assert t[0] == '-', what
        may_look, tiles, one, look, eager, srows, rbw, npanels = (int(v) for v in t[1:9])
        v = [int(x) for x in t[9:]]
        ends, split = v[0:2 * npanels:2], v[1:2 * npanels:2]
        assert len(v) == (5 if eager else 2) * npanels, what
        # the implications PotrfCall's stages rely on (the comment above PotrfPlan), and the launcher's: streams only where look-ahead is possible
        assert not one or tiles, what
        assert not tiles or (esize == 8 and n % NB == 0 and n // NB * S <= ncu), what
        assert may_look == (n >= 2048 and not one), what
        assert look == (may_look and aux and not cap), what
        assert not eager or (look and tiles and S == 1 and inv and eager_panels > 0), what
        assert not eager or (n % NBO == 0 and n >= 16 * NBO and n >= 4 * rbw and rbw == eager_panels * NBO), what
        assert srows == split_rows, what
        # the panels cover [0, n) exactly
        assert ends[-1] == n and all(a < b for a, b in zip([0] + ends, ends)), what
        for c0, pe, sp in zip([0] + ends, ends, split):
            assert one or pe - c0 <= NBO, what
            assert not tiles or (c0 % NB == 0 and pe % NB == 0), what
            assert sp == (tiles and split_rows > 0 and (n - pe) // NB >= split_rows), what       # (so split => panel_tiles)
        if eager:
            e = v[2 * npanels:]
            fires, start, nxt = e[0::3], e[1::3], e[2::3]
            assert fires[-1], what
            firing = [pe for pe, f in zip(ends, fires) if f]
            for pe, nf in zip(ends[:-1], nxt):
                assert nf == min(q for q in firing if q > pe), what      # the FIRST firing point in (pe, n]
            covered = 0
            for pe, f, s0 in zip(ends, fires, start):
                if f:
                    assert s0 == covered and s0 < pe, what
                    covered = pe
            assert covered == n, what
        seen.add((tiles, one, look, eager, any(split)))
    # the sweep reaches every form: the column form with and without look-ahead, one launch, tile panels with and without look-ahead and the
    # split, the eager inverse
    assert seen >= {(0, 0, 0, 0, False), (0, 0, 1, 0, False), (1, 1, 0, 0, False), (1, 0, 0, 0, False), (1, 0, 0, 0, True), (1, 0, 1, 0, False),
                    (1, 0, 1, 0, True), (1, 0, 1, 1, True), (1, 0, 1, 1, False)}


def test_potrf_plan_pinned_rows(plans):
    for (r, want), got in zip(PINNED, plans([r for r, _ in PINNED])):
        assert got == want, (r, got)


def test_refusals(plans):
    # one matrix row per grid.y slot of the pass that zeroes the upper triangle: refused by the plan, before anything is queued
    got = plans([req(8, 1, 65536, aux=1), req(8, 1, 65536, aux=1, zero_upper=0), ('trtri', 65536), ('trtri', 65535)])
    assert got[0] == 'n too large' and got[1].startswith('- 1 0 0 1 0 ') and got[2] == 'n too large' and got[3].startswith('- 10 '), got


def test_trtri_levels(plans):
    """The merge levels on 64-row block indices: every merge finds its two diagonal sub-blocks complete, writes an off-diagonal block nothing has
    written, and the last level leaves every block on or below the diagonal written exactly once."""
    for n, line in zip(NS, plans([('trtri', n) for n in NS])):
        t = line.split()
        assert t[0] == '-', (n, line)
        v = [int(x) for x in t[2:]]
        assert len(v) == 5 * int(t[1]), (n, line)
        nblk = -(-n // NB)
        done = {(i, i) for i in range(nblk)}           # level 0: the diagonal blocks

        def merge(r0, r1, r2):                         # block rows [r0, r1) and [r1, r2) -> the inverse of [r0, r2)
            for a, b in ((r0, r1), (r1, r2)):
                assert all((i, j) in done for i in range(a, b) for j in range(a, i + 1)), (n, line, r0, r1, r2)
            off = {(i, j) for i in range(r1, r2) for j in range(r0, r1)}
            assert off and not (off & done), (n, line, r0, r1, r2)
            done.update(off)

        for bs, pairs, ragged_at, b2, tri in zip(v[0::5], v[1::5], v[2::5], v[3::5], v[4::5]):
            assert bs % NB == 0 and tri == (bs >= TRI_MIN), (n, line)
            w = bs // NB
            assert pairs * 2 * bs <= n
            for p in range(pairs):
                merge(2 * p * w, 2 * p * w + w, 2 * p * w + 2 * w)
            if b2:
                assert 0 < b2 < bs and ragged_at == pairs * 2 * bs and ragged_at + bs + b2 == n, (n, line)
                merge(ragged_at // NB, ragged_at // NB + w, nblk)
        assert done == {(i, j) for i in range(nblk) for j in range(i + 1)}, (n, line)
