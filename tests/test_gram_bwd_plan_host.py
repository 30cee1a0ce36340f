"""CPU test of the launch plans of the Gram reverse passes (mxfusion_amd/csrc/gram_bwd_plan.h: plain C++, no HIP).  tests/host/gram_bwd_plan_check.cpp,
built with the system C++ compiler, prints the plan of every shape it reads; the invariants the kernels rely on are asserted here, and two rows
are pinned to what the launchers computed before the plans were split out of them."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = [(N, N2, S, QT, PT, elem, kb, 4096)
         for N, N2, S, QT, PT, elem, kb in itertools.product((1, 64, 65, 1024, 8192), (1, 257, 1024, 100000), (1, 300), (2, 8, 16), (0, 1, 8),
                                                             (4, 8), (30, 80))]
PLAIN_TOO_LARGE = [(64 * 65536, 257, 1, 16, 8, 8, 30, 4096), (64, 257, 65536, 2, 0, 4, 30, 4096)]
PLAIN_PINNED = (1024, 1024, 1, 8, 0, 8, 30, 4096)         # float64 M x M core Gram

MFMA_MS, MFMA_SBS = (20, 128, 144, 1024), (16, 208, 1040, 2097152)
# B: one sample, and the smaller whole-sample splits with B % 16 == 0 (at most 65535 samples)
MFMA = [(M, SB, B, 1024) for M in MFMA_MS for SB in MFMA_SBS for B in sorted({SB, SB // 13, SB // 32, 16}) if B > 0 and B % 16 == 0 and SB % B == 0 and SB // B <= 65535]
MFMA_PINNED = (1024, 2097152, 2097152 // 4, 1024)
# more than 2^31 - 4096 columns; samples that do not tile the columns, or more than 65535 of them; more than 65535 row bands
MFMA_REFUSED = [((128, 2 ** 31, 2 ** 20, 1024), 'more than 2^31 columns'), ((128, 208, 48, 1024), 'bad sample layout'), ((128, 208, 0, 1024), 'bad sample layout'),
                ((128, 16 * 65536, 16, 1024), 'bad sample layout'), ((128 * 65536, 1040, 1040, 1024), 'too many row bands')]


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('gram_bwd_plan') / 'gram_bwd_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'gram_bwd_plan_check.cpp'), '-o', exe], check=True)

    def run(tag, rows):
        text = '\n'.join(tag + ' ' + ' '.join(str(v) for v in row) for row in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split('\n')
        assert len(out) == len(rows)
        return [[int(t) for t in line.split()] if tag == 'g' else [int(t) for t in line.split()[:14]] + [' '.join(line.split()[14:])] for line in out]
    return run


def test_plain_plan_invariants(plans):
    rows = PLAIN + PLAIN_TOO_LARGE
    for (N, N2, S, QT, PT, elem, kb, target), got in zip(rows, plans('g', rows)):
        rb, ct, gx, rblocks, gz, lds, too_large = got
        what = 'N %d N2 %d S %d QT %d PT %d elem %d, %d KB: %r' % (N, N2, S, QT, PT, elem, kb, got)
        assert rb % 64 == 0 and rb >= 64, what
        assert rblocks * rb >= N and (rblocks - 1) * rb < N, what                # the bands cover the rows, none is empty
        assert 1 <= ct <= 64 and gx * ct * 256 >= N2 and (gx - 1) * ct * 256 < N2, what
        assert gz == S, what
        fixed = (64 * QT + 64 * PT + 16) * elem + 16 * 8 + 64                   # the staged tile of 64 rows, 16 + 16 reduction words, slack
        assert lds == rb * (QT + PT) * elem + fixed, what
        assert lds <= kb * 1024 or rb == 64, what                               # inside the budget unless one tile of rows is already over it
        assert too_large == int(rblocks > 65535 or S > 65535), what
    assert [g[-1] for g in plans('g', PLAIN_TOO_LARGE)] == [1, 1]


def test_plain_plan_pinned_row(plans):
    rb, ct, gx, gy, gz, lds, too_large = plans('g', [PLAIN_PINNED])[0]
    assert (rb, ct, (gx, gy, gz), lds, too_large) == (64, 1, (4, 16, 1), 8512, 0)


def test_mfma_plan_invariants(plans):
    assert {r[0] for r in MFMA} == set(MFMA_MS) and {r[1] for r in MFMA} == set(MFMA_SBS)
    rows = MFMA + [MFMA_PINNED]
    for (M, SB, B, target), got in zip(rows, plans('m', rows)):
        ct, gx, bands, gz, full = got[:5]
        what = 'M %d SB %d B %d: %r' % (M, SB, B, got)
        assert got[14] == '-', what
        assert bands * 128 >= M and (bands - 1) * 128 < M and gz == 1, what
        assert 1 <= ct <= 256 and gx * ct * 64 >= SB and (gx - 1) * ct * 64 < SB, what
        assert full == int(M % 128 == 0 and SB % 64 == 0), what
        _check_scratch(M, SB, got[5:14], what)


def _check_scratch(M, SB, offsets, what):
    zacc, dls3, mx, centre, Zs, Xs, Xn, zero_bytes, total_bytes = offsets
    regions = sorted([(zacc, M * 16 * 8), (dls3, 8 * 8), (mx, 2 * 4), (centre, 8 * 4), (Zs, M * 8 * 4), (Xs, SB * 8 * 4), (Xn, SB * 4)])
    for (o0, n0), (o1, _) in zip(regions, regions[1:]):
        assert o0 + n0 <= o1, what
    assert regions[0][0] >= 0 and regions[-1][0] + regions[-1][1] <= total_bytes, what
    for o, n in ((zacc, M * 16 * 8), (dls3, 64), (mx, 8)):                        # the accumulators and the bound words are cleared on every call
        assert o + n <= zero_bytes, what
    assert zero_bytes <= Zs, what                                                  # ... and the clear stops short of the coordinates
    assert zacc % 8 == 0 and dls3 % 8 == 0 and mx % 4 == 0 and centre % 4 == 0, what
    assert Zs % 16 == 0 and Xs % 16 == 0 and Xn % 16 == 0, what                  # read as 16-byte vectors
    # the layout the launcher placed by hand before: accumulators, dls3, two bound words, the centre one double behind them, then the coordinates
    assert (zacc, dls3, mx, centre) == (0, M * 128, M * 128 + 64, M * 128 + 72), what
    assert (zero_bytes, Zs, Xs, Xn, total_bytes) == (M * 128 + 128, M * 128 + 128, M * 160 + 128, M * 160 + 128 + SB * 32, M * 160 + 128 + SB * 36), what


def test_mfma_plan_pinned_row(plans):
    ct, gx, gy, gz, full = plans('m', [MFMA_PINNED])[0][:5]
    assert (ct, (gx, gy, gz), full) == (256, (128, 8, 1), 1)


def test_mfma_plan_refusals(plans):
    got = plans('m', [row for row, _ in MFMA_REFUSED])
    assert [g[14] for g in got] == [why for _, why in MFMA_REFUSED]
