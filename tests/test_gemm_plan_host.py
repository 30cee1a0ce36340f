"""CPU test of the dense GEMM's launch plan (mxfusion_amd/csrc/gemm_plan.h: plain C++, no HIP).  tests/host/gemm_plan_check.cpp, built with the
system C++ compiler, prints the plan of every shape it reads; the invariants the kernels rely on are asserted here, and the workload's own shapes
are pinned to what the launcher computed before the plan was split out of it."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL, DMA, GENERIC = 0, 1, 2
NONE, UPPER, LOWER = 0, 1, 2
KMAX = 16384                               # MXF_GEMM_SMALL_KMAX as shipped

MN = (1, 64, 65, 128, 130, 1024, 1152, 2048, 8192)
KS = (0, 1, 33, 127, 128, 255, 256, 4100, 131072, 2097152)
# (ta, tri) as a caller may pass them; the last two are hints in the orientation they do not describe, which the launcher drops
TA_TRI = ((0, NONE), (1, NONE), (1, UPPER), (0, LOWER), (0, UPPER), (1, LOWER))


def row(elem, M, N, K, ta=0, batch=1, lower=0, reserve=0, tri=NONE, vec=1, beta=0.0, kmax=KMAX):
    return (elem, ta, M, N, K, batch, lower, reserve, tri, vec, vec, beta, kmax)


# lower_only is legal on a square output only
SWEEP = [row(elem, M, N, K, ta, batch, lower, reserve, tri, vec, beta)
         for elem, M, N, K, batch in itertools.product((4, 8), MN, MN, KS, (1, 3))
         for lower in ((0, 1) if M == N else (0,)) for ta, tri in TA_TRI for reserve in ((0, 16, 148, 202) if (ta, tri) in TA_TRI[:4] else (0,))
         for vec, beta in ((1, 0.0), (0, 1.0), (1, 0.5))]

# (request, plan of the launcher before the split): kernel tm tn ntiles splitk kchunk atomic nwg xc_max rev_m prescale
PINNED = [
    (row(8, 1024, 1024, 1024), (SMALL, 16, 16, 256, 4, 256, 1, 1024, 0, 0, 1)),                                # float64 M x M core product
    (row(8, 1024, 1024, 131072, ta=1, lower=1, reserve=148), (DMA, 8, 8, 36, 3, 43712, 1, 108, 0, 1, 1)),      # Psi2 phase A: the small kernel steps aside
    (row(4, 1024, 131072, 1024), (GENERIC, 8, 1024, 8192, 1, 1024, 0, 8192, 0, 1, 0)),                         # float32 T = H0 Kuf
    (row(8, 8192, 8192, 8192, ta=1, lower=1, tri=UPPER, beta=1.0), (DMA, 64, 64, 2080, 1, 8192, 0, 2304, 288, 1, 0)),   # exact GP, -P/2 L^-T L^-1: balanced grid
    (row(8, 7680, 7680, 512, lower=1, beta=1.0), (DMA, 60, 60, 1830, 1, 512, 0, 1830, 0, 1, 0)),               # potrf(8192): trailing update after the first panel
    (row(8, 1936, 1936, 1936, ta=1, lower=1, tri=UPPER), (GENERIC, 16, 16, 136, 1, 1952, 0, 192, 24, 1, 0)),   # the smallest balanced grid, ragged
]

# lower_only on a non-square output at a size the small kernel declines; 65536 rows with split-K and a pre-scale (512 tile rows are as many as
# the most slots there are, so only a caller that lends CUs, reserve_cus < 0, gets this far); a grid past 2^31 - 1
REFUSED = [(row(8, 8192, 1024, 256, lower=1), -2, 'lower_only needs a square output'),
           (row(4, 65536, 64, 4096, reserve=-256), -3, 'split-K path needs M<=65535'),
           (row(4, 2 ** 23, 2 ** 23, 1), -3, 'grid too large')]


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('gemm_plan') / 'gemm_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'gemm_plan_check.cpp'), '-o', exe], check=True)

    def run(rows):
        text = '\n'.join(' '.join(repr(v) if isinstance(v, float) else str(v) for v in r) for r in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split('\n')
        assert len(out) == len(rows)
        return [[int(t) for t in line.split()[:13]] + [' '.join(line.split()[13:])] for line in out]
    return run


def test_plan_invariants(plans):
    rows = SWEEP + [r for r, _ in PINNED]
    seen = set()
    for req, got in zip(rows, plans(rows)):
        elem, ta, M, N, K, batch, lower, reserve, tri_in, vecA, vecB, beta, kmax = req
        kernel, tm, tn, ntiles, splitk, kchunk, atomic, nwg, xc_max, rev_m, prescale, tri, rc, refusal = got
        what = '%r: %r' % (req, got)
        assert tri == (tri_in if (tri_in == UPPER and ta) or (tri_in == LOWER and not ta) else NONE), what
        assert (rc, refusal) == (0, '-'), what
        bm, bk = (64, 16) if kernel == SMALL else (128, 32)
        assert tm * bm >= M > (tm - 1) * bm and tn * bm >= N > (tn - 1) * bm, what
        assert ntiles == (tm * (tm + 1) // 2 if lower else tm * tn), what
        if K > 0:
            assert kchunk % bk == 0 and splitk * kchunk >= K > (splitk - 1) * kchunk, what
        else:
            assert splitk == 1, what
        assert atomic == int(splitk > 1), what
        assert tri == NONE or splitk == 1, what
        assert prescale == int(atomic and beta != 1.0), what
        if xc_max > 0:
            assert lower and tri == UPPER and splitk == 1 and tm >= 16, what
            assert nwg == 8 * xc_max * batch, what
            per_xcd = [sum(r + 1 for r in range(x, tm, 8)) for x in range(8)]         # row r of the triangle has r + 1 tiles
            assert max(per_xcd) == xc_max, what
        else:
            assert not (lower and tri == UPPER and splitk == 1 and tm >= 16 and kernel != SMALL), what
            assert nwg == ntiles * batch * splitk, what
        assert 0 < nwg <= 2 ** 31 - 1, what
        t128 = -(-M // 128) * -(-N // 128) * batch
        if kernel == DMA:
            assert elem == 8 and vecA and vecB and M % 128 == 0 and N % 128 == 0 and K % 16 == 0 and kchunk % 16 == 0, what
        if kernel == SMALL:
            assert elem == 8 and t128 <= 64 and M <= 65535, what
            assert not (K > kmax and tri == NONE and M >= 512 and N >= 512), what
            assert (xc_max, rev_m) == (0, 0), what
        else:
            assert rev_m == 1, what
        seen.add((elem, kernel, bool(xc_max), atomic))
    # the sweep reaches every kernel in both split forms, and the balanced grid
    assert seen >= {(8, SMALL, False, 0), (8, SMALL, False, 1), (8, DMA, False, 0), (8, DMA, False, 1), (8, DMA, True, 0), (8, GENERIC, False, 0),
                    (8, GENERIC, False, 1), (8, GENERIC, True, 0), (4, GENERIC, False, 0), (4, GENERIC, False, 1), (4, GENERIC, True, 0)}


def test_plan_pinned_rows(plans):
    for (req, want), got in zip(PINNED, plans([r for r, _ in PINNED])):
        assert tuple(got[:11]) == want and got[12:] == [0, '-'], (req, got)


def test_plan_refusals(plans):
    got = plans([r for r, _, _ in REFUSED])
    assert [(g[12], g[13]) for g in got] == [(rc, why) for _, rc, why in REFUSED]
