"""CPU test of the forward Gram launch plans (mxfusion_amd/csrc/gram_plan.h: plain C++, no HIP).  tests/host/gram_plan_check.cpp, built with the system
C++ compiler, prints the plan of every request it reads; the invariants the kernels rely on are asserted here over a sweep, and the workload's own
shapes are pinned to what the launcher computed before the plan was split out of it."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENERIC, COORD_FAST, COORD_SLOW, LEAN, LEAN_XF = range(5)
CEN_NONE, CEN_X, CEN_X2 = range(3)
RBF, MATERN12, MATERN32, MATERN52, LINEAR, BIAS, WHITE = range(7)
WRITE, ACC_ADD, ACC_MUL = range(3)
# columns of a Gram plan as gram_plan_check prints it
(PATH, QT, TR, NCB, GX, GY, GZ, PADR, PADC, PADX, SX, SZ, CENTRE, SCEN, XS, ZS, XN, ZN, SXS, SZS, SXN, SZN, BYTES, HAS_DIAG, RC) = range(25)
# ... and of a request
(R_KIND, R_ELEM, R_S, R_N, R_N2, R_Q, R_SQUARE, R_SX, R_SX2, R_SLS, R_VEC, R_MODE, R_DIAG) = range(13)

NS = (1, 11, 12, 13, 63, 64, 65, 255, 256, 257, 1028, 1031, 65536)
QS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 20)


def gram_row(kind, elem, N, N2=0, Q=8, S=1, square=1, sX=0, sX2=0, sls=0, vec=1, mode=WRITE, diag=0):
    return (kind, elem, S, N, N2, Q, square, sX, sX2, sls, vec, mode, diag)


def sweep(elem, kind):
    """every (S, N, N2, Q, mode, vec) with each combination of shared / sampled X, X2, ls; a square Gram has no N2 and no X2.  As request text."""
    rows = []
    for S, Q, mode, vec in itertools.product((1, 3), QS, (WRITE, ACC_ADD, ACC_MUL), (1, 0)):
        head, tail = 'G %d %d %d ' % (kind, elem, S), ' %d %d 0' % (vec, mode)
        for N, sx, sl in itertools.product(NS, (0, 1), (0, 1)):
            rows.append('%s%d 0 %d 1 %d 0 %d%s' % (head, N, Q, sx * N * Q, sl * Q, tail))
            rows += ['%s%d %d %d 0 %d %d %d%s' % (head, N, N2, Q, sx * N * Q, sx2 * N2 * Q, sl * Q, tail) for N2 in NS for sx2 in (0, 1)]
    return '\n'.join(rows)


# (request, plan of the launcher before the split), printed by a transcription of the launcher's arithmetic as it stood before gram_plan.h; None: the
# launcher formed no such value on that path (no norms outside LEAN_XF, no diagonal flags outside the lean kernel)
PINNED = [
    # the benchmark's roofline Gram, float32 RBF N = 65536, Q = 8 ... and in float64
    (gram_row(RBF, 4, 65536), (LEAN, 8, 12, 256, 256, 5462, 1, 65536, 65536, 65536, 1, 1, CEN_X, 0, 0, 0, None, None, 0, 0, 0, 0, 2097152, 0)),
    (gram_row(RBF, 8, 65536), (LEAN_XF, 8, 16, 512, 512, 4096, 1, 65536, 65536, 65536, 1, 1, CEN_X, 0, 0, 0, 524288, 524288, 0, 0, 0, 0, 4718592, 2)),
    # the SVGP step's Kuu: float64, M = 1024, square with jitter
    (gram_row(RBF, 8, 1024, diag=1), (LEAN_XF, 8, 16, 8, 8, 64, 1, 1024, 1024, 1024, 1, 1, CEN_X, 0, 0, 0, 8192, 8192, 0, 0, 0, 0, 73728, 3)),
    # float32 k(Z, X): M = 1024 x SB = 131072
    (gram_row(RBF, 4, 1024, 131072, square=0), (LEAN, 8, 12, 512, 512, 86, 1, 1024, 131072, 1024, 1, 1, CEN_X, 0, 0, 8192, None, None, 0, 0, 0, 0, 4227072, 0)),
    # slow path: N2 = 1031 accumulated into, Matern 5/2, three samples of X against a shared X2
    (gram_row(MATERN52, 4, 257, 1031, Q=5, S=3, square=0, sX=1285, mode=ACC_ADD),
     (COORD_SLOW, 8, 64, 5, 25, 1, 3, 320, 2048, 320, 3, 1, CEN_X2, 0, 0, 7680, None, None, 2560, 0, 320, 0, 96256, None)),
    # generic: Q = 20
    (gram_row(MATERN32, 8, 300, 300, Q=20, square=0), (GENERIC, 0, 0, 0, 2, 300, 1, 0, 0, 0, 0, 0, CEN_NONE, 0, 0, 0, None, None, 0, 0, 0, 0, 0, None)),
]
# planes request (R, Kn, Q, fused, has_w, Pw, kb) -> QT padr padk kbpb grid.x grid.y PT bytes
PINNED_PLANES = [
    ((131072, 1024, 8, 0, 0, 0, 8), (8, 131072, 1024, 8, 2048, 8, 0, 4227072)),        # the SVGP step's Kfu planes, plain
    ((131072, 1024, 8, 1, 1, 1, 8), (8, 131072, 1024, 64, 2048, 1, 1, 4227072)),       # ... and with the fused row, one output
    ((1024, 131072, 8, 0, 0, 0, 8), (8, 1024, 131072, 8, 16, 1024, 0, 4227072)),       # the Kuf planes
]


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('gram_plan') / 'gram_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'gram_plan_check.cpp'), '-o', exe], check=True)

    def run(tag, rows, ncol):
        """rows: request tuples, or request text -> (int64 array of the numeric columns, list of refusal texts)"""
        text = rows if isinstance(rows, str) else '\n'.join(tag + ' ' + ' '.join(map(str, r)) for r in rows)
        n = text.count('\n') + 1
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
        assert out.count('\n') == n
        if out.count(' -\n') == n:      # no refusal anywhere: the numeric columns in one go
            return np.fromstring(out.replace(' -\n', '\n'), dtype=np.int64, sep=' ').reshape(n, ncol), ['-'] * n
        out = out.strip().split('\n')
        why = [line.split(' ', ncol)[ncol] for line in out]
        return np.array([line.split(' ', ncol)[:ncol] for line in out], dtype=np.int64), why
    return run


def holds(cond, req, got, what):
    bad = np.flatnonzero(~cond)
    assert bad.size == 0, '%s: %d rows, first request %r -> plan %r' % (what, bad.size, req[bad[0]].tolist(), got[bad[0]].tolist())


@pytest.mark.parametrize('elem', (4, 8))
def test_gram_plan_invariants(plans, elem):
    seen = set()
    for kind in range(7):
        text = sweep(elem, kind)
        req = np.fromstring(text.replace('G', ''), dtype=np.int64, sep=' ').reshape(-1, 13)
        p, why = plans('G', text, 25)
        chk = lambda cond, what: holds(cond, req, p, what)
        S, N, Q, square, vec, mode = (req[:, c] for c in (R_S, R_N, R_Q, R_SQUARE, R_VEC, R_MODE))
        N2 = np.where(square == 1, N, req[:, R_N2])
        sX, sls = req[:, R_SX], req[:, R_SLS]
        sX2 = np.where(square == 1, sX, req[:, R_SX2])
        VEC = 16 // elem
        flat = kind in (BIAS, WHITE)
        chk(p[:, RC] == 0, 'no refusal in the sweep')
        assert set(why) == {'-'}
        # path
        gen = Q > 16
        chk((p[:, PATH] == GENERIC) == gen, 'generic iff Q > 16')
        chk(~gen | ((p[:, BYTES] == 0) & (p[:, QT] == 0)), 'the generic path takes no scratch')
        rows = 12 if (kind == RBF and elem == 4) else (16 if kind == RBF else 64)
        c = ~gen
        chk(gen | (p[:, TR] == rows), 'rows per workgroup')
        rblocks = -(-N // rows)
        lean = c & (mode == WRITE) & (vec == 1) & (N2 % VEC == 0) & (not flat) & (rblocks <= 65535)
        chk(np.isin(p[:, PATH], (LEAN, LEAN_XF)) == lean, 'lean rule')
        chk((p[:, PATH] == LEAN_XF) == (lean & (elem == 8) & (kind == RBF)), 'expansion form: lean, float64, RBF')
        fast = c & (mode == WRITE) & (vec == 1) & (N2 % VEC == 0)
        chk(lean | gen | ((p[:, PATH] == COORD_FAST) == fast), 'coordinate kernel: fast iff whole 16-byte overwrites')
        qt = np.full_like(Q, 2) if flat else np.select([Q <= 2, Q <= 4, Q <= 8], [2, 4, 8], 16)
        chk(gen | (p[:, QT] == qt), 'QT')
        # grids: within the hardware limits, and covering the output
        chk((p[:, GX] >= 1) & (p[:, GX] <= 2 ** 31 - 1) & (p[:, GY] >= 1) & (p[:, GY] <= 65535) & (p[:, GZ] == S) & (S <= 65535), 'grid limits')
        chk(~gen | ((p[:, GX] * 256 >= N2) & ((p[:, GX] - 1) * 256 < N2) & (p[:, GY] == np.minimum(N, 65535))), 'generic grid (rows strided over grid.y)')
        cw = 64 * VEC
        chk(gen | ((p[:, NCB] * cw >= N2) & ((p[:, NCB] - 1) * cw < N2)), 'column blocks cover N2')
        lp = np.isin(p[:, PATH], (LEAN, LEAN_XF))
        chk(~lp | ((p[:, GX] == p[:, NCB]) & (p[:, GY] == rblocks)), 'lean grid')
        cp = np.isin(p[:, PATH], (COORD_FAST, COORD_SLOW))
        chk(~cp | ((p[:, GX] == p[:, NCB] * rblocks) & (p[:, GY] == 1)), 'coordinate kernel grid')
        # bias / white: no coordinates, no scratch
        if flat:
            chk(p[:, BYTES] == 0, 'bias and white take no scratch')
            chk(~np.isin(p[:, PATH], (LEAN, LEAN_XF)), 'bias and white are never lean')
        else:
            # padding
            chk(gen | ((p[:, PADR] % 64 == 0) & (p[:, PADR] >= N) & (p[:, PADR] - 64 < N)), 'padr')
            chk(gen | ((p[:, PADC] % (4 * cw) == 0) & (p[:, PADC] >= N2) & (p[:, PADC] - 4 * cw < N2)), 'padc')
            chk(gen | (p[:, PADX] == np.where(square == 1, np.maximum(p[:, PADR], p[:, PADC]), p[:, PADR])), 'padx')
            # sample copies
            chk(gen | (p[:, SX] == np.where((sX == 0) & (sls == 0), 1, S)), 'Sx == 1 iff X and ls are shared (else one copy per sample)')
            chk(gen | (p[:, SZ] == np.where((sX2 == 0) & (sls == 0), 1, S)), 'Sz likewise')
            chk(gen | ((p[:, SXS] == 0) == (p[:, SX] == 1)) & ((p[:, SZS] == 0) == (p[:, SZ] == 1)), 'a coordinate sample stride is 0 exactly when its count is 1')
            chk(gen | ((p[:, SXN] == 0) == (p[:, SX] == 1)) & ((p[:, SZN] == 0) == (p[:, SZ] == 1)), 'a norm sample stride is 0 exactly when its count is 1')
            chk(gen | ((p[:, SX] == 1) | ((p[:, SXS] == p[:, PADX] * p[:, QT]) & (p[:, SXN] == p[:, PADX]))), 'x sample strides')
            chk(gen | (square == 1) | (p[:, SZ] == 1) | ((p[:, SZS] == p[:, PADC] * p[:, QT]) & (p[:, SZN] == p[:, PADC])), 'z sample strides')
            # centring
            want = np.full_like(Q, CEN_NONE) if kind == LINEAR else np.where((square == 0) & (sX != 0) & (sX2 == 0), CEN_X2, CEN_X)
            chk(gen | (p[:, CENTRE] == want), 'centring choice')
            chk(gen | (p[:, SCEN] == np.where(p[:, CENTRE] == CEN_X, sX, 0)), 'centre stride')
            # scratch: xs | zs | xn | zn in order, no overlap, ending at the byte total; a square Gram has no z regions; norms only with LEAN_XF
            xf = p[:, PATH] == LEAN_XF
            sq = square == 1
            nx = p[:, SX] * p[:, PADX] * p[:, QT]
            nz = np.where(sq, 0, p[:, SZ] * p[:, PADC] * p[:, QT])
            nxn = np.where(xf, p[:, SX] * p[:, PADX], 0)
            nzn = np.where(xf & ~sq, p[:, SZ] * p[:, PADC], 0)
            chk(gen | ((p[:, XS] == 0) & (p[:, ZS] == np.where(sq, p[:, XS], nx))), 'coordinate regions')
            chk(gen | ~xf | ((p[:, XN] == nx + nz) & (p[:, ZN] == np.where(sq, p[:, XN], p[:, XN] + nxn))), 'norm regions')
            chk(gen | (p[:, BYTES] == (nx + nz + nxn + nzn) * elem), 'the regions end at the byte total')
            chk(gen | ~sq | ((p[:, ZS] == p[:, XS]) & (p[:, SZS] == p[:, SXS]) & (p[:, SZN] == p[:, SXN])), 'a square Gram reads the x copy in both roles')
        seen |= set(np.unique(p[:, PATH]).tolist())
    # the sweep reaches all five paths in this dtype (LEAN_XF exists in float64 only, where RBF has no plain LEAN)
    assert seen >= ({GENERIC, COORD_FAST, COORD_SLOW, LEAN} | ({LEAN_XF} if elem == 8 else set()))


def test_gram_plan_diag_flags(plans):
    req = np.array([gram_row(kind, elem, N, N2, square=sq, diag=d) for kind, elem, N, N2, sq, d in
                    itertools.product((RBF, MATERN32, LINEAR), (4, 8), (64, 1028), (64, 256), (0, 1), (0, 1))], dtype=np.int64)
    p, _ = plans('G', req, 25)
    lean = np.isin(p[:, PATH], (LEAN, LEAN_XF))
    assert lean.all()
    # bit 0: a diagonal term exists; bit 1: the expansion form of a square Gram sets k(x, x) = variance before it adds the term
    holds(p[:, HAS_DIAG] == (req[:, R_DIAG] | 2 * ((p[:, PATH] == LEAN_XF) & (req[:, R_SQUARE] == 1))), req, p, 'diagonal flags')


def test_gram_plan_pinned_rows(plans):
    p, why = plans('G', [r for r, _ in PINNED], 25)
    for (req, want), got, w in zip(PINNED, p.tolist(), why):
        assert [g for g, x in zip(got[:24], want) if x is not None] == [x for x in want if x is not None] and got[24] == 0 and w == '-', (req, got)


def test_gram_plan_refusal(plans):
    # 2^24 x 2^24 float32: 2^16 column blocks x 1.4 M row blocks do not fit one grid.x; the check precedes the choice of the lean grid, as it always did
    p, why = plans('G', [gram_row(RBF, 4, 2 ** 24, 2 ** 24, square=0)], 25)
    assert (p[0, RC], why[0]) == (-3, 'problem too large for one launch')


def test_planes_plan(plans):
    req = [(R, Kn, Q, fused, fused, Pw, kb) for R, Kn, Q, (fused, Pw), kb in
           itertools.product((1, 63, 64, 65, 127, 128, 129, 1024, 131072), (1, 15, 16, 17, 255, 256, 257, 1024, 131072, 2 ** 24 + 5, 2 ** 27), (1, 2, 8, 9, 16),
                             ((0, 0), (1, 1), (1, 2), (1, 8)), (1, 8, 64))]
    p, why = plans('P', req, 9)
    req = np.array(req, dtype=np.int64)
    R, Kn, Q, fused, Pw, kb = (req[:, c] for c in (0, 1, 2, 3, 5, 6))
    qt, padr, padk, kbpb, gx, gy, pt, nbytes, rc = (p[:, c] for c in range(9))
    chk = lambda cond, what: holds(cond, req, p, what)
    K16 = -(-Kn // 16)
    chk(rc == 0, 'no refusal')
    chk(qt == np.where(Q <= 8, 8, 16), 'QT')
    chk((padr % 128 == 0) & (padr >= R) & (padr - 128 < R), 'padr: whole pairs of 64-row blocks')
    chk((padk % 256 == 0) & (padk >= Kn) & (padk - 256 < Kn), 'padk: whole groups of sixteen k blocks')
    chk(nbytes == (padr + padk) * qt * 4, 'scratch bytes')
    chk((gx * 64 >= R) & ((gx - 1) * 64 < R) & (gx <= 2 ** 31 - 1), 'grid.x covers the rows')
    chk((gy >= 1) & (gy <= 65535) & (gy * kbpb >= K16) & ((gy - 1) * kbpb < K16), 'grid.y covers the k blocks')
    chk((fused == 0) | ((gy == 1) & (kbpb == K16)), 'a fused row walks every k block in one workgroup')
    doubled = kbpb // kb
    chk((fused == 1) | ((kbpb == kb * doubled) & ((doubled & (doubled - 1)) == 0) & ((doubled == 1) | (-(-K16 // np.maximum(kbpb // 2, 1)) > 65535))),
        'k blocks per workgroup: the knob, doubled only as often as grid.y needs')
    chk(pt == np.where(fused == 0, 0, np.where(Pw == 1, 1, 8)), 'PT by Pw')
    assert (doubled > 1).any()


def test_planes_plan_pinned_and_refusals(plans):
    p, why = plans('P', [r for r, _ in PINNED_PLANES], 9)
    for (req, want), got, w in zip(PINNED_PLANES, p.tolist(), why):
        assert tuple(got[:8]) == want and got[8] == 0 and w == '-', (req, got)
    p, why = plans('P', [(100, 100, 17, 0, 0, 0, 8), (100, 100, 3, 1, 0, 1, 8), (100, 100, 3, 1, 1, 9, 8)], 9)
    assert list(zip(p[:, 8].tolist(), why)) == [(-3, 'Q > 16 not supported'), (-3, 'fused w^T K needs w and P <= 8'), (-3, 'fused w^T K needs w and P <= 8')]
    # the scratch size is the same function of (R, Kn, Q) whatever else is asked: mxf_gram_planes_scratch_bytes is this plan's byte count
    assert p[0, 7] == (128 + 256) * 16 * 4 and p[1, 7] == (128 + 256) * 8 * 4
