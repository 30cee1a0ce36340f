"""Backward error of mxf_potrf, mxf_trsm, mxf_trtri and mxf_sumlogdiag on the GPU at the conditioning a GP gives them, in both dtypes, against
LAPACK on the same operand (tests/_chol_ref.py has the families, the metrics and LAPACK's side; tests/test_chol_ref_host.py checks that
side on the CPU).

Shapes: the smallest that reach each form of csrc/chol_plan.h, S in {1, 3}:
    n = 1, 5, 64, 65, 200    potrf_panel_kernel once per 64 columns (ragged n, n < 128, all of float32), the identity padding of
                             solve_cols_kernel and trtri_diag_kernel
    n = 128, 512             potrf_tiles_kernel in one launch, at its smallest and at one_max
    n = 576                  potrf_tiles_kernel in panel form: panels of 512 + 64 columns, one trailing update; S = 3 is 27 workgroups
    n = 1088 (S = 1, f64)    three panels, two trailing updates; trtri's triangular-aware merge (a ragged pair at bs = 1024 = TRI_MIN)
Every rung of the rbf ladder at n in {65, 128, 576}, the middle rung elsewhere; graded at n in {200, 576}; easy at every n but 1088.
trsm: nrhs in {1, 3, 257} (257: a second workgroup of 256 columns), both transposes, L per sample and L shared over S through stride 0
(above n = 200 the 257-column group per sample only), once on LAPACK's factor (test_trsm) and once on the kernel's own inside the chain (test_potrf).

Bars: metric_gpu <= C max(metric_lapack, u) for eta, omega, the chain and trtri over cond_1(L); trtri over |L|_F |X|_F is printed for every
case and held to its C on the easy family only; sumlogdiag <= (log2 n + 4) u relative to sum |log l_ii| (_chol_ref.sld_bar has the
derivation from the kernel's summation order).  The constants do NOT depend on the family or the rung: that is the property under test.
They are the next power of two at or above four times the worst ratio metric_gpu / max(metric_lapack, u) of ONE run over the easy family
(every easy case below), capped at 64:

    metric                     worst ratio, float64              worst ratio, float32             4 x worst    C
    eta (potrf)                3.56  (n = 512, S = 3)            4.93  (n = 576, S = 3)           19.7         32
    omega (trsm)               1.25  (n = 64, L^T, L shared)     1.11  (n = 64, L)                5.0          8
    chain                      0.69  (n = 200, S = 3)            0.80  (n = 64, S = 3)            3.2          4
    trtri / cond_1(L)          0.29  (n = 1)                     0.23  (n = 1)                    1.15         2
    trtri / |L|_F |X|_F        0.29  (n = 1)                     0.23  (n = 1)                    1.15         2

(LAPACK's own trtri residuals are below u on the easy family, so both trtri floors are u there and the kernel's inverse is itself within
0.3 u of either unit.)  The same run on the other families, for the record: rbf eta 3.28 (f64) and 7.08 (f32), omega 1.30, chain 0.66,
trtri / cond_1(L) 0.54; graded eta 1.53 (f64) and 10.6 (f32); at n = 576, S = 1, float64 the three rungs (cond_1(A) 4e5, 6e8, 2e9) give
eta 1.79, 1.68, 1.71 and the chain 0.32, 0.12, 0.08 of their floors: independent of the rung as measured.  sumlogdiag: at most 0.21 of its bar.

Every test prints the ratio of each metric to the floor of its bar, max(LAPACK's value, u); `worst` lines give the ratio to the bar itself."""
import numpy as np
import pytest
import torch

import _chol_ref as R

if not R.LONGDOUBLE_OK:
    pytest.skip('long double is no wider than double here', allow_module_level=True)

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [R.case_id(c) for c in CASES]
TORCH = {'f64': torch.float64, 'f32': torch.float32}


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=TORCH[dt]).cuda()


def _host(t):
    return t.cpu().numpy().astype(np.float64)


class Worst:
    """collects metric / bar, prints every figure, asserts at the end so that one run shows all of a case's ratios"""

    def __init__(self, case):
        self.case, self.rows = R.case_id(case), []
        print()

    def add(self, what, got, bar, floor=None):
        self.rows.append((what, got / bar))
        print('ratio %-40s %-34s got %.3g%s bar %.3g  got/bar %.3g' % (
            self.case, what, got, '' if floor is None else '  floor %.3g  got/floor %.3g' % (floor, got / floor), bar, got / bar))

    def note(self, what, got, floor):
        print('ratio %-40s %-34s got %.3g  floor %.3g  got/floor %.3g  (printed, not held)' % (self.case, what, got, floor, got / floor))

    def check(self):
        what, worst = max(self.rows, key=lambda r: r[1])
        print('worst %-40s %-34s %.3g' % (self.case, what, worst))
        bad = [r for r in self.rows if not r[1] <= 1.0]
        assert not bad, bad


def _held(w, metric, what, got, ref, dt):
    floor = max(ref, R.EPS[dt])
    w.add(what, got, R.C[metric] * floor, floor)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_potrf_sumlogdiag_and_the_chain(case):
    """the kernel's own factor: eta, a clean upper triangle, info == 0; its log-determinant; and alpha = L^-T (L^-1 y) by two trsm_ calls on it"""
    from mxfusion_amd import ops
    family, n, rung, S, dt = case
    A, Y, ref = R.operand(case), R.rhs(case)[:, :, :1], R.lapack_potrf_metrics(case)
    L, info = ops.potrf_(_dev(A, dt))
    assert info.cpu().tolist() == [0] * S, info.cpu().tolist()       # (no case can break down within the bar: tests/test_chol_ref_host.py)
    sld = _host(ops.sumlogdiag(L))
    alpha = _host(ops.trsm_(L, ops.trsm_(L, _dev(Y, dt)), transpose=True))
    Lh = _host(L)
    assert np.isfinite(Lh).all() and np.isfinite(alpha).all()
    assert np.all(np.triu(Lh, 1) == 0), 'the strict upper triangle of the factor is not exactly zero'
    w = Worst(case)
    _held(w, 'eta', 'potrf eta', max(R.eta(A[s], Lh[s], R.HI[dt]) for s in range(S)), ref['eta'], dt)
    w.add('sumlogdiag of the kernel\'s factor', max(R.sld_error(Lh[s], sld[s], R.HI[dt]) for s in range(S)), R.sld_bar(n, dt))
    _held(w, 'chain', 'chain residual', max(R.chain_residual(A[s], alpha[s], Y[s], R.HI[dt]) for s in range(S)), ref['chain'], dt)
    w.check()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_trsm(case):
    """LAPACK's factor as the operand (so operand and reference are identical), both transposes, the three widths; L per sample and shared"""
    from mxfusion_amd import ops
    family, n, rung, S, dt = case
    L, B = R.lapack_factor(case).astype(np.float64), R.rhs(case)
    w = Worst(case)
    for shared in ((False, True) if S > 1 else (False,)):
        Ld = _dev(L[:1] if shared else L, dt)
        for trans in (False, True):
            got = 0.0
            for at, k in R.rhs_groups():
                if shared and at + k > R.shared_columns(n):
                    continue
                Bk = B[:, :, at:at + k]
                X = _host(ops.trsm_(Ld, _dev(Bk, dt), transpose=trans))
                assert np.isfinite(X).all()
                got = max([got] + [R.omega(L[0 if shared else s], X[s], Bk[s], trans, R.HI[dt]) for s in range(S)])
            _held(w, 'omega', 'trsm omega %s%s' % ('L^T' if trans else 'L', ', L shared' if shared else ''), got,
                  R.lapack_omega(case, trans, shared), dt)
    w.check()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_trtri_and_sumlogdiag(case):
    """LAPACK's factor as the operand: both residuals of the inverse in the forward unit (held) and in the backward-stable unit (held on
    the easy family), a clean upper triangle; and the log-determinant of the same operand"""
    from mxfusion_amd import ops
    family, n, rung, S, dt = case
    L, ref = R.lapack_factor(case).astype(np.float64), R.lapack_trtri_metrics(case)
    Ld = _dev(L, dt)
    X, sld = _host(ops.trtri(Ld)), _host(ops.sumlogdiag(Ld))
    assert np.isfinite(X).all()
    assert np.all(np.triu(X, 1) == 0), 'the strict upper triangle of the inverse is not exactly zero'
    got = {}
    for s in range(S):
        for k, v in R.trtri_residuals(L[s], X[s], R.HI[dt]).items():
            got[k] = max(got.get(k, 0.0), v)
    w = Worst(case)
    print('cond_1(L) %.3g' % ref['cond1'])
    for side in ('left', 'right'):
        _held(w, 'trtri', 'trtri %s / cond_1(L)' % side, got[side + '_fwd'], ref[side + '_fwd'], dt)
        if family == 'easy':
            _held(w, 'trtri_bwd', 'trtri %s / |L||X|' % side, got[side + '_bwd'], ref[side + '_bwd'], dt)
        else:
            w.note('trtri %s / |L||X|' % side, got[side + '_bwd'], max(ref[side + '_bwd'], R.EPS[dt]))
    w.add('sumlogdiag of LAPACK\'s factor', max(R.sld_error(L[s], sld[s], R.HI[dt]) for s in range(S)), R.sld_bar(n, dt))
    w.check()
