"""The reference side of tests/test_gpu_chol_backward_error.py, checked on the CPU (no GPU): tests/_chol_ref.py's families, metrics and
LAPACK's own figures on every case the GPU test runs.

1. LAPACK stays inside every bar of the GPU test on every case in both dtypes.  The bars of eta, omega, the chain and trtri are C times
   LAPACK's own value (floored at u), so what is asserted here is what those floors rest on: LAPACK's figures are of the size theory gives
   them -- eta <= gamma_{n+1} <= (n + 2) u (Higham, Accuracy and Stability, Thm 10.3, with |L||L^T|_ij <= sqrt(a_ii a_jj)), omega <= n u
   (Thm 8.5), the chain <= 4 (n + 1) u, trtri within 8 of its forward unit cond_1(L) u -- and numpy's sumlogdiag is inside (log2 n + 4) u.
   Every figure is printed in units of u.
2. No breakdown: lambda_min(A) >= 4 C_eta u |A|_F for every case (eigvalsh in float64; C_eta and u of the dtype the case runs in), so a
   factorisation within the eta bar cannot meet a non-positive pivot and info != 0 on the GPU is a failure of the kernel, never a property
   of the input.  For the graded family the condition is stated on H = D^-1 A D^-1 scaled to a unit diagonal: eta is invariant under the
   scaling and bounds the perturbation of H entry by entry, while lambda_min(D A D) <= 1e-8 (1 + jitter) by construction (its last
   diagonal entry), below 4 C u |A|_F for any jitter in float32.  The float32 ladder is chosen so that the condition holds at the cap C = 64.
   cond_1(A) at S = 1, rbf family (the test prints every case's):
        f64   n = 65: 78, 1.8e4, 4.1e7      n = 128: 2.0e3, 1.4e6, 3.6e8      n = 576: 4.0e5, 5.9e8, 2.2e9
        f32   n = 65: 1.8e2, 1.0e3, 1.1e3    n = 128: 5.4e2, 3.5e3, 3.1e3      n = 576: 6.6e3, 1.9e4, 1.6e4
3. The metrics see what np.allclose(L, L_lapack, rtol=1e-11, atol=1e-11) cannot: three degraded copies of LAPACK's float64 factor of the
   (1.0, 1e-6) rung at n = 576 fail the float64 eta bar, the first of them while passing that allclose."""
import numpy as np
import pytest

import _chol_ref as R

if not R.LONGDOUBLE_OK:
    pytest.skip('long double is no wider than double here', allow_module_level=True)

CASES = R.cases()
IDS = [R.case_id(c) for c in CASES]


def test_cases_cover_the_table():
    ns = {(c[1], c[4]) for c in CASES}
    assert ns == {(n, dt) for n in (1, 5, 64, 65, 128, 200, 512, 576) for dt in ('f64', 'f32')} | {(1088, 'f64')}
    for dt in ('f64', 'f32'):
        for n in (65, 128, 576):
            assert {c[2] for c in CASES if c[0] == 'rbf' and c[1] == n and c[4] == dt} == set(R.LADDER[dt])
        assert {c[1] for c in CASES if c[0] == 'graded' and c[4] == dt} == {200, 576}
        assert {c[1] for c in CASES if c[0] == 'easy' and c[4] == dt} >= {200, 576}
        assert {c[3] for c in CASES if c[4] == dt and c[1] != 1088} == {1, 3}
    assert [c for c in CASES if c[1] == 1088] == [('rbf', 1088, (1.0, 1e-6), 1, 'f64')]
    assert all(1.0 <= c <= R.C_CAP for c in R.C.values())


def test_families_are_pure_symmetric_and_graded_is_a_scaling():
    for fam, rung in (('rbf', (1.0, 1e-6)), ('graded', (1.0, 1e-6)), ('easy', None)):
        A = R.matrix(fam, 65, rung, 3)
        R.matrix.cache_clear()
        B = R.matrix(fam, 65, rung, 3)
        assert A.dtype == np.float64 and A.shape == (3, 65, 65) and np.array_equal(A, B) and np.array_equal(A, np.swapaxes(A, 1, 2))
        assert not np.array_equal(A[0], A[1])
    d = 10.0 ** np.linspace(0, -4, 65)
    assert np.allclose(R.matrix('graded', 65, (1.0, 1e-6), 1)[0], d[:, None] * R.matrix('rbf', 65, (1.0, 1e-6), 1)[0] * d[None, :], rtol=1e-15, atol=0)
    c32 = ('rbf', 65, R.MIDDLE['f32'], 1, 'f32')
    assert np.array_equal(R.operand(c32), R.operand(c32).astype(np.float32).astype(np.float64))


def test_triangular_products_match_the_full_ones():
    rng = np.random.default_rng(0)
    for n in (1, 5, 64, 65, 200):
        L, X, B = [a.astype(np.longdouble) for a in (np.tril(rng.standard_normal((n, n))), np.tril(rng.standard_normal((n, n))), rng.standard_normal((n, 3)))]
        assert np.allclose(R.lower_llt(L), np.tril(L @ L.T), rtol=1e-13, atol=1e-13)
        assert np.allclose(R.lower_product(X, L), X @ L, rtol=1e-13, atol=1e-13)
        assert np.allclose(R.lower_apply(L, B, False), L @ B, rtol=1e-13, atol=1e-13)
        assert np.allclose(R.lower_apply(L, B, True), L.T @ B, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_lapack_is_inside_every_bar(case):
    family, n, rung, S, dt = case
    u = R.EPS[dt]
    p, t = R.lapack_potrf_metrics(case), R.lapack_trtri_metrics(case)
    om = {(tr, sh): R.lapack_omega(case, tr, sh) for tr in (False, True) for sh in ((False, True) if S > 1 else (False,))}
    print('lapack %-40s cond_1(L) %.3g | in u: eta %.3g  chain %.3g  omega %s  trtri/cond_1 left %.3g right %.3g  trtri/|L||X| left %.3g right %.3g'
          '  sld %.3g of its bar %.3g' % (R.case_id(case), t['cond1'], p['eta'] / u, p['chain'] / u, ' '.join('%.3g' % (v / u) for v in om.values()),
                                         t['left_fwd'] / u, t['right_fwd'] / u, t['left_bwd'] / u, t['right_bwd'] / u, p['sld'] / u, R.sld_bar(n, dt) / u))
    assert p['eta'] <= (n + 2) * u
    assert p['chain'] <= 4 * (n + 1) * u
    assert max(om.values()) <= max(n, 2) * u
    assert max(t['left_fwd'], t['right_fwd']) <= 8 * u
    assert p['sld'] <= R.sld_bar(n, dt)
    # ... and with room to spare inside the bars themselves: the ratio the GPU test would print for LAPACK's own result is at most 1 of C
    for metric, v in (('eta', p['eta']), ('chain', p['chain']), ('omega', max(om.values())), ('trtri', t['left_fwd']), ('trtri', t['right_fwd']),
                      ('trtri_bwd', t['left_bwd']), ('trtri_bwd', t['right_bwd'])):
        assert R.ratio(metric, v, v, dt) <= 1.0 <= R.C[metric]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_no_breakdown_within_the_bar(case):
    family, n, rung, S, dt = case
    A = R.operand(case)
    worst = np.inf
    for s in range(S):
        H = A[s]
        if family == 'graded':
            d = np.sqrt(np.diagonal(H))
            H = H / (d[:, None] * d[None, :])
        need = 4 * R.C['eta'] * R.EPS[dt] * np.linalg.norm(H)
        worst = min(worst, np.linalg.eigvalsh(H)[0] / need)
    print('margin %-40s cond_1(A) %.3g  lambda_min / (4 C u |A|_F) %.3g' % (R.case_id(case), max(np.linalg.cond(A[s], 1) for s in range(S)), worst))
    assert worst >= 1.0


def test_degraded_factors_fail_the_new_bar_and_one_passes_the_old():
    case = ('rbf', 576, (1.0, 1e-6), 1, 'f64')
    A, L = R.operand(case)[0], np.array(R.lapack_factor(case)[0])
    bar = R.C['eta'] * max(R.lapack_potrf_metrics(case)['eta'], R.EPS['f64'])
    cap = R.C_CAP * max(R.lapack_potrf_metrics(case)['eta'], R.EPS['f64'])
    old = lambda M: np.allclose(M, L, rtol=1e-11, atol=1e-11)
    a = L.copy()                                    # (a) one 64 x 64 tile below the diagonal perturbed by 1e-12 |tile|
    a[64:128, 0:64] += 1e-12 * np.abs(a[64:128, 0:64])
    b = np.linalg.cholesky(A.astype(np.float32)).astype(np.float64)          # (b) the factor computed in float32 and widened
    c = L.copy()                                    # (c) the panel rows below the first diagonal block as A21 inv(L11)^T, inv rounded to float32
    c[64:, :64] = A[64:, :64] @ np.linalg.inv(L[:64, :64]).astype(np.float32).astype(np.float64).T
    assert old(L) and R.eta(A, L, np.longdouble) <= bar
    for name, M in (('a', a), ('b', b), ('c', c)):
        e = R.eta(A, M, np.longdouble)
        print('degraded (%s): eta %.3g = %.3g of the bar, %.3g of the bar at the cap C = %g; old allclose %s' % (name, e, e / bar, e / cap, R.C_CAP, old(M)))
        assert e > cap >= bar, name
    assert old(a) and not old(b)
