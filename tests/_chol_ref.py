"""Host reference of the Cholesky family's backward-error tests (mxf_potrf, mxf_trsm, mxf_trtri, mxf_sumlogdiag): the matrix families, the
metrics in extended precision, and LAPACK's value of every metric on the same operand in the same dtype.  Plain module, no fixtures, numpy
(and scipy's triangular LAPACK routines where scipy imports); no GPU.  tests/test_chol_ref_host.py checks this side on the CPU,
tests/test_gpu_chol_backward_error.py holds the kernels to it.

Families (float64 arrays (S, n, n), a pure function of (family, n, rung, S); a float32 run and its reference both see `operand`, the
float32-rounded values):
    rbf      exp(-|x - x'|^2 / 2 l^2) + jitter I,  x ~ U(-2, 2)^3;  rung = (l, jitter)
    graded   D A D of the rbf matrix, D = diag(10^linspace(0, -4, n)): a Cholesky factor is invariant under this scaling up to rounding, so
             the family shows any ABSOLUTE error (atomics, a dropped small term)
    easy     G G^T / n + I  (cond < 10; rung = None): the matrices of tests/test_gpu_linalg.py, and the anchor of the constants C

Metrics (u = eps of the working dtype; residuals of float64 results in long double, of float32 results in float64):
    eta      potrf:  max_{i >= j} |A - L L^T|_ij / sqrt(a_ii a_jj)         scaled componentwise backward error, invariant under D A D;
                     LAPACK-style Cholesky holds eta <= gamma_{n+1} (|L||L^T|_ij <= sqrt(a_ii a_jj) by Cauchy-Schwarz)
    omega    trsm:   max_j |op(L) x_j - b_j|_inf / (|L|_inf |x_j|_inf + |b_j|_inf)         normwise backward error per column
    trtri    |X L - I|_F and |L X - I|_F, each divided by cond_1(L) (the forward-error unit is cond_1(L) u) and again by |L|_F |X|_F (the
             unit a backward-stable method holds, |L|_F |X|_F u)
    sld      |got - sum log l_ii| / sum |log l_ii|
    chain    alpha = L^-T (L^-1 y) from the factor under test by two solves:  |A alpha - y|_inf / (|A|_inf |alpha|_inf + |y|_inf)

The bar of a metric m is  m_gpu <= C[m] max(m_lapack, u): the form is derived, the constant C[m] is measured against LAPACK on the easy
family and is the same on every rung (header of tests/test_gpu_chol_backward_error.py)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

try:
    from scipy.linalg import lapack as _lapack, solve_triangular as _solve_triangular
except ImportError:          # numpy's general solvers then stand in for the triangular ones
    _lapack = _solve_triangular = None

try:        # the operands are small: BLAS threads only get in the way of the pool below (where threadpoolctl is absent they stay as they are)
    from threadpoolctl import threadpool_limits as _threadpool_limits
except ImportError:
    _threadpool_limits = None


def _one_blas_thread(fn):
    @functools.wraps(fn)
    def wrapped(*args):
        if _threadpool_limits is None:
            return fn(*args)
        with _threadpool_limits(limits=1, user_api='blas'):
            return fn(*args)
    return wrapped


# x87 extended (64-bit significand) or better; where long double is no wider than double the float64 residuals cannot be refereed, and the
# test modules skip themselves
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)

DTYPES = {'f64': np.float64, 'f32': np.float32}
HI = {'f64': np.longdouble, 'f32': np.float64}                   # the precision a dtype's residuals are computed in
EPS = {k: float(np.finfo(v).eps) for k, v in DTYPES.items()}

# (lengthscale, jitter), from the mildest to the hardest.  cond_1 at n = 576, S = 1 (tests/test_chol_ref_host.py prints every case's):
#   f64: 4e5, 6e8, 2e9.   f32: 7e3, 2e4, 2e4 -- the no-breakdown condition lambda_min >= 4 C u |A|_F with u = 1.2e-7 and |A|_F of 60 to 320 asks
#   for a jitter of 1e-2 and more at the cap C = 64, which the ladder is chosen for (margins of 5, 7 and 10 there).
LADDER = {'f64': ((0.5, 1e-4), (1.0, 1e-6), (2.2, 1e-6)),
          'f32': ((0.5, 1e-2), (1.0, 3e-2), (2.2, 1e-1))}
MIDDLE = {k: v[1] for k, v in LADDER.items()}
FAMILY_ID = {'rbf': 0, 'graded': 1, 'easy': 2}

# One constant per metric, the same on every family and rung; how they were measured is in the header of tests/test_gpu_chol_backward_error.py.
C = {'eta': 32.0, 'omega': 8.0, 'chain': 4.0, 'trtri': 2.0, 'trtri_bwd': 2.0}
C_CAP = 64.0


def case_id(case):
    family, n, rung, S, dt = case
    return '%s-n%d-%s-S%d-%s' % (family, n, 'x' if rung is None else 'l%g-j%g' % rung, S, dt)


def _rng(family, n, rung, S, salt=0):
    l, j = (0.0, 1.0) if rung is None else rung
    return np.random.default_rng([FAMILY_ID[family], n, S, int(round(l * 1000)), int(round(-np.log10(j) * 100)), salt])


def _sym(A):
    """the lower triangle mirrored: exactly symmetric, whichever triangle a routine reads"""
    T = np.tril(A)
    return T + np.swapaxes(np.tril(A, -1), -1, -2)


@functools.lru_cache(maxsize=None)
def matrix(family, n, rung, S):
    if family == 'easy':
        G = _rng(family, n, rung, S).standard_normal((S, n, n))
        return _sym(G @ np.swapaxes(G, 1, 2) / n + np.eye(n)[None])
    l, jitter = rung
    x = _rng('rbf', n, rung, S).uniform(-2, 2, (S, n, 3))
    d2 = ((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1)
    A = np.exp(-d2 / (2 * l * l)) + jitter * np.eye(n)[None]
    if family == 'graded':
        d = 10.0 ** np.linspace(0, -4, n)
        A = d[None, :, None] * A * d[None, None, :]
    return _sym(A)


def operand(case):
    """what the run of `case` factors: float64 values, float32-rounded for a float32 case"""
    family, n, rung, S, dt = case
    return matrix(family, n, rung, S).astype(DTYPES[dt]).astype(np.float64)


NRHS = (1, 3, 257)          # trsm: the right-hand sides of a case are one (S, n, 261) array, cut into these column groups


def rhs(case):
    family, n, rung, S, dt = case
    return _rng(family, n, rung, S, salt=1).standard_normal((S, n, sum(NRHS))).astype(DTYPES[dt]).astype(np.float64)


def rhs_groups():
    at = 0
    for k in NRHS:
        yield at, k
        at += k


# ---- extended-precision products of triangular operands, 64 x 64 blocks, only the blocks and the k range that are not zero ------------------
# numpy multiplies long doubles at ~0.15 Gflop/s without the GIL: the block rows go to four threads, and L L^T costs a sixth of the full product
_B = 64
_POOL = ThreadPoolExecutor(4)


def _blocks(n):
    return [(a, min(a + _B, n)) for a in range(0, n, _B)]


def _block_rows(n, row):
    """row(i0, i1) for every block row, the heavy (last) ones first"""
    list(_POOL.map(lambda b: row(*b), reversed(_blocks(n))))


def lower_llt(L):
    """tril(L L^T) for lower-triangular L, in L's dtype"""
    if L.dtype == np.float64:
        return np.tril(L @ L.T)          # (BLAS)
    n = L.shape[0]
    out = np.zeros_like(L)

    def row(i0, i1):
        for j0, j1 in _blocks(i1):
            out[i0:i1, j0:j1] = L[i0:i1, :j1] @ L[j0:j1, :j1].T
    _block_rows(n, row)
    return np.tril(out)


def lower_product(X, L):
    """X L for lower-triangular X and L (lower triangular again), in their dtype"""
    if L.dtype == np.float64:
        return np.tril(X @ L)
    n = L.shape[0]
    out = np.zeros_like(L)

    def row(i0, i1):
        for j0, j1 in _blocks(i1):
            out[i0:i1, j0:j1] = X[i0:i1, j0:i1] @ L[j0:i1, j0:j1]
    _block_rows(n, row)
    return np.tril(out)


def lower_apply(L, X, trans):
    """op(L) X for lower-triangular L and a dense X, in their dtype"""
    if L.dtype == np.float64:
        return (L.T if trans else L) @ X
    n = L.shape[0]
    out = np.empty_like(X)

    def row(i0, i1):
        out[i0:i1] = L[i0:, i0:i1].T @ X[i0:] if trans else L[i0:i1, :i1] @ X[:i1]
    _block_rows(n, row)
    return out


# ---- the metrics: one matrix (n, n) each, operands as float64 arrays, `hi` the precision of the residual ----------------------------------
def eta(A, L, hi):
    A, L = np.tril(A).astype(hi), np.tril(L).astype(hi)
    d = np.sqrt(np.diagonal(A))
    return float(np.max(np.abs(A - lower_llt(L)) / (d[:, None] * d[None, :])))


def omega(L, X, B, trans, hi):
    L, X, B = np.tril(L).astype(hi), X.astype(hi), B.astype(hi)
    R = np.abs(lower_apply(L, X, trans) - B).max(0)
    normL = np.abs(L).sum(0 if trans else 1).max()
    return float(np.max(R / (normL * np.abs(X).max(0) + np.abs(B).max(0))))


def cond1(L):
    L = np.tril(np.asarray(L, np.float64))
    Li = _solve_triangular(L, np.eye(L.shape[0]), lower=True) if _solve_triangular else np.linalg.inv(L)
    return float(np.abs(L).sum(0).max() * np.abs(Li).sum(0).max())


def trtri_residuals(L, X, hi):
    """{'left_fwd', 'right_fwd', 'left_bwd', 'right_bwd'}: |X L - I|_F (left) and |L X - I|_F (right) over cond_1(L) and over |L|_F |X|_F"""
    k = cond1(L)
    L, X = np.tril(L).astype(hi), np.tril(X).astype(hi)
    I = np.eye(L.shape[0], dtype=hi)
    fro = lambda M: float(np.sqrt((M * M).sum()))
    left, right, unit = fro(lower_product(X, L) - I), fro(lower_product(L, X) - I), fro(L) * fro(X)
    return {'left_fwd': left / k, 'right_fwd': right / k, 'left_bwd': left / unit, 'right_bwd': right / unit}


def sld_error(L, got, hi):
    logs = np.log(np.abs(np.diagonal(L)).astype(hi))
    return float(abs(hi(got) - logs.sum()) / np.abs(logs).sum())


def sld_bar(n, dt):
    """One rounding per logarithm (a 1-ulp log: u |log l_ii|) and a summation tree.  sumlogdiag_kernel (csrc/chol.hip) adds ceil(n / 256) - 1
    <= 4 terms in sequence per thread for n <= 1088, then a 64-lane butterfly (6 levels) and one over the four wave sums (2 levels): at most
    12 additions of u / 2 each on any term's path, 7 u in all -- below (log2 n + 4) u from n = 8 on; for n < 8 a single wave's butterfly adds
    ceil(log2 n) levels, (1 + log2(n) / 2) u.  So the tree-sum bar holds for this kernel as it stands."""
    return (np.log2(n) + 4) * EPS[dt]


def chain_residual(A, alpha, y, hi):
    A, alpha, y = A.astype(hi), alpha.astype(hi), y.astype(hi)
    return float(np.abs(A @ alpha - y).max() / (np.abs(A).sum(1).max() * np.abs(alpha).max() + np.abs(y).max()))


# ---- LAPACK on the same operand in the same dtype -------------------------------------------------------------------------------------------
def lapack_solve(L, B, trans):
    if _solve_triangular:
        return _solve_triangular(L, B, lower=True, trans=1 if trans else 0, check_finite=False)
    return np.linalg.solve(L.T if trans else L, B)


def lapack_trtri(L):
    if _lapack:
        X, info = _lapack.get_lapack_funcs('trtri', (L,))(L, lower=1)
        assert info == 0
        return np.tril(X)
    return np.tril(np.linalg.inv(L))


@functools.lru_cache(maxsize=None)
def lapack_factor(case):
    """LAPACK's factor of `operand(case)` in the case's dtype, (S, n, n); read-only"""
    L = np.linalg.cholesky(operand(case).astype(DTYPES[case[4]]))
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
@_one_blas_thread
def lapack_potrf_metrics(case):
    """{'eta', 'sld', 'chain'}: the worst over the case's samples of LAPACK's own figures (chain: the first right-hand side of `rhs`)"""
    dt = case[4]
    A, L, Y = operand(case), lapack_factor(case), rhs(case)[:, :, :1].astype(DTYPES[dt])
    out = {'eta': 0.0, 'sld': 0.0, 'chain': 0.0}
    for s in range(A.shape[0]):
        alpha = lapack_solve(L[s], lapack_solve(L[s], Y[s], False), True)
        got = {'eta': eta(A[s], L[s], HI[dt]), 'sld': sld_error(L[s], np.log(np.diagonal(L[s])).sum(dtype=DTYPES[dt]), HI[dt]),
               'chain': chain_residual(A[s], alpha, Y[s], HI[dt])}
        out = {k: max(out[k], got[k]) for k in out}
    return out


def shared_columns(n):
    """trsm with L shared over S: all of `rhs`'s columns up to n = 200, above that the groups of 1 and 3 (the 257-column group, whose second
    workgroup does not depend on the stride of L, runs per sample there: the long-double residual costs n^2 per column)"""
    return sum(NRHS) if n <= 200 else sum(NRHS[:2])


@functools.lru_cache(maxsize=None)
@_one_blas_thread
def lapack_omega(case, trans, shared):
    """the worst omega of LAPACK's triangular solve over the case's samples and `rhs`'s columns; shared: every sample against L[0], over
    shared_columns"""
    dt = case[4]
    L, B = lapack_factor(case), rhs(case).astype(DTYPES[dt])
    if shared:
        B = B[:, :, :shared_columns(case[1])]
    return max(omega(L[0 if shared else s], lapack_solve(L[0 if shared else s], B[s], trans), B[s], trans, HI[dt]) for s in range(B.shape[0]))


@functools.lru_cache(maxsize=None)
@_one_blas_thread
def lapack_trtri_metrics(case):
    """the worst of each of trtri_residuals' figures over the case's samples, for LAPACK's trtri of LAPACK's factor; and the worst cond_1(L)"""
    dt = case[4]
    L = lapack_factor(case)
    out = {}
    for s in range(L.shape[0]):
        got = dict(trtri_residuals(L[s], lapack_trtri(L[s]), HI[dt]), cond1=cond1(L[s]))
        out = {k: max(out.get(k, 0.0), v) for k, v in got.items()}
    return out


def ratio(metric, got, ref, dt):
    """got over the floor of its bar, max(LAPACK's value, u): the bar is ratio <= C[metric]"""
    return got / max(ref, EPS[dt])


# ---- the cases (tests/test_gpu_chol_backward_error.py has the table of forms) --------------------------------------------------------------
def cases():
    out = []
    for dt in ('f64', 'f32'):
        for n in (1, 5, 64, 65, 200, 128, 512, 576):
            rungs = LADDER[dt] if n in (65, 128, 576) else (MIDDLE[dt],)
            fams = [('rbf', r) for r in rungs] + [('easy', None)]
            if n in (200, 576):
                fams += [('graded', MIDDLE[dt])]
            out += [(f, n, r, S, dt) for f, r in fams for S in (1, 3)]
    out.append(('rbf', 1088, MIDDLE['f64'], 1, 'f64'))
    return out
