"""The host reference of the Gram reverse mode (tests/_gram_ref.py) checked on the CPU, so that the GPU tests that rest on it compare the
kernels with something known to be right: against autograd through the oracle (an independent derivation: expansion-form distance,
reverse-mode differentiation) and against a central finite difference of its own forward value.

Precision of the float64 comparisons: numpy.longdouble where it has a 64-bit significand (eps < 2e-19: x86); elsewhere _gram_ref.HI falls
back to float64 -- the one place that decides it is _gram_ref.LONGDOUBLE_OK, and test_longdouble_has_64_bit_significand says so loudly."""
import numpy as np
import pytest
import torch

import _gram_ref as R
from oracle import gp_oracle as O

OK = {'rbf': O.RBF, 'matern12': O.Matern12, 'matern32': O.Matern32, 'matern52': O.Matern52}


def test_longdouble_has_64_bit_significand():
    assert np.finfo(np.longdouble).eps < 2e-19, 'float64 results are refereed by a float64 reference on this machine (_gram_ref.HI)'
    assert R.LONGDOUBLE_OK and R.HI is np.longdouble


def _separated(seed, S, N, Q):
    """points on a jittered grid along the first coordinate: every pair at least 0.25 apart (before scaling; length-scales <= 1.8), so the
    oracle's expansion form x^2 - 2xz + z^2 keeps its digits and no pair is near the Matern clip"""
    rng = np.random.RandomState(seed)
    X = rng.uniform(-2, 2, (S, N, Q))
    for s in range(S):
        X[s, :, 0] = (rng.permutation(N) - N / 2) * 0.3 + rng.uniform(-0.02, 0.02, N)
    return X


def _oracle_grads(kind, X, X2, ls, var, dK, ard):
    S = dK.shape[0]
    k = OK[kind](X.shape[-1], ARD=ard)
    lv = [None if a is None else O.T(a).clone().requires_grad_(True) for a in (X, X2, ls, var)]
    ex = lambda t: None if t is None else t.expand((S,) + tuple(t.shape[1:]))
    K = k.K(ex(lv[0]), ex(lv[1]), **{k.name + '_lengthscale': ex(lv[2]), k.name + '_variance': ex(lv[3])})
    (K * O.T(dK)).sum().backward()
    return dict(zip(('dX', 'dX2', 'dls', 'dvar'), (None if t is None else t.grad.numpy() for t in lv)))


CASES = [(kind, ard, p) for kind in R.KINDS for ard in (True, False) for p in R.RECT_PATTERNS + R.SQUARE_PATTERNS]


@pytest.mark.parametrize('kind,ard,pattern', CASES, ids=['%s-%s-%s' % (k, 'ard' if a else 'iso', R.pattern_id(p)) for k, a, p in CASES])
def test_reference_equals_oracle_autograd(kind, ard, pattern):
    """every kind, ARD and isotropic, square and rectangular, every sample-axis pattern: 1e-10 of the absolute sum, per element"""
    S, N, N2, Q = 3, 9, 7, 3
    sx, sz, sl, sv = pattern
    X, X2, ls, var, dK = R.make_case(11, N, None if sz is None else N2, Q, ard, pattern, S=S)
    # well-separated: X and X2 are cut from one jittered grid, so cross pairs are apart as well
    both = _separated(5, max(X.shape[0], 1 if X2 is None else X2.shape[0]), N + N2, Q)
    X = both[:X.shape[0], :N]
    X2 = None if X2 is None else both[:X2.shape[0], N:]
    ref = _oracle_grads(kind, X, X2, ls, var, dK, ard)
    for dtype in (np.float64, R.HI):
        grad, scale = R.gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=dtype)
        for name in ('dX', 'dX2', 'dls', 'dvar'):
            if ref[name] is None:
                assert grad[name] is None
                continue
            assert grad[name].dtype == dtype and grad[name].shape == ref[name].shape
            err = np.abs(grad[name].astype(np.float64) - ref[name])
            assert (err <= 1e-10 * scale[name].astype(np.float64)).all(), (name, float((err / scale[name].astype(np.float64)).max()))


def test_reference_is_inside_the_gpu_bar_on_the_gpu_tests_inputs():
    """on uniform(-2, 2) inputs (close pairs included) the float64 evaluation of the reference agrees with the extended-precision one to a few
    roundoffs of the absolute sum: the reference's own error is far inside the bar of tests/test_gpu_gram_bwd_axes.py"""
    worst = 0.0
    for kind in R.KINDS:
        X, X2, ls, var, dK = R.make_case(3, 65, 257, 3, True, (True, True, True, True))
        lo, _ = R.gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=np.float64)
        hi, scale = R.gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=R.HI)
        for name in lo:
            worst = max(worst, R.worst_ratio(lo[name], hi[name], scale[name], 2.0 ** -53))
    assert worst < 8.0, worst


def _fd_case(kind, square):
    """9 rows with exact duplicates inside X; rectangular: the first rows of X2 are copies of rows of X (Z = X[:M])"""
    rng = np.random.RandomState(4)
    base = rng.uniform(-2, 2, (6, 2))
    X = np.concatenate([base, base[:2], base[:1]])[None]
    X2 = None if square else np.concatenate([X[0, :3], rng.uniform(-2, 2, (4, 2))])[None]
    ls, var = rng.uniform(0.8, 1.8, (1, 2)), rng.uniform(0.5, 1.5, (1, 1))
    dK = rng.randn(1, 9, 9 if square else 7)
    return X, X2, ls, var, dK


@pytest.mark.parametrize('square', [False, True], ids=['rect', 'square'])
@pytest.mark.parametrize('kind', R.KINDS)
def test_reference_equals_central_difference_of_its_forward(kind, square):
    """d/dθ sum(dK * K(θ)) by central differences of gram_ref in extended precision, at a duplicated row of X (zero distances: a Matern12 pair
    sits on its kink, where the symmetric difference is 0 like the clip convention's slope), a row of X2 copied from X, a length-scale and the
    variance.  h = 1e-6: truncation ~h^2, rounding ~eps / h -- 1e-8 of the absolute sum is far above both."""
    X, X2, ls, var, dK = _fd_case(kind, square)
    grad, scale = R.gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=R.HI)
    ops = dict(dX=X, dX2=X2, dls=ls, dvar=var)
    h = R.HI(1e-6)

    def value(name, idx, step):
        a = {k: None if v is None else np.asarray(v, dtype=R.HI).copy() for k, v in ops.items()}
        a[name][idx] += step
        return (np.asarray(dK, dtype=R.HI) * R.gram_ref(kind, a['dX'], a['dX2'], a['dls'], a['dvar'], dtype=R.HI)).sum()

    points = [('dX', (0, 0, 1)), ('dX', (0, 6, 0)), ('dX', (0, 4, 1)), ('dls', (0, 1)), ('dvar', (0, 0))]
    if not square:
        points += [('dX2', (0, 1, 0)), ('dX2', (0, 5, 1))]
    for name, idx in points:
        fd = (value(name, idx, h) - value(name, idx, -h)) / (2 * h)
        assert abs(fd - grad[name][idx]) <= 1e-8 * scale[name][idx], (name, idx, float(fd), float(grad[name][idx]))


def test_clip_conventions():
    """inside the clip radius (0 < r2 < 1e-14) the slope is 0 for Matern12 / Matern32 and +5/3 e for Matern52, which is what autograd through
    sqrt(clamp(r2, 1e-14)) gives (the oracle, in the difference form so that r2 is exact); exact duplicates contribute nothing at all"""
    r2 = np.array([0.0, 1e-18, 9e-15, 1.1e-14, 1e-3, 2.0])
    t = torch.tensor(r2, requires_grad=True)
    R_ = torch.sqrt(torch.clamp(t, min=1e-14))
    forms = {'rbf': torch.exp(t / -2), 'matern12': torch.exp(-R_), 'matern32': (1 + 3 ** 0.5 * R_) * torch.exp(-3 ** 0.5 * R_),
             'matern52': (1 + 5 ** 0.5 * R_ + 5 / 3. * t) * torch.exp(-5 ** 0.5 * R_)}
    for kind, val in forms.items():
        slope, = torch.autograd.grad(val.sum(), t, retain_graph=True)
        f, fp = R.f_and_slope(kind, r2.astype(R.HI))
        assert np.allclose(f.astype(np.float64), val.detach().numpy(), rtol=1e-14, atol=0), kind
        # (autograd forms the Matern32 / 52 slopes as a difference of two terms ~1 / r each: at r = 1e-7 it keeps ~9 digits)
        assert np.allclose(fp.astype(np.float64), slope.numpy(), rtol=1e-8, atol=0), kind
    assert R.f_and_slope('matern52', np.array([1e-18]))[1][0] > 1.6 and R.f_and_slope('matern12', np.array([1e-18]))[1][0] == 0
