"""The per-sample log-pdf reductions (mxf_normal_logpdf_ps*, mxf_univariate_logpdf_ps*) through ops.logpdf_per_sample_ /
ops.logpdf_per_sample_bwd_ on the MI355X: out[s] += scale * sum_i log p(x[s,i] | a, b) and its reverse mode with per-sample weights, for
the Normal and the six univariate kinds in both dtypes.  Expected values are the float64 CPU restatement of tests/_score_ref.py; the
tolerances are stated there (float64 1e-9 of the summed magnitudes; float32 rtol 1e-4, atol 1e-5 after the CPU float32 precondition).

Shapes: n = 1, 257 (one element past a 256-thread workgroup), 512 * 256 + 3 (a second grid-stride trip; one kind per dtype); S = 1, 2, 5,
and S = 65 537 with n = 2 (past the 65 535 limit of a grid's y and z axes, and past the kernel's own 65 536-workgroup grid: the pair loop
takes a second trip); every pair of parameter layouts {single element, per element, per sample and element}; every nullable output of
the reverse mode null in turn; weights of mixed signs with one exact zero; outputs pre-filled, since every output is accumulated into."""
import numpy as np
import pytest
import torch

import _score_ref as R

pytestmark = pytest.mark.gpu

OUT_FILL, GRAD_FILL = 0.75, -0.5
SCALE = 0.625


def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=R.tdt(dtype)).cuda()


def existing_mean(kind, x, a, b, la, lb, scale):
    """sum_s out[s] / S from the entry points that were there before: the reduced kernels at scale / S where they take the layouts
    (parameters without a sample axis), the un-reduced univariate kernel summed where a parameter is sampled; None: the Normal with a
    sampled parameter, which no earlier entry point takes"""
    from mxfusion_amd import ops
    S = x.shape[0]
    acc = torch.zeros(1, dtype=x.dtype, device=x.device)
    if 'sn' not in (la, lb) or S == 1:
        if kind == 'normal':
            ops.normal_logpdf_(x, a.reshape(-1), b.reshape(-1), scale / S, acc)
        else:
            ops.univariate_logpdf_(kind, x, a.reshape(-1), b.reshape(-1), scale / S, acc)
        return float(acc)
    if kind == 'normal':
        return None
    return float(ops.univariate_logpdf_elem(kind, x, a, b, scale / S).double().sum())


def run_case(kind, dtype, S, n, la, lb, tie=True, nulls=True):
    from mxfusion_amd import ops
    what = (kind, dtype, S, n, la, lb)
    x, a, b = R.make_inputs(kind, S, n, la, lb, dtype)
    if kind == 'bernoulli':
        lb = la
    w = R.weights(S, dtype)
    (out, dx, da, db), mags = R.expected(kind, x, a, b, la, lb, w, SCALE)
    if dtype == 'float32':
        R.assert_float32_formula_meets_the_bar(what, R.expected(kind, x, a, b, la, lb, w, SCALE, torch.float32)[0], (out, dx, da, db))
    if kind == 'uniform' and S >= 2:
        assert np.isneginf(out[S - 1]) and np.isfinite(out[:S - 1]).all()
    X, A, B, W = dev(x, dtype), dev(a, dtype), dev(b, dtype), dev(w, dtype)
    got = ops.logpdf_per_sample_(kind, X, A, B, SCALE, torch.full((S,), OUT_FILL, dtype=X.dtype, device=X.device))
    R.assert_close(what + ('out',), got.cpu().numpy(), out, mags[0], dtype, OUT_FILL)

    fill = lambda t: torch.full_like(t, GRAD_FILL)
    full = [fill(X), fill(A), fill(B)]
    ops.logpdf_per_sample_bwd_(kind, X, A, B, W, SCALE, *full)
    for name, g, want, mag in zip(('dx', 'da', 'db'), full, (dx, da, db), mags[1:]):
        R.assert_close(what + (name,), g.cpu().numpy(), want.reshape(g.shape), mag.reshape(g.shape), dtype, GRAD_FILL)
    if kind == 'uniform' and S >= 2:          # nothing was added from the element outside the support
        assert float(full[0][S - 1, n - 1]) == GRAD_FILL
    if nulls:
        for k in range(3):
            bufs = [None if j == k else fill(t) for j, t in enumerate((X, A, B))]
            ops.logpdf_per_sample_bwd_(kind, X, A, B, W, SCALE, *bufs)
            for j, (name, want, mag) in enumerate(zip(('dx', 'da', 'db'), (dx, da, db), mags[1:])):
                if j != k:
                    R.assert_close(what + (name, 'without output %d' % k), bufs[j].cpu().numpy(), want.reshape(bufs[j].shape),
                                   mag.reshape(bufs[j].shape), dtype, GRAD_FILL)
    if tie:
        old = existing_mean(kind, X, A, B, la, lb, SCALE)
        if old is not None:
            fresh = ops.logpdf_per_sample_(kind, X, A, B, SCALE, torch.zeros(S, dtype=X.dtype, device=X.device)).double().cpu().numpy()
            new = fresh.sum() / S
            R.assert_close(what + ('mean against the reduced kernel',), np.array([new]), np.array([old]), np.array([mags[0].sum() / S]), dtype)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', R.KINDS)
def test_per_sample_logpdf_and_reverse_mode(kind, dtype):
    for n in (1, 257):
        for S in (1, 2, 5):
            for la in R.LAYOUTS:
                for lb in (R.LAYOUTS if kind != 'bernoulli' else ('1',)):
                    run_case(kind, dtype, S, n, la, lb)


@pytest.mark.parametrize('kind,dtype', [('normal', 'float32'), ('laplace', 'float64')])
def test_per_sample_logpdf_second_grid_stride_trip(kind, dtype):
    n = 512 * 256 + 3
    run_case(kind, dtype, 2, n, 'sn', '1', nulls=False)
    run_case(kind, dtype, 1, n, 'n', 'n', nulls=False)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('kind', ['normal', 'laplace'])
def test_per_sample_logpdf_more_samples_than_a_grid_axis(kind, dtype):
    run_case(kind, dtype, 65537, 2, '1', 'n', nulls=False)
    run_case(kind, dtype, 65537, 2, 'sn', '1', nulls=False)


def test_per_sample_wrappers_check_their_buffers():
    from mxfusion_amd import ops
    x = torch.zeros(3, 4, dtype=torch.float64).cuda()
    one = torch.ones(1, dtype=torch.float64).cuda()
    with pytest.raises(ValueError):
        ops.logpdf_per_sample_('normal', x, one, one, 1.0, torch.zeros(4, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        ops.logpdf_per_sample_bwd_('normal', x, one, one, torch.zeros(3, dtype=torch.float64).cuda(), 1.0, dx_acc=torch.zeros(12, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        ops.logpdf_per_sample_('laplace', x, torch.ones(5, dtype=torch.float64).cuda(), one, 1.0, torch.zeros(3, dtype=torch.float64).cuda())
