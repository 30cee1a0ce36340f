"""The float32 reverse modes that sum a shared operand's gradient in double (csrc/shared_grad.h), at the one seam they have in common: the
table of up to three segments of handle scratch.  For each family every operand that can be shared is shared over every axis its entry
point allows, and the reverse mode runs for every non-empty subset of the wanted gradient buffers, so that absent segments fall at the
front, in the middle and at the back of the table.  Each returned gradient is compared with the same call in float64, to the bar of that
family's own float32 gradient test (taken from its module: 4 x the error of torch's float32 CPU evaluation, and the floors stated there).

Also here: ops.mvn_logpdf_bwd_ refuses a gradient buffer that is not shaped like its operand."""
import itertools

import numpy as np
import pytest
import torch

import test_gpu_dense as td
import test_gpu_mvn as tm
import test_gpu_simplex as ts
import test_gpu_wishart as tw

pytestmark = pytest.mark.gpu

S, B = 3, 5


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _subsets(k):
    return [m for m in itertools.product((False, True), repeat=k) if any(m)]


def _sweep(what, run, shapes, bars, measure=None):
    """run(dtype, buffers) accumulates into the buffers that are not None.  float64 with all of them is the reference of every float32
    subset; bars: one per buffer."""
    measure = measure or [lambda a: a] * len(shapes)
    zeros = lambda dtype, keep: [torch.zeros(s, dtype=dtype, device='cuda') if k else None for s, k in zip(shapes, keep)]
    want = zeros(torch.float64, [True] * len(shapes))
    run(torch.float64, want)
    want = [f(w.cpu().numpy()) for f, w in zip(measure, want)]
    for keep in _subsets(len(shapes)):
        got = zeros(torch.float32, keep)
        run(torch.float32, got)
        torch.cuda.synchronize()
        for i, (g, w, bar, f) in enumerate(zip(got, want, bars, measure)):
            if g is None:
                continue
            err = tm.nerr(f(g.double().cpu().numpy()), w)
            print('%s wanted %s gradient %d: error %.3g, bar %.3g' % (what, keep, i, err, bar))
            assert err <= bar, (what, keep, i, err, bar)


@pytest.mark.parametrize('form', [0, 1])
def test_mvn_segments(form):
    from mxfusion_amd import ops
    n = 3
    r = np.random.RandomState(form)
    x, mean, A = _f32(r.randn(1, B, n) * 2), _f32(r.randn(1, 1, n)), tm.spd(r, (1, 1), n)
    A = _f32(A)
    A = 0.5 * (A + np.swapaxes(A, -1, -2))
    cot = _f32(r.uniform(0.5, 1.5, (S, B)))
    ref64, ref32 = (tm.reference(tm.FORMS[form], x, mean, A, cot, dt) for dt in (torch.float64, torch.float32))
    bar = 4 * max(tm.nerr(g, w) for g, w in zip(ref32, ref64))

    def run(dtype, grads):
        xd, md, Ad, c = (torch.as_tensor(t, dtype=dtype).cuda() for t in (x, mean, A, cot))
        F, _, _ = ops.mvn_factor(Ad, form)
        ops.mvn_logpdf_bwd_(xd, md, F, c, form, 1.0, *grads)
    _sweep('mvn form %d' % form, run, [x.shape, mean.shape, A.shape], [bar] * 3)


def test_wishart_segments():
    """the wrapper takes S from its operands, so one of them has to carry the sample axis: the degrees of freedom (S, 1), shared over the
    batch; X (1, B, n, n) and V (1, 1, n, n) are shared over all they can be, and all three segments are in the table"""
    from mxfusion_amd import ops
    n = 3
    r = np.random.RandomState(2)
    X, V = tw.spd(r, (1, B), n, 'float32'), tw.spd(r, (1, 1), n, 'float32')
    nu, cot = _f32(n - 1 + r.uniform(0.5, 6.0, (S, 1))), _f32(r.uniform(0.5, 1.5, (S, B)))
    ref64, ref32 = (tw.reference(X, nu, V, cot, dt) for dt in (torch.float64, torch.float32))
    bar = 4 * max(tw.nerr(g, w) for g, w in zip(ref32, ref64))

    def run(dtype, grads):
        Xd, nd, Vd, c = (torch.as_tensor(t, dtype=dtype).cuda() for t in (X, nu, V, cot))
        ops.wishart_logpdf_bwd_(Xd, nd, Vd, c, 1.0, *grads)
    _sweep('wishart', run, [X.shape, nu.shape, V.shape], [bar] * 3, [tw._sym, lambda a: a, tw._sym])


def test_categorical_segments():
    from mxfusion_amd import ops
    (logp, x, cot), _, bars = ts.cat_case('float32', 3, S, B, 'both', 'samples', True, True)

    def run(dtype, grads):
        lp, xd, c = (torch.as_tensor(t, dtype=dtype).cuda() for t in (logp, x, cot))
        ops.categorical_logpdf_bwd_(lp, xd, c, True, True, 1.0, *grads)
    _sweep('categorical', run, [logp.shape, x.shape], bars[1:])


def test_dirichlet_segments():
    from mxfusion_amd import ops
    (x, alpha, cot), _, bars = ts.dir_case('float32', 3, S, B, 'both', 'samples', True)

    def run(dtype, grads):
        xd, ad, c = (torch.as_tensor(t, dtype=dtype).cuda() for t in (x, alpha, cot))
        ops.dirichlet_logpdf_bwd_(xd, ad, c, True, 1.0, *grads)
    _sweep('dirichlet', run, [x.shape, alpha.shape], bars[1:])


def test_dense_segments():
    from mxfusion_amd import ops
    N, I, O = 5, 3, 2
    (X, W, b, cot), want, bars = td.case('float32', I, O, N, S, 'tanh', 'shared', 'shared', 'shared')
    Y = _f32(want[0])

    def run(dtype, grads):
        Xd, Wd, Yd, c = (torch.as_tensor(t, dtype=dtype).cuda() for t in (X, W, Y, cot))
        ops.dense_bwd_(Xd, Wd, Yd, c, 'tanh', *grads)
    _sweep('dense', run, [X.shape, W.shape, b.shape], bars[1:])


def test_mvn_refuses_a_gradient_buffer_of_the_full_shape():
    """the matrix is shared, its gradient is (1, 1, n, n): a buffer (S, B, n, n) is refused before anything is launched or written"""
    from mxfusion_amd import ops
    n = 3
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')
    x, mean, A = z(S, B, n), z(S, B, n), torch.eye(n, dtype=torch.float64, device='cuda').reshape(1, 1, n, n)
    F, _, _ = ops.mvn_factor(A)
    dx, dA = z(S, B, n), z(S, B, n, n)
    with pytest.raises(ValueError):
        ops.mvn_logpdf_bwd_(x, mean, F, torch.ones(S, B, dtype=torch.float64, device='cuda'), dx_acc=dx, dA_acc=dA)
    torch.cuda.synchronize()
    assert not dx.any() and not dA.any()
    ops.mvn_logpdf_bwd_(x, mean, F, torch.ones(S, B, dtype=torch.float64, device='cuda'), dx_acc=dx, dA_acc=z(1, 1, n, n))
