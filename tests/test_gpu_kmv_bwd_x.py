"""mxf_kmv_bwd_x on the GPU, in both dtypes: the gradient of sum_j w_j A[:, j]^T K(X, X2) V[:, j] in X and X2 against tests/_gram_ref.py on the
written-out cotangent dK = sum_j w_j A[:, j] V[:, j]^T, errors relative to that function's absolute sums, at tests/test_gpu_kmv.py's bars
and from the sizes it documents.  Beyond those: the square product is fused in float32 and at J <= 4 and two role passes in float64 at
J > 4; N = 100 x 5000, its transpose and a square N = 3000 split the streamed rows; dup: rows of X2 copied from X (a clipped pair has no
slope).  The buffers start at 1: the results are accumulated."""
import functools

import numpy as np
import pytest
import torch

import _gram_ref as GR

pytestmark = pytest.mark.gpu

BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
ALL = frozenset(('X', 'X2', 'ls', 'var', 'V', 'A'))

#         kind, ard, N, N2 (None: square), Q, J, S, operands that own a sample axis, rows of X2 copied from X
CASES = [('rbf', True, n, n2, 3, 5, 1, ALL, 0) for n in (1, 127, 129, 300) for n2 in (1, 63, 65, 200)]
CASES += [(k, ard, 129, 65, q, 17 if q % 2 else 4, 1, ALL, 0) for q, k in ((1, 'matern12'), (3, 'matern32'), (8, 'matern52'), (16, 'rbf'))
          for ard in (True, False)]
CASES += [('rbf', False, 129, 65, 3, j, 1, ALL, 0) for j in (1, 4, 16, 17, 70)]
CASES += [(k, True, 129, None, 3, 5, 1, ALL, 0) for k in GR.KINDS] + [('matern52', False, 129, None, 16, 17, 1, ALL, 0),
                                                                       ('rbf', True, 300, None, 8, 70, 1, ALL, 0), ('matern32', True, 65, None, 3, 4, 1, ALL, 0)]
CASES += [('rbf', True, 129, 70, 3, 17, 2, own, 0) for own in (ALL, ALL - {'X'}, ALL - {'X2'}, frozenset(['V', 'A']))]
CASES += [('matern32', True, 130, None, 3, j, 2, own, 0) for j in (4, 17) for own in (ALL, frozenset(['ls', 'V', 'A']))]
CASES += [('rbf', True, 100, 5000, 3, 5, 1, ALL, 0), ('rbf', True, 5000, 100, 3, 5, 1, ALL, 0), ('matern32', False, 3000, None, 2, 4, 1, ALL, 0)]
CASES += [(k, True, 129, 65, 3, 5, 1, ALL, 3) for k in GR.KINDS[1:]]
IDS = ['%s-%s-N%d-N2%s-Q%d-J%d-S%d-%s-dup%d' % (k, 'ard' if a else 'iso', n, n2, q, j, s, 'all' if own == ALL else '+'.join(sorted(own)), dup)
       for k, a, n, n2, q, j, s, own, dup in CASES]


@functools.lru_cache(maxsize=None)
def _case(case, rounded):
    """(float64 numpy operands with the sample axis, (grad, scale) of the reference); rounded: the values a float32 run sees"""
    kind, ard, N, N2, Q, J, S, own, dup = case
    rng = np.random.default_rng(N * 1000003 + (N2 or 0) * 1009 + Q * 31 + S * 7 + 2 * len(own) + 13 * J + GR.KIND_ID[kind])
    ax = lambda name: S if name in own else 1
    M = N if N2 is None else N2
    p = dict(X=rng.uniform(-2, 2, (ax('X'), N, Q)), X2=None if N2 is None else rng.uniform(-2, 2, (ax('X2'), N2, Q)),
             ls=rng.uniform(0.8, 1.8, (ax('ls'), Q if ard else 1)), var=rng.uniform(0.5, 1.5, (ax('var'), 1)),
             V=rng.standard_normal((ax('V'), M, J)), A=rng.standard_normal((ax('A'), N, J)), w=rng.uniform(-1, 1, J))
    if dup:
        p['X2'][:, :dup] = p['X'][:, 5:5 + dup]
    if rounded:
        p = {k: v if v is None or k == 'w' else v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    bc = lambda a: np.broadcast_to(a, (S,) + a.shape[1:])
    dK = np.einsum('snj,smj,j->snm', bc(p['A']), bc(p['V']), p['w'])
    return p, GR.gram_bwd_ref(kind, p['X'], p['X2'], p['ls'], p['var'], dK)


_device = lambda p, dtype: {k: None if v is None else torch.as_tensor(v).to(dtype).cuda().contiguous() for k, v in p.items() if k != 'w'}


def _close(got, ref, mag, dtype, what):
    rtol, atol = BARS[dtype]
    got, ref, mag = got.double().cpu(), torch.as_tensor(ref).double(), torch.as_tensor(mag).double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (what, got.shape, ref.shape)
    err = (got - ref).abs()
    ratio = float((err / (rtol * mag + atol)).max())
    print('ratio', what, str(dtype)[6:], '%.3g' % ratio, 'max error', float(err.max()), 'max magnitude', float(mag.max()))
    assert ratio <= 1.0, (what, float(err.max()), float(mag.max()), ratio)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_kernel_against_the_reference(case, dtype):
    from mxfusion_amd import ops
    (kind, ard), (p, (g, sc)) = case[:2], _case(case, dtype == torch.float32)
    d = _device(p, dtype)
    run = lambda dX, dX2: ops.kernel_matvec_bwd_x_(kind, d['X'], d['X2'], d['ls'], d['var'], ard, d['A'], d['V'], list(p['w']), dX, dX2)
    dX, dX2 = torch.ones_like(d['X']), None if d['X2'] is None else torch.ones_like(d['X2'])
    run(dX, dX2)
    _close(dX, g['dX'] + 1.0, sc['dX'] + 1.0, dtype, 'dX')
    if dX2 is not None:
        _close(dX2, g['dX2'] + 1.0, sc['dX2'] + 1.0, dtype, 'dX2')
        for name, alone in (('dX', (torch.ones_like(d['X']), None)), ('dX2', (None, torch.ones_like(d['X2'])))):
            run(*alone)
            _close(alone[0] if name == 'dX' else alone[1], g[name] + 1.0, sc[name] + 1.0, dtype, name + ' alone')


def test_status_codes_leave_the_buffers_alone():
    """Q = 17 is -3; a null A, both outputs null and dX2_acc with a null X2 are -2; nothing is written"""
    from mxfusion_amd import _lib, ops
    mk = lambda *s: torch.ones(*s, dtype=torch.float64).cuda()

    def call(Q=3, null=(), square=False):
        X, X2, ls, var, V, A = mk(1, 4, Q), mk(1, 5, Q), mk(1, Q), mk(1, 1), mk(1, 4 if square else 5, 2), mk(1, 4, 2)
        dX, dX2 = 7.0 * mk(1, 4, Q), 7.0 * mk(1, 5, Q)
        ptr = lambda name, t: None if name in null or (square and name == 'X2') else t.data_ptr()
        try:
            _lib.call('mxf_kmv_bwd_x', ops._h(X), _lib.K_RBF, _lib.F64, 1, 4, 5, Q, 2, X.data_ptr(), 0, ptr('X2', X2), 0, ls.data_ptr(), 0, 1,
                      var.data_ptr(), 0, ptr('A', A), 0, V.data_ptr(), 0, (_lib._c.c_double * 2)(1.0, 1.0), ptr('dX', dX), ptr('dX2', dX2),
                      ops._stream())
        finally:
            torch.cuda.synchronize()
            assert float((dX - 7.0).abs().max()) == 0.0 and float((dX2 - 7.0).abs().max()) == 0.0
    with pytest.raises(_lib.MXFError, match=r'\(-3\)'):
        call(Q=17)
    for kw in (dict(null=('A',)), dict(null=('dX', 'dX2')), dict(square=True)):
        with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
            call(**kw)
    call()          # coincident points: the same call with nothing wrong adds no gradient


def test_autograd():
    """ops.KernelMatvec and StationaryKernel.matvec(inputs_grad=True): X and X2 get the gradients of sum(out G); Q = 17 names the limit"""
    from mxfusion_amd import ops
    from mxfusion_amd.components.distributions.gp.kernels import Matern52
    p, _ = _case(('matern52', True, 129, 70, 3, 5, 1, ALL, 0), False)
    g, sc = GR.gram_bwd_ref('matern52', p['X'], p['X2'], p['ls'], p['var'], np.einsum('snj,smj->snm', p['A'], p['V']))
    d = _device(p, torch.float64)
    kern = Matern52(3, ARD=True)
    for f in (lambda X, X2: ops.KernelMatvec.apply('matern52', True, X, X2, d['ls'], d['var'], d['V'], None),
              lambda X, X2: kern.matvec(None, X, d['V'], X2=X2, inputs_grad=True, matern52_lengthscale=d['ls'], matern52_variance=d['var'])):
        X, X2 = d['X'].clone().requires_grad_(True), d['X2'].clone().requires_grad_(True)
        (f(X, X2) * d['A']).sum().backward()
        _close(X.grad, g['dX'], sc['dX'], torch.float64, 'gradient in X')
        _close(X2.grad, g['dX2'], sc['dX2'], torch.float64, 'gradient in X2')
    X17, V17 = torch.zeros(1, 5, 17, dtype=torch.float64).cuda().requires_grad_(True), torch.ones(1, 5, 2, dtype=torch.float64).cuda()
    out = ops.KernelMatvec.apply('rbf', False, X17, None, d['ls'][:, :1].contiguous(), d['var'], V17, None)
    with pytest.raises(NotImplementedError, match='at most 16 input dimensions'):
        out.sum().backward()
