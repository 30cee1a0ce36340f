"""mxf_kmv and mxf_kmv_bwd on the GPU, in both dtypes:
    out[s, n, j] = sum_n2 k(X[s, n], X2[s, n2]) V[s, n2, j] (+ diag_add[s] V[s, n, j], square)        against ops.gram(...) @ V in float64,
    dls, dvar of sum_j w_j A[:, j]^T K V[:, j]                                                        against tests/_gram_ref.py with the
cotangent dK = sum_j w_j A[:, j] V[:, j]^T written out (float64 numpy).

Sizes of csrc/kmv.hip that the shapes are chosen from: a wavefront is 64 rows, a workgroup KMV_RB = 128 rows, a thread one row; a thread sums
KMV_CH = 64 values of n2 in the working dtype between two additions to its double register; a pass serves a block of 4 columns of V for J <= 4
and of KMV_JB = 16 above, a larger J takes further passes, and the reverse mode prepares KMV_WG = 64 weighted columns per prep launch (J = 70
takes two); Q is padded to 4, 8 or 16; n2 is split over min(ceil(1024 / (ceil(N / 128) * S)), ceil(N2 / 64)) workgroup rows, which add
into doubles.  So N in {1, 127, 129, 300} x N2 in {1, 63, 65, 200}, Q in {1, 3, 8, 16}, J in {1, 4, 5, 16, 17, 33, 70}, the four kinds with
and without ARD, S in {1, 2} with shared and per-sample operands, square with diag_add and rectangular, N = 100 x N2 = 5 000 (a split
into 79 workgroup rows of 64 that add into the double scratch) and N = 140 000 x N2 = 3 (1 094 row workgroups).  N2 <= 64 is written by the
threads themselves; every larger N2 here is split.

Operands: x in [-2, 2], length-scales in [0.8, 1.8], variance in [0.5, 1.5], V, A standard normal, weights in [-1, 1].  Bars: float64 rtol
1e-9 / atol 1e-11, float32 rtol 1e-4 / atol 1e-5, relative to the sum of the magnitudes of an element's terms (|K| |V| forward; the absolute
sums of _gram_ref.gram_bwd_ref reverse); the reference of a float32 run sees the rounded operands.  The output lies in a buffer with a guard
band of 64 elements on each side that must stay untouched.  Every test prints the worst ratio of an error to its bar."""
import functools

import numpy as np
import pytest
import torch

import _gram_ref as GR

pytestmark = pytest.mark.gpu

BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
OPS = ('X', 'X2', 'ls', 'var', 'V', 'A', 'diag')
ALL = frozenset(OPS)
GUARD = 64

#         kind, ard, N, N2 (None: square, with diag_add), Q, J, S, operands that own a sample axis
CASES = [('rbf', True, n, n2, 3, 5, 1, ALL) for n in (1, 127, 129, 300) for n2 in (1, 63, 65, 200)]
CASES += [(k, True, 129, 65, q, 17 if q % 2 else 4, 1, ALL) for q, k in ((1, 'matern12'), (3, 'matern32'), (8, 'matern52'), (16, 'rbf'))]
CASES += [('rbf', False, 129, 65, 3, j, 1, ALL) for j in (1, 4, 16, 17, 33, 70)]
CASES += [(k, ard, 129, None, 3, 5, 1, ALL) for k in GR.KINDS for ard in (True, False)]
CASES += [(k, False, 127, 65, 5, 17, 1, ALL) for k in GR.KINDS[1:]]
CASES += [('rbf', True, 129, 70, 3, 17, 2, own) for own in (ALL, frozenset(['X']), frozenset(['ls', 'var', 'V', 'A']), frozenset(['V', 'A']),
                                                             frozenset(['X2', 'ls']))]
CASES += [('matern52', True, 300, None, 3, 5, 2, ALL), ('matern32', False, 129, None, 2, 17, 2, frozenset(['V', 'A', 'diag'])),
          ('rbf', True, 130, None, 3, 4, 2, frozenset(['ls', 'var', 'V', 'A']))]
CASES += [('rbf', True, 100, 5000, 3, 5, 1, ALL), ('matern32', False, 140000, 3, 2, 1, 1, ALL)]
IDS = ['%s-%s-N%d-N2%s-Q%d-J%d-S%d-%s' % (k, 'ard' if a else 'iso', n, n2, q, j, s, 'all' if own == ALL else '+'.join(sorted(own)))
       for k, a, n, n2, q, j, s, own in CASES]


def _inputs(case, rounded=False):
    """float64 numpy operands with the sample axis (extent 1 where shared); rounded: the values a float32 run sees"""
    kind, ard, N, N2, Q, J, S, own = case
    rng = np.random.default_rng(N * 1000003 + (N2 or 0) * 1009 + Q * 31 + S * 7 + 2 * len(own) + 13 * J + GR.KIND_ID[kind])
    ax = lambda name: S if name in own else 1
    M = N if N2 is None else N2
    p = dict(X=rng.uniform(-2, 2, (ax('X'), N, Q)), X2=None if N2 is None else rng.uniform(-2, 2, (ax('X2'), N2, Q)),
             ls=rng.uniform(0.8, 1.8, (ax('ls'), Q if ard else 1)), var=rng.uniform(0.5, 1.5, (ax('var'), 1)),
             V=rng.standard_normal((ax('V'), M, J)), A=rng.standard_normal((ax('A'), N, J)),
             diag=rng.uniform(0.05, 0.5, (ax('diag'), 1)) if N2 is None else None, w=rng.uniform(-1, 1, J))
    if rounded:
        p = {k: v if v is None or k == 'w' else v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    return p


def _device(p, dtype):
    return {k: None if v is None else torch.as_tensor(v).to(dtype).cuda().contiguous() for k, v in p.items() if k != 'w'}


@functools.lru_cache(maxsize=None)
def _reverse_reference(case, rounded=False):
    """(grad, scale) of tests/_gram_ref.py for the cotangent sum_j w_j A[:, j] V[:, j]^T"""
    kind, ard, N, N2, Q, J, S, own = case
    p = _inputs(case, rounded)
    bc = lambda a: np.broadcast_to(a, (S,) + a.shape[1:])
    dK = np.einsum('snj,smj,j->snm', bc(p['A']), bc(p['V']), p['w'])
    return GR.gram_bwd_ref(kind, p['X'], p['X2'], p['ls'], p['var'], dK)


def _close(got, ref, mag, dtype, what):
    rtol, atol = BARS[dtype]
    got, ref, mag = got.double().cpu(), torch.as_tensor(ref).double().cpu(), torch.as_tensor(mag).double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    ratio = float((err / (rtol * mag + atol)).max())
    print('ratio', what, str(dtype)[6:], '%.3g' % ratio, 'max error', float(err.max()), 'max magnitude', float(mag.max()))
    assert ratio <= 1.0, (what, float(err.max()), float(mag.max()), ratio)


def _forward_reference(case, rounded):
    """K V (+ diag V) and |K| |V| (+ diag |V|) in float64 on the device from ops.gram"""
    from mxfusion_amd import ops
    kind, ard = case[:2]
    d = _device(_inputs(case, rounded), torch.float64)
    K = ops.gram(kind, d['X'], d['X2'], d['ls'], d['var'], ard)
    ref, mag = K @ d['V'], K.abs() @ d['V'].abs()
    if d['diag'] is not None:
        ref, mag = ref + d['diag'].unsqueeze(-1) * d['V'], mag + d['diag'].unsqueeze(-1) * d['V'].abs()
    return ref, mag


def _guarded_forward(d, kind, ard):
    """the raw entry point into the middle of a buffer of sevens: (out, the buffer)"""
    from mxfusion_amd import _lib, ops
    S, N, N2, Q, J, args = ops._kmv_operands('test', kind, d['X'], d['X2'], d['ls'], d['var'], ard, d['V'])
    buf = torch.full((S * N * J + 2 * GUARD,), 7.0, dtype=d['X'].dtype).cuda()
    out = buf[GUARD:GUARD + S * N * J]
    st = lambda t: 0 if t is None or t.shape[0] == 1 else t.stride(0)
    _lib.call('mxf_kmv', ops._h(d['X']), *args, ops._p(d['diag']), st(d['diag']), ops._p(d['V']), st(d['V']), out.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    return out.reshape(S, N, J), buf


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_and_reverse(case, dtype):
    from mxfusion_amd import ops
    kind, ard, N, N2, Q, J, S, own = case
    rounded = dtype == torch.float32
    ref, mag = _forward_reference(case, rounded)
    p = _inputs(case)
    d = _device(p, dtype)
    got = ops.kernel_matvec(kind, d['X'], d['X2'], d['ls'], d['var'], ard, d['V'], d['diag'])
    assert got.dtype == dtype
    _close(got, ref, mag, dtype, 'forward')
    out, buf = _guarded_forward(d, kind, ard)
    _close(out, ref, mag, dtype, 'forward into the guarded buffer')
    assert float((buf[:GUARD] - 7.0).abs().max()) == 0.0 and float((buf[-GUARD:] - 7.0).abs().max()) == 0.0, 'the guard band was written'
    # accumulated into: the buffers start at 1, the magnitudes of the terms gain that 1
    g, sc = _reverse_reference(case, rounded)
    dls, dvar = torch.ones_like(d['ls']), torch.ones_like(d['var'])
    ops.kernel_matvec_bwd_(kind, d['X'], d['X2'], d['ls'], d['var'], ard, d['A'], d['V'], list(p['w']), dls, dvar)
    _close(dls, g['dls'] + 1.0, sc['dls'] + 1.0, dtype, 'reverse, lengthscale')
    _close(dvar, g['dvar'] + 1.0, sc['dvar'] + 1.0, dtype, 'reverse, variance')
    only = torch.ones_like(d['var'])
    ops.kernel_matvec_bwd_(kind, d['X'], d['X2'], d['ls'], d['var'], ard, d['A'], d['V'], list(p['w']), None, only)
    _close(only, g['dvar'] + 1.0, sc['dvar'] + 1.0, dtype, 'reverse, variance alone')


def test_status_codes_leave_the_buffers_alone():
    """Q = 17 is -3; a null pointer, a bad stride, a non-stationary kind and J = 0 are -2; nothing is written"""
    from mxfusion_amd import _lib, ops
    mk = lambda *s: torch.ones(*s, dtype=torch.float64).cuda()

    def call(Q=3, J=2, null=None, ss_V=0, kind=_lib.K_RBF, bwd=False, valid=False):
        X, X2, ls, var, V, A = mk(1, 4, Q), mk(1, 5, Q), mk(1, Q), mk(1, 1), mk(1, 5, max(J, 1)), mk(1, 4, max(J, 1))
        out, out2 = torch.full((1, 4, max(J, 1)), 7.0, dtype=torch.float64).cuda(), torch.full((1, Q), 7.0, dtype=torch.float64).cuda()
        ptr = lambda name, t: None if null == name else t.data_ptr()
        head = [kind, _lib.F64, 1, 4, 5, Q, J, ptr('X', X), 0, ptr('X2', X2), 0, ptr('ls', ls), 0, 1, ptr('var', var), 0]
        try:
            if bwd:
                _lib.call('mxf_kmv_bwd', ops._h(X), *head, ptr('A', A), 0, ptr('V', V), ss_V, (_lib._c.c_double * max(J, 1))(*[1.0] * max(J, 1)),
                          out2.data_ptr(), None, ops._stream())
            else:
                _lib.call('mxf_kmv', ops._h(X), *head, None, 0, ptr('V', V), ss_V, out.data_ptr(), ops._stream())
        finally:
            torch.cuda.synchronize()
            if not valid:
                assert float((out - 7.0).abs().max()) == 0.0 and float((out2 - 7.0).abs().max()) == 0.0
        return out, out2
    for bwd in (False, True):
        with pytest.raises(_lib.MXFError, match=r'\(-3\)'):
            call(Q=17, bwd=bwd)
        for kw in (dict(null='X'), dict(null='V'), dict(null='ls'), dict(null='var'), dict(ss_V=7), dict(J=0), dict(kind=_lib.K_LINEAR)):
            with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
                call(bwd=bwd, **kw)
    with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
        call(null='A', bwd=True)
    # the same calls with nothing wrong run: all-ones operands, k = 1 for every pair, five columns
    assert float((call(valid=True)[0] - 5.0).abs().max()) == 0.0
    assert float((call(bwd=True, valid=True)[1] - 7.0).abs().max()) == 0.0          # coincident points: no gradient in the lengthscale


def test_autograd_function():
    """ops.KernelMatvec / StationaryKernel.matvec under autograd: V, lengthscale and variance get the gradients of sum(out G) (the gradient in
    V is K^T G from ops.gram, the others tests/_gram_ref.py); an X that requires a gradient is an error"""
    from mxfusion_amd import ops
    from mxfusion_amd.components.distributions.gp.kernels import Matern52
    case = ('matern52', True, 129, 70, 3, 5, 1, ALL)
    p = _inputs(case)
    d = _device(p, torch.float64)
    kern = Matern52(3, ARD=True)
    ls, var, V = [d[k].clone().requires_grad_(True) for k in ('ls', 'var', 'V')]
    out = kern.matvec(None, d['X'], V, X2=d['X2'], matern52_lengthscale=ls, matern52_variance=var)
    G = d['A']
    (out * G).sum().backward()
    K = ops.gram('matern52', d['X'], d['X2'], d['ls'], d['var'], True)
    _close(V.grad, K.transpose(1, 2) @ G, K.transpose(1, 2).abs() @ G.abs(), torch.float64, 'gradient in V')
    dK = np.einsum('snj,smj->snm', p['A'], p['V'])
    g, sc = GR.gram_bwd_ref('matern52', p['X'], p['X2'], p['ls'], p['var'], dK)
    _close(ls.grad, g['dls'], sc['dls'], torch.float64, 'gradient in the lengthscale')
    _close(var.grad, g['dvar'], sc['dvar'], torch.float64, 'gradient in the variance')
    with pytest.raises(NotImplementedError, match='no reverse mode'):
        kern.matvec(None, d['X'].clone().requires_grad_(True), d['V'], X2=d['X2'], matern52_lengthscale=d['ls'], matern52_variance=d['var'])
