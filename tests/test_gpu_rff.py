"""mxf_rff_eval and mxf_rff_eval_bwd on the GPU against tests/_pathwise_ref.py, in both dtypes:
    out[s, n, j] = sum_d cos(X[s, n] . Omega[s, d] + phase[s, d]) W[s, d, j],      dX = the reverse mode of that in X.

Sizes of csrc/rff.hip that the shapes are chosen from: a wavefront is 64 rows, a workgroup RFF_RB = 128 rows, a thread one row; a thread sums
RFF_DCH = 64 values of d in the working dtype between two additions to its double register; a pass serves a block of 4 weights per feature
for J <= 4 and of RFF_JB = 16 above, a larger J takes further passes; Q is padded to 4, 8 or 16; d is split over
min(ceil(1024 / (ceil(N / 128) * S)), ceil(D / 64)) workgroup rows, which add into doubles -- with one such row a thread writes its results
itself.  So: N in {1, 63, 65, 127, 129}, D in {1, 63, 64, 65, 130}, J in {1, 4, 5, 16, 17}, Q in {1, 3, 4, 5, 8, 9, 16}, S in {1, 2} with each
of X, Omega, phase and W shared or owning its sample axis (a shared X at S = 2 is the reverse pass's summed case, with and without a split of
d); N = 70 000 at D = 3 (547 row workgroups, no split) and at D = 130 (split in two, the second with a tail of two); N = 131 073 at D = 65:
1 025 row workgroups, so no split, and two chunks of the double register.

Operands: x in [-2, 2], Omega = N(0, 1) / l with l in [0.7, 1.5], phase in [0, 2 pi), W and the cotangent standard normal.  Bars, relative
to the sum of the magnitudes of an element's terms (sum_d |W[d,j]| forward, sum_d |Omega[d,q]| sum_j |G[n,j] W[d,j]| reverse): float64 rtol
1e-9 / atol 1e-11, float32 rtol 1e-4 / atol 1e-5; the reference of a float32 run sees the rounded operands.  The argument of the cosine stays
below about 40 here, so its worst float32 rounding (Q + 2) 2^-24 40 = 4e-5 is inside the float32 bar.  Every test prints the worst ratio of
an error to its bar."""
import functools

import numpy as np
import pytest
import torch

import _pathwise_ref as PW

pytestmark = pytest.mark.gpu

BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
OPS = ('X', 'Omega', 'phase', 'W')
ALL = frozenset(OPS)
JB = 16         # RFF_JB of csrc/rff.hip (RFF_JB_SMALL = 4 for J <= 4)

#        N,   D,  Q,  J, S, operands that own a sample axis
CASES = [(n, 65, 3, 5, 1, ALL) for n in (1, 63, 65, 127, 129)]
CASES += [(129, d, 3, j, 1, ALL) for d, j in ((1, 1), (63, 4), (64, JB), (65, JB + 1), (130, 5))]
CASES += [(127, 9, q, JB + 1 if q % 2 else 4, 1, ALL) for q in (1, 3, 4, 5, 8, 9, 16)]
CASES += [(129, 70, 3, JB + 1, 2, own) for own in (ALL, frozenset(['X']), frozenset(['Omega', 'phase', 'W']), frozenset(['W']), frozenset(['Omega']),
                                                  frozenset(['X', 'phase']))]
CASES += [(129, 5, 3, 5, 2, frozenset(['Omega', 'phase', 'W']))]
CASES += [(70000, 3, 1, 1, 1, ALL), (70000, 130, 2, 1, 1, ALL), (131073, 65, 1, 1, 1, ALL)]
IDS = ['N%d-D%d-Q%d-J%d-S%d-%s' % (n, d, q, j, s, 'all' if own == ALL else '+'.join(sorted(own))) for n, d, q, j, s, own in CASES]


def _inputs(case, rounded=False):
    """float64 CPU operands with the sample axis (extent 1 where shared) and the cotangent G (S, N, J); rounded: the values a float32 run sees"""
    N, D, Q, J, S, own = case
    rng = np.random.default_rng(N * 1000003 + D * 1009 + Q * 31 + S * 7 + 2 * len(own) + 13 * J)
    ax = lambda name: S if name in own else 1
    p = dict(X=rng.uniform(-2, 2, (ax('X'), N, Q)), Omega=rng.standard_normal((ax('Omega'), D, Q)) / rng.uniform(0.7, 1.5, (ax('Omega'), 1, Q)),
             phase=rng.uniform(0, 2 * np.pi, (ax('phase'), D)), W=rng.standard_normal((ax('W'), D, J)), G=rng.standard_normal((S, N, J)))
    return {k: torch.as_tensor(v).float().double() if rounded else torch.as_tensor(v) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _reference(case, rounded=False):
    """(out, its magnitudes, dX, its magnitudes) in float64 on the CPU: the reverse mode is autograd through the restatement"""
    p = _inputs(case, rounded)
    X = p['X'].clone().requires_grad_(True)
    out, mag = PW.rff_eval(X, p['Omega'], p['phase'], p['W'])
    dX, = torch.autograd.grad((out * p['G']).sum(), X)
    return out.detach(), mag, dX, PW.rff_bwd_scale(p['X'], p['Omega'], p['phase'], p['W'], p['G'])


def _close(got, ref, mag, dtype, what):
    rtol, atol = BARS[dtype]
    got, ref, mag = got.double().cpu(), ref.double(), mag.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    ratio = float((err / (rtol * mag + atol)).max())
    print('ratio', what, str(dtype)[6:], '%.3g' % ratio, 'max error', float(err.max()), 'max magnitude', float(mag.max()))
    assert ratio <= 1.0, (what, float(err.max()), float(mag.max()), ratio)


def _device(p, dtype):
    return {k: v.to(dtype).cuda().contiguous() for k, v in p.items()}


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_and_reverse(case, dtype):
    from mxfusion_amd import ops
    ref, mag, dref, dmag = _reference(case, dtype == torch.float32)
    d = _device(_inputs(case), dtype)
    got = ops.rff_eval(*[d[k] for k in OPS])
    assert got.dtype == dtype
    _close(got, ref, mag, dtype, 'forward')
    # accumulated into: the buffer starts at 1, the magnitudes of the terms gain that 1
    dX = torch.ones_like(d['X'])
    ops.rff_eval_bwd_(*[d[k] for k in OPS], d['G'], dX)
    _close(dX, dref + 1.0, dmag + 1.0, dtype, 'reverse')


def test_autograd_function_against_central_differences():
    """float64, N = 3, D = 5, Q = 2: the gradient of ops.RFFEval in X against central differences of its own forward pass (torch.autograd.gradcheck,
    step 1e-6: truncation 1e-12 |Omega|^3, rounding 1e-16 / 1e-6); no gradient for the basis and the weights"""
    from mxfusion_amd import ops
    d = _device(_inputs((3, 5, 2, 3, 1, ALL)), torch.float64)
    X = d['X'].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: ops.RFFEval.apply(x, d['Omega'], d['phase'], d['W']), (X,), eps=1e-6, atol=1e-7, rtol=1e-6)
    lv = [d[k].clone().requires_grad_(True) for k in OPS]
    ops.RFFEval.apply(*lv).sum().backward()
    assert lv[0].grad is not None and all(t.grad is None for t in lv[1:])


def test_status_codes():
    """Q above MXF_RFF_MAX_Q is -3; J = 0, D = 0, a null operand or output and a bad sample stride are -2; none touches the output"""
    from mxfusion_amd import _lib, ops
    mk = lambda *shape: torch.ones(shape, dtype=torch.float64).cuda()

    def call(Q, J, D=3, null=None, ss_W=0, bwd=False):
        X, Om, ph, W = mk(1, 4, Q), mk(1, max(D, 1), Q), mk(1, max(D, 1)), mk(1, max(D, 1), max(J, 1))
        out = torch.full((1, 4, max(J, 1)) if not bwd else (1, 4, Q), 7.0, dtype=torch.float64).cuda()
        ptr = lambda name, t: None if null == name else t.data_ptr()
        tail = [ptr('out', out)] if not bwd else [ptr('G', mk(1, 4, max(J, 1))), ptr('out', out)]
        try:
            _lib.call('mxf_rff_eval_bwd' if bwd else 'mxf_rff_eval', ops._h(X), _lib.F64, 1, 4, D, Q, J, ptr('X', X), 0, ptr('Omega', Om), 0,
                      ptr('phase', ph), 0, ptr('W', W), ss_W, *tail, ops._stream())
        finally:
            torch.cuda.synchronize()
            assert float((out - 7.0).abs().max()) == 0.0
    for bwd in (False, True):
        with pytest.raises(_lib.MXFError, match=r'\(-3\)'):
            call(_lib.RFF_MAX_Q + 1, 2, bwd=bwd)
        for kw in (dict(J=0), dict(J=2, D=0), dict(J=2, ss_W=5), dict(J=2, null='X'), dict(J=2, null='Omega'), dict(J=2, null='phase'),
                   dict(J=2, null='W'), dict(J=2, null='out')):
            with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
                call(2, bwd=bwd, **kw)
    with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
        call(2, J=2, null='G', bwd=True)
    with pytest.raises(ValueError, match='sample axes'):
        ops.rff_eval(mk(2, 4, 2), mk(3, 3, 2), mk(1, 3), mk(1, 3, 2))
    with pytest.raises(ValueError, match='buffer of shape'):
        ops.rff_eval_bwd_(mk(1, 4, 2), mk(1, 3, 2), mk(1, 3), mk(1, 3, 2), mk(1, 4, 2), mk(2, 4, 2))
