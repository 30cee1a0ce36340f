"""mxf_psi_rbf_quad on the GPU against tests/_psi_predict_ref.py, in both dtypes: R[s, n, j] = sum_{m,m'} A[s, j, m, m'] psi2n[s, n, m, m'].

Sizes of csrc/psi.hip that the shapes are chosen from: a workgroup owns 128 rows, a thread one row; a pass over the terms serves a block of
PSI_JB = 4 weight matrices, a larger J takes further passes; m is split, interleaved, over min(ceil(2048 / (ceil(N / 128) * S)), M)
workgroups, which add into double scratch -- with one such workgroup a thread writes its results itself; Q is padded to 4, 8 or 16.  So: N in
{1, 127, 129, 257}, M in {1, 16, 17, 33}, Q in {1, 3, 8, 9, 16} with ARD on and off, J in {1, 4, 5}, S in {1, 2} with every operand, A
included, shared or owning its sample axis; N = 43 700 at M = 13: 342 row workgroups, so 6 over m, each striding twice over the 13 values
with a tail of one; and N = 262 100 at M = 2: 2 048 row workgroups, one over m, the path without scratch.

Every fifth element of s cycles through 0, 1e-8, 0.3 and 100.  Bars of tests/test_gpu_psi.py: float64 rtol 1e-9 / atol 1e-11, float32 rtol 1e-4 /
atol 1e-5, relative to the sum of the magnitudes of an element's terms, sum |A_j| psi2n; the reference of a float32 run sees the rounded
operands."""
import functools

import numpy as np
import pytest
import torch

import _psi_ref as R
import _psi_predict_ref as PR

pytestmark = pytest.mark.gpu

BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
OPS = ('mu', 's', 'Z', 'ls', 'var')
ALL = frozenset(OPS + ('A',))
JB = 4          # PSI_JB of csrc/psi.hip

#        N,   M,  Q, ard,  J, S, operands that own a sample axis
CASES = [(n, 5, 3, True, j, 1, ALL) for n, j in ((1, 5), (127, 1), (129, JB), (257, JB + 1))]
CASES += [(129, m, 1, False, j, 1, ALL) for m, j in ((1, JB + 1), (16, 1), (17, JB), (33, JB + 1))]
CASES += [(127, 17, q, ard, 1 + (q % 2) * JB, 1, ALL) for q in (1, 3, 8, 9, 16) for ard in (True, False)]
CASES += [(129, 17, 3, True, JB + 1, 2, own) for own in (ALL, frozenset(['A']), frozenset(['mu']), frozenset(['Z', 'ls', 'var']), frozenset(['s', 'A']))]
CASES += [(43700, 13, 1, True, JB + 1, 1, ALL), (262100, 2, 1, True, JB + 1, 1, ALL)]
IDS = ['N%d-M%d-Q%d-%s-J%d-S%d-%s' % (n, m, q, 'ard' if a else 'iso', j, s, 'all' if own == ALL else '+'.join(sorted(own)))
       for n, m, q, a, j, s, own in CASES]


def _inputs(case, rounded=False):
    """float64 CPU operands with the sample axis (extent 1 where shared) and the weights A (S|1, J, M, M), not symmetric; every fifth element
    of s cycles through 0, 1e-8, 0.3 and 100.  rounded: the values a float32 run sees"""
    N, M, Q, ard, J, S, own = case
    rng = np.random.default_rng(N * 1000003 + M * 1009 + Q * 31 + S * 7 + int(ard) + 2 * len(own) + 13 * J)
    ax = lambda name: S if name in own else 1
    s = rng.uniform(0.05, 1.5, (ax('s'), N, Q))
    idx = np.arange(0, s.size, 5)
    s.reshape(-1)[idx] = np.resize([0.0, 1e-8, 0.3, 100.0], idx.size)
    p = dict(mu=rng.uniform(-2, 2, (ax('mu'), N, Q)), s=s, Z=rng.uniform(-2, 2, (ax('Z'), M, Q)),
             ls=rng.uniform(0.7, 1.5, (ax('ls'), Q if ard else 1)), var=rng.uniform(0.8, 1.6, (ax('var'), 1)),
             A=rng.standard_normal((ax('A'), J, M, M)))
    return {k: torch.as_tensor(v).float().double() if rounded else torch.as_tensor(v) for k, v in p.items()}


def _reference_of(p, case):
    """R (S, N, J) and the sums of the magnitudes of its terms; rows in chunks of 4096 (the contraction is row by row)"""
    N, M, Q, ard, J, S, own = case
    out, mag = torch.empty(S, N, J, dtype=torch.float64), torch.empty(S, N, J, dtype=torch.float64)
    for smp in range(S):
        o = {k: p[k][smp if p[k].shape[0] > 1 else 0] for k in OPS + ('A',)}
        for r0 in range(0, N, 4096):
            p2 = R.psi2n(o['mu'][r0:r0 + 4096], o['s'][r0:r0 + 4096], o['Z'], o['ls'], o['var'])
            out[smp, r0:r0 + 4096] = torch.einsum('jab,nab->nj', o['A'], p2)
            mag[smp, r0:r0 + 4096] = torch.einsum('jab,nab->nj', o['A'].abs(), p2)
    return out, mag


@functools.lru_cache(maxsize=None)
def _reference(case, rounded=False):
    return _reference_of(_inputs(case, rounded), case)


def _close(got, ref, mag, dtype, what):
    rtol, atol = BARS[dtype]
    got, ref, mag = got.double().cpu(), ref.double(), mag.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    worst = float((err - (rtol * mag + atol)).max())
    print(what, 'max error', float(err.max()), 'max magnitude', float(mag.max()))
    assert worst <= 0, (what, float(err.max()), float(mag.max()), worst)


def _device(p, dtype):
    return {k: v.to(dtype).cuda().contiguous() for k, v in p.items()}


def _run(d, ard):
    from mxfusion_amd import ops
    return ops.psi_rbf_quad(*[d[k] for k in OPS], ard, d['A'])


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_contraction(case, dtype):
    N, M, Q, ard, J, S, own = case
    ref, mag = _reference(case, dtype == torch.float32)
    got = _run(_device(_inputs(case), dtype), ard)
    assert got.dtype == dtype
    _close(got, ref, mag, dtype, 'R')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_only_the_symmetric_part_of_the_weights_counts(dtype):
    """A and (A + A^T) / 2 have the same A + A^T bit for bit (halving is exact): the same R to the bar"""
    case = (129, 17, 3, True, JB + 1, 1, ALL)
    p = _inputs(case)
    d = _device(p, dtype)
    got = _run(d, True)
    sym = dict(d, A=((d['A'] + d['A'].transpose(-1, -2)) / 2).contiguous())
    assert not torch.equal(sym['A'], d['A'])
    got_sym = _run(sym, True)
    _, mag = _reference(case, dtype == torch.float32)
    _close(got_sym, got.double().cpu(), mag, dtype, 'symmetrised A')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_summed_over_the_rows_it_is_the_weighted_sum_of_psi2(dtype):
    """J = 1, A = G2: sum_n R[n] = sum(G2 * Psi2) of ops.psi_rbf, relative to sum(|G2| * Psi2)"""
    from mxfusion_amd import ops
    case = (257, 33, 3, True, 1, 1, ALL)
    d = _device(_inputs(case), dtype)
    got = _run(d, True).double().sum()
    _, Psi2 = ops.psi_rbf(*[d[k] for k in OPS], True, want_psi1=False)
    G2, Psi2 = d['A'][:, 0].double(), Psi2.double()
    ref, mag = (G2 * Psi2).sum(), (G2.abs() * Psi2).sum()
    rtol, atol = BARS[dtype]
    print('sum', float(got), 'reference', float(ref), 'magnitude', float(mag))
    assert abs(float(got) - float(ref)) <= rtol * float(mag) + atol


def test_status_codes():
    """Q above MXF_PSI_MAX_Q is -3; J = 0, a null A and a bad sample stride of A are -2; none touches R"""
    from mxfusion_amd import _lib, ops
    mk = lambda *shape: torch.ones(shape, dtype=torch.float64).cuda()
    one = mk(1, 1)

    def call(Q, J, A, ss_A=0):
        mu, Z = mk(1, 4, Q), mk(1, 3, Q)
        out = torch.full((1, 4, max(J, 1)), 7.0, dtype=torch.float64).cuda()
        try:
            _lib.call('mxf_psi_rbf_quad', ops._h(mu), _lib.F64, 1, 4, 3, Q, mu.data_ptr(), 0, mu.data_ptr(), 0, Z.data_ptr(), 0, one.data_ptr(), 0, 0,
                      one.data_ptr(), 0, J, None if A is None else A.data_ptr(), ss_A, out.data_ptr(), ops._stream())
        finally:
            torch.cuda.synchronize()
            assert float((out - 7.0).abs().max()) == 0.0
    with pytest.raises(_lib.MXFError, match=r'\(-3\)'):
        call(_lib.PSI_MAX_Q + 1, 2, mk(1, 2, 3, 3))
    with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
        call(2, 0, mk(1, 2, 3, 3))
    with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
        call(2, 2, None)
    with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
        call(2, 2, mk(1, 2, 3, 3), ss_A=5)
    with pytest.raises(_lib.MXFError, match=r'\(-2\)'):          # a null R
        mu, Z, A = mk(1, 4, 2), mk(1, 3, 2), mk(1, 2, 3, 3)
        _lib.call('mxf_psi_rbf_quad', ops._h(mu), _lib.F64, 1, 4, 3, 2, mu.data_ptr(), 0, mu.data_ptr(), 0, Z.data_ptr(), 0, one.data_ptr(), 0, 0,
                  one.data_ptr(), 0, 2, A.data_ptr(), 0, None, ops._stream())


def test_kernel_method():
    """RBF.psi2_quadratic is the op; it refuses operands that require a gradient while autograd records; other kernels and active_dims raise
    the ModelSpecificationError of psi_statistics"""
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions.gp.kernels import RBF, Matern52
    case = (129, 17, 3, True, JB + 1, 1, ALL)
    d = _device(_inputs(case), torch.float64)
    k = RBF(input_dim=3, ARD=True, dtype='float64')
    params = {'rbf_lengthscale': d['ls'], 'rbf_variance': d['var']}
    got = k.psi2_quadratic(None, d['mu'], d['s'], d['Z'], d['A'], **params)
    _close(got, *_reference(case), torch.float64, 'RBF.psi2_quadratic')
    with pytest.raises(NotImplementedError, match='no reverse mode'):
        k.psi2_quadratic(None, d['mu'].clone().requires_grad_(True), d['s'], d['Z'], d['A'], **params)
    with torch.no_grad():
        k.psi2_quadratic(None, d['mu'].clone().requires_grad_(True), d['s'], d['Z'], d['A'], **params)
    for bad, pp in ((Matern52(input_dim=3, ARD=True, dtype='float64'), {'matern52_lengthscale': d['ls'], 'matern52_variance': d['var']}),
                    (RBF(input_dim=3, ARD=True, active_dims=[0, 1, 2], dtype='float64'), params)):
        with pytest.raises(ModelSpecificationError, match='single RBF kernel'):
            bad.psi2_quadratic(None, d['mu'], d['s'], d['Z'], d['A'], **pp)
