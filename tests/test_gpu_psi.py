"""mxf_psi_rbf_fwd / mxf_psi_rbf_bwd on the GPU against tests/_psi_ref.py (values, and autograd for every gradient), in both dtypes.

Sizes of csrc/psi.hip that the shapes are chosen from: the pair-owned kernel works on 16 x 16 tiles of (m, m' <= m) and splits the rows into
min(ceil(2048 / (tile pairs * S)), ceil(N / 64)) chunks, each summed 64 rows at a time in T and then in double; the row-owned kernels take
128 (Psi2 reverse) or 256 (Psi1) rows per workgroup, 32 values of m per Psi1 chunk, and the Psi2 reverse pass strides over m with
min(ceil(2048 / (ceil(N / 128) * S)), M) workgroups; Q is padded to 4, 8 or 16.  So: N in {1, 63, 65, 257} (257 = five chunks of 52 rows at
M <= 16), M in {1, 5, 15, 16, 17, 33} (either side of one tile, three tiles in two tile rows), Q in {1, 3, 8, 16} with ARD on and off, S in
{1, 2} with every operand shared or owning its sample axis, and N = 22 000 at M = 33, Q = 1: 342 chunks of 65 rows (more than one 64-row
partial sum, with a tail of one row) and 12 strides over the 33 values of m (tail of 9).

Every fifth element of s cycles through 0, 1e-8, 0.3 and 100.  Bars of tests/test_gpu_likelihood.py: float64 rtol 1e-9 / atol 1e-11, float32 rtol 1e-4 / atol
1e-5, a sum taken relative to the sum of the magnitudes of its terms (computed here from the closed forms, term by term)."""
import functools

import numpy as np
import pytest
import torch

import _psi_ref as R

pytestmark = pytest.mark.gpu

BARS = {torch.float64: (1e-9, 1e-11), torch.float32: (1e-4, 1e-5)}
OPS = ('mu', 's', 'Z', 'ls', 'var')
ALL = frozenset(OPS)

#        N,   M,  Q, ard,  S, operands that own a sample axis
CASES = [(n, 5, 3, True, 1, ALL) for n in (1, 63, 65, 257)]
CASES += [(65, m, 1, False, 1, ALL) for m in (1, 15, 16, 17, 33)]
CASES += [(63, 17, q, ard, 1, ALL) for q in (1, 3, 8, 16) for ard in (True, False)]
CASES += [(65, 17, 3, True, 2, own) for own in (ALL, frozenset(['mu']), frozenset(['Z', 'ls', 'var']), frozenset(['s']))]
CASES += [(22000, 33, 1, True, 1, ALL)]
IDS = ['N%d-M%d-Q%d-%s-S%d-%s' % (n, m, q, 'ard' if a else 'iso', s, 'all' if own == ALL else '+'.join(sorted(own))) for n, m, q, a, s, own in CASES]


def _inputs(case, rounded=False):
    """float64 CPU operands with the sample axis (extent 1 where shared) and the cotangents G1 (S, M, N), G2 (S, M, M), not symmetric; every
    fifth element of s cycles through 0, 1e-8, 0.3 and 100.  rounded: the values a float32 run sees"""
    N, M, Q, ard, S, own = case
    rng = np.random.default_rng(N * 1000003 + M * 1009 + Q * 31 + S * 7 + int(ard) + 2 * len(own))
    ax = lambda name: S if name in own else 1
    s = rng.uniform(0.05, 1.5, (ax('s'), N, Q))
    idx = np.arange(0, s.size, 5)
    s.reshape(-1)[idx] = np.resize([0.0, 1e-8, 0.3, 100.0], idx.size)
    p = dict(mu=rng.uniform(-2, 2, (ax('mu'), N, Q)), s=s, Z=rng.uniform(-2, 2, (ax('Z'), M, Q)),
             ls=rng.uniform(0.7, 1.5, (ax('ls'), Q if ard else 1)), var=rng.uniform(0.8, 1.6, (ax('var'), 1)),
             G1=rng.standard_normal((S, M, N)), G2=rng.standard_normal((S, M, M)))
    return {k: torch.as_tensor(v).float().double() if rounded else torch.as_tensor(v) for k, v in p.items()}


def _magnitudes(mu, s, Z, ls, var, G1, G2, P1, p2):
    """the sum of the magnitudes of the terms of each gradient of sum(G1 Psi1) + sum(G2 Psi2): |cotangent| * term * |d log term / d operand|"""
    Q = mu.shape[1]
    l2 = (ls * ls).expand(Q)
    a1, a2 = 1 / (s + l2), 1 / (2 * s + l2)
    d = (mu[None] - Z[:, None]).abs()                                    # (M, N, Q)
    w1 = (G1.abs() * P1)[..., None]                                      # (M, N, 1)
    dz = (Z[:, None] - Z[None]).abs()                                    # (M, M, Q)
    e = (mu[:, None, None] - 0.5 * (Z[:, None] + Z[None])[None]).abs()   # (N, M, M, Q)
    w2 = (G2.abs()[None] * p2)[..., None]                                # (N, M, M, 1)
    A2 = a2[:, None, None]
    t_z = w2 * (A2 * e + dz[None] / (2 * l2))
    dl1 = (w1 * 0.5 * (a1[None] ** 2 * d * d + (a1 * s / l2)[None])).sum((0, 1))
    dl2 = (w2 * ((a2 * s / l2)[:, None, None] + dz[None] ** 2 / (4 * l2 * l2) + A2 ** 2 * e * e)).sum((0, 1, 2))
    dl = 2 * ls * (dl1 + dl2 if ls.numel() == Q else (dl1 + dl2).sum().reshape(1))
    return dict(mu=(w1 * a1[None] * d).sum(0) + (w2 * 2 * A2 * e).sum((1, 2)),
                s=(w1 * 0.5 * a1[None] * (a1[None] * d * d + 1)).sum(0) + (w2 * A2 * (2 * A2 * e * e + 1)).sum((1, 2)),
                Z=(w1 * a1[None] * d).sum(1) + t_z.sum((0, 2)) + t_z.sum((0, 1)), ls=dl, var=(w1.sum() + 2 * w2.sum()) / var)


@functools.lru_cache(maxsize=None)
def _reference(case, rounded=False):
    """Psi1 (S, M, N), Psi2 (S, M, M), the gradients of sum(G1 Psi1) + sum(G2 Psi2) shaped like the operands (summed over the samples that share
    them) and the magnitude sums of all of these; rows in chunks of 512 (the sum is linear in the rows)"""
    N, M, Q, ard, S, own = case
    p = _inputs(case, rounded)
    out = dict(Psi1=[], Psi2=[], grad={k: torch.zeros_like(p[k]) for k in OPS}, mag={k: torch.zeros_like(p[k]) for k in OPS})
    for smp in range(S):
        leaf = {k: p[k][smp if k in own else 0].clone().requires_grad_(True) for k in OPS}
        P1s, P2 = [], torch.zeros(M, M, dtype=torch.float64)
        for r0 in range(0, N, 512):
            mu, s, G1 = leaf['mu'][r0:r0 + 512], leaf['s'][r0:r0 + 512], p['G1'][smp][:, r0:r0 + 512]
            P1 = R.psi1(mu, s, leaf['Z'], leaf['ls'], leaf['var'])
            p2 = R.psi2n(mu, s, leaf['Z'], leaf['ls'], leaf['var'])
            ((G1 * P1).sum() + (p['G2'][smp][None] * p2).sum()).backward()
            with torch.no_grad():
                mg = _magnitudes(mu, s, leaf['Z'], leaf['ls'], leaf['var'], G1, p['G2'][smp], P1, p2)
                for k in OPS:
                    if k in ('mu', 's'):
                        out['mag'][k][smp if k in own else 0][r0:r0 + 512] += mg[k]
                    else:
                        out['mag'][k][smp if k in own else 0] += mg[k]
                P1s.append(P1.detach())
                P2 += p2.sum(0)
        out['Psi1'].append(torch.cat(P1s, 1))
        out['Psi2'].append(P2)
        for k in OPS:
            out['grad'][k][smp if k in own else 0] += leaf[k].grad
    out['Psi1'], out['Psi2'] = torch.stack(out['Psi1']), torch.stack(out['Psi2'])
    return out


def _close(got, ref, mag, dtype, what):
    rtol, atol = BARS[dtype]
    got, ref, mag = got.double().cpu(), ref.double(), mag.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    worst = float((err - (rtol * mag + atol)).max())
    assert worst <= 0, (what, float(err.max()), float(mag.max()), worst)


def _device(p, dtype):
    return {k: v.to(dtype).cuda().contiguous() for k, v in p.items()}


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_and_reverse(case, dtype):
    from mxfusion_amd import ops
    N, M, Q, ard, S, own = case
    ref = _reference(case, dtype == torch.float32)          # the reference of a float32 run sees the rounded operands
    d = _device(_inputs(case), dtype)
    args = [d[k] for k in OPS] + [ard]
    Psi1, Psi2 = ops.psi_rbf(*args)
    _close(Psi1, ref['Psi1'], ref['Psi1'], dtype, 'Psi1')
    _close(Psi2, ref['Psi2'], ref['Psi2'], dtype, 'Psi2')
    assert torch.equal(Psi2, Psi2.transpose(1, 2)), 'Psi2 is not bitwise symmetric'
    acc = {k: torch.full_like(d[k], 0.5) for k in OPS}          # accumulated into pre-filled buffers
    ops.psi_rbf_bwd_(*args, d['G1'], d['G2'], *[acc[k] for k in OPS])
    for k in OPS:
        _close(acc[k] - 0.5, ref['grad'][k], ref['mag'][k] + 0.5, dtype, 'd' + k)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_null_outputs_and_null_cotangents(dtype):
    """each output null in turn, then each cotangent: what remains equals the matching part of the full call"""
    from mxfusion_amd import ops
    case = (65, 17, 3, True, 2, frozenset(['mu', 's']))
    d = _device(_inputs(case), dtype)
    args = [d[k] for k in OPS] + [True]
    P1, P2 = ops.psi_rbf(*args)
    assert ops.psi_rbf(*args, want_psi2=False)[1] is None and ops.psi_rbf(*args, want_psi1=False)[0] is None
    assert torch.equal(ops.psi_rbf(*args, want_psi2=False)[0], P1)
    _close(ops.psi_rbf(*args, want_psi1=False)[1], P2.double().cpu(), P2.double().cpu(), dtype, 'Psi2 alone')
    full = {}
    for G1, G2 in ((d['G1'], None), (None, d['G2'])):
        acc = {k: torch.zeros_like(d[k]) for k in OPS}
        ops.psi_rbf_bwd_(*args, G1, G2, *[acc[k] for k in OPS])
        full[G1 is None] = acc
    both = {k: torch.zeros_like(d[k]) for k in OPS}
    ops.psi_rbf_bwd_(*args, d['G1'], d['G2'], *[both[k] for k in OPS])
    rtol = 1e-9 if dtype == torch.float64 else 1e-4
    for k in OPS:
        parts = full[False][k].double() + full[True][k].double()
        scale = full[False][k].double().abs() + full[True][k].double().abs()
        assert bool(((both[k].double() - parts).abs() <= rtol * scale + 1e-5 * rtol).all()), k
        only = {j: (torch.zeros_like(d[j]) if j == k else None) for j in OPS}
        ops.psi_rbf_bwd_(*args, d['G1'], d['G2'], *[only[j] for j in OPS])
        assert bool(((only[k].double() - both[k].double()).abs() <= rtol * scale + 1e-5 * rtol).all()), k


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_zero_variance_is_the_gram(dtype):
    """s = 0: Psi1 = K(Z, X) and Psi2 = K K^T of the library's own Gram kernel"""
    from mxfusion_amd import ops
    d = _device(_inputs((65, 17, 3, True, 1, ALL)), dtype)
    zero = torch.zeros_like(d['s'])
    Psi1, Psi2 = ops.psi_rbf(d['mu'], zero, d['Z'], d['ls'], d['var'], True)
    K = ops.gram('rbf', d['Z'], d['mu'], d['ls'], d['var'], True).double().cpu()
    _close(Psi1, K, K, dtype, 'Psi1 at s = 0')
    _close(Psi2, K @ K.transpose(1, 2), K @ K.transpose(1, 2), dtype, 'Psi2 at s = 0')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
def test_far_rows_are_finite_zeros(dtype):
    """rows 50 lengthscales from every z: zeros in the values and finite zeros in the gradients, next to ordinary rows that keep theirs"""
    from mxfusion_amd import ops
    p = _inputs((65, 17, 3, True, 1, ALL))
    p['mu'][0, ::2] = 50.0 * p['ls'].max() + 2.0 + p['mu'][0, ::2].abs()
    p['s'][0, ::2] = torch.as_tensor([0.0, 1e-8, 0.3])
    d = _device(p, dtype)
    args = [d[k] for k in OPS] + [True]
    Psi1, Psi2 = ops.psi_rbf(*args)
    assert bool(torch.isfinite(Psi1).all()) and bool(torch.isfinite(Psi2).all())
    assert float(Psi1[0, :, ::2].abs().max()) == 0.0 and float(Psi1[0, :, 1::2].abs().max()) > 0.0
    acc = {k: torch.zeros_like(d[k]) for k in OPS}
    ops.psi_rbf_bwd_(*args, d['G1'], d['G2'], *[acc[k] for k in OPS])
    for k in OPS:
        assert bool(torch.isfinite(acc[k]).all()), k
    assert float(acc['mu'][0, ::2].abs().max()) == 0.0 and float(acc['s'][0, ::2].abs().max()) == 0.0
    assert float(acc['mu'][0, 1::2].abs().max()) > 0.0


def test_status_codes():
    """Q above MXF_PSI_MAX_Q is -3, a null mu is -2, and neither touches a buffer"""
    from mxfusion_amd import _lib, ops
    assert _lib.PSI_MAX_Q >= 16
    Q = _lib.PSI_MAX_Q + 1
    mk = lambda *shape: torch.ones(shape, dtype=torch.float64).cuda()
    with pytest.raises(_lib.MXFError, match=r'\(-3\)'):
        ops.psi_rbf(mk(1, 4, Q), mk(1, 4, Q), mk(1, 3, Q), mk(1, 1), mk(1, 1), False)
    mu, Z, one = mk(1, 4, 2), mk(1, 3, 2), mk(1, 1)
    out = torch.full((1, 3, 4), 7.0, dtype=torch.float64).cuda()
    with pytest.raises(_lib.MXFError, match=r'\(-2\)'):
        _lib.call('mxf_psi_rbf_fwd', ops._h(mu), _lib.F64, 1, 4, 3, 2, None, 0, mu.data_ptr(), 0, Z.data_ptr(), 0, one.data_ptr(), 0, 0, one.data_ptr(),
                  0, out.data_ptr(), None, ops._stream())
    assert float((out - 7.0).abs().max()) == 0.0
