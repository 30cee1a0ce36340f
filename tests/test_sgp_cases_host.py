"""Host checks of the sparse-GP shape sweep's inputs (tests/_sgp_cases.py): every case meets the builder's condition-number limit and has
a finite oracle, the limit refuses what it should, and the grading is sensitive to the defect the sweep was written for -- dpsi1 = a / s2^2
(M x P) with its entries from M M on left out gives a dY that misses the float64 AND the float32 tolerance at every P > M shape."""
import numpy as np
import pytest
import torch

import _sgp_cases as C

CASES = [(s, k, a) for s in C.SHAPES for k in C.KINDS for a in (True, False)]
P_GT_M = [s for s in C.SHAPES if s[3] > s[1]]


def test_the_shapes_cross_the_seams_they_name():
    assert len(set(C.SHAPES)) == 8 and max(C.SHAPES) == (70, 65, 2, 3)
    assert P_GT_M == [(5, 3, 2, 7), (3, 17, 1, 20), (2, 31, 4, 33), (40, 33, 3, 40)]
    Ms = {s[1] for s in C.SHAPES}
    assert {1, 3, 16, 17, 31, 32, 33, 65} == Ms
    assert any(s[0] < s[1] for s in C.SHAPES) and any(s[2] == 1 and s[1] > 1 for s in C.SHAPES) and any(s[3] == 1 for s in C.SHAPES)


@pytest.mark.parametrize('shape,kind,ard', CASES, ids=['%s-%s-%s' % ('x'.join(map(str, s)), k, 'ard' if a else 'iso') for s, k, a in CASES])
def test_case_is_well_conditioned_and_finite(shape, kind, ard):
    a, ref, cond = C.build(shape, kind, ard)
    B, M, Q, P = shape
    assert 1.0 <= cond <= C.COND_LIMIT
    assert a['X'].shape == (B, Q) and a['Y'].shape == (B, P) and a['Z'].shape == (M, Q) and a['ls'].shape == ((Q,) if ard else (1,))
    assert np.all(np.abs(a['X']) <= 2) and float(a['var'][0]) == 1.3 and float(a['noise'][0]) == 0.05
    c = C.C_LS * M ** (-1.0 / Q)
    assert np.all(a['ls'] >= 0.8 * c) and np.all(a['ls'] <= 1.2 * c)
    assert np.isfinite(ref['logL']) and all(np.isfinite(ref[k]).all() for k in C.POST_KEYS + C.GRAD_KEYS)
    assert ref['wv'].shape == (M, P) and ref['L'].shape == ref['LA'].shape == (M, M) and ref['dls'].shape == a['ls'].shape
    assert C.failed_keys(ref, ref, shape, True) == []
    assert C.build(shape, kind, ard)[0] is a, 'built once, shared'
    with pytest.raises(ValueError):
        a['Y'][0, 0] = 0.


def test_cond_1_and_the_limit():
    assert C.cond_1(np.diag([4., 1., 0.5])) == 8.
    K = np.array([[2., 1.], [1., 2.]])
    assert abs(C.cond_1(K) - 3.0) < 1e-14                     # |K|_1 = 3, K^-1 = [[2, -1], [-1, 2]] / 3: |K^-1|_1 = 1
    # the limit is live: twice the lengthscale at (70, 65, 2, 3) with RBF is past it
    a = C.inputs((70, 65, 2, 3), 'rbf', False)
    assert C.cond_1(C.kuu('rbf', False, a['Z'], a['ls'], a['var'], C.JITTER)) <= C.COND_LIMIT
    assert C.cond_1(C.kuu('rbf', False, a['Z'], 2 * a['ls'], a['var'], C.JITTER)) > C.COND_LIMIT
    assert (C.SEED, C.C_LS) == (20, 2.0)


@pytest.mark.parametrize('shape', P_GT_M, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('ard', [True, False], ids=['ard', 'iso'])
def test_grading_sees_a_truncated_dpsi1(shape, kind, ard):
    """dY = Kuf^T dpsi1 - Y / s2 with dpsi1 = wv / s2 is the oracle's dY; with the flat entries M M .. M P - 1 of dpsi1 zeroed it fails both
    tolerances, and so does dKuf = ... + dpsi1 Y^T (seen in dvar, the sum of dKuf * Kuf / var)."""
    a, ref, _ = C.build(shape, kind, ard)
    B, M, Q, P = shape
    k = C.KERNELS[kind](Q, ARD=ard)
    with torch.no_grad():
        Kuf = k.K(torch.tensor(a['Z'])[None], torch.tensor(a['X'])[None], **C.kernel_params(k, torch.tensor(a['ls']), torch.tensor(a['var'])))[0].numpy()
    s2 = float(a['noise'][0])
    dpsi1 = ref['wv'] / s2
    dY = Kuf.T @ dpsi1 - a['Y'] / s2
    assert np.allclose(dY, ref['dY'], rtol=1e-9, atol=1e-9 * np.abs(ref['dY']).max())
    cut = dpsi1.copy().reshape(-1)
    cut[M * M:] = 0.
    cut = cut.reshape(M, P)
    d_dY, d_dvar = Kuf.T @ (dpsi1 - cut), ((dpsi1 - cut) @ a['Y'].T * Kuf).sum() / float(a['var'][0])
    assert np.abs(d_dY).max() > 0.1 * max(1., np.abs(ref['dY']).max()) and abs(d_dvar) > 0.1 * max(1., abs(float(ref['dvar'][0])))
    for float64 in (True, False):
        got = dict(ref, dY=dY - d_dY, dvar=ref['dvar'] - d_dvar)
        assert C.failed_keys(got, ref, shape, float64) == ['dY', 'dvar'], (float64, C.failed_keys(got, ref, shape, float64))
