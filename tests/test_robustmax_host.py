"""Host-side tests of the robust-max likelihood (no GPU): the new entry points in the header, the binding and the built library; the float64
restatement tests/_robustmax_ref.py against the two-class closed form and against a 200-node rule; the one-row functions of
mxfusion_amd/csrc/likelihood.h, built with the system C++ compiler, against autograd on the restatement."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _robustmax_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_robustmax_expect', 'mxf_robustmax_probs')
t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def test_new_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert '#define MXF_ROBUSTMAX_MAX_C %d' % _lib.ROBUSTMAX_MAX_C in header and _lib.ROBUSTMAX_MAX_C == 32


def test_exports_and_no_cpu_fallback():
    from mxfusion_amd import _lib, ops
    from mxfusion_amd.modules import gp_modules
    from mxfusion_amd.modules.gp_modules import RobustMax, BernoulliLogit
    assert gp_modules.RobustMax is RobustMax
    lik = RobustMax(3)
    assert lik.num_latent == 3 and lik.num_classes == 3 and BernoulliLogit().num_latent is None
    for bad in (1, 33, 2.5):
        with pytest.raises(ValueError):
            RobustMax(bad)
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            RobustMax(3, epsilon=bad)
    m, v = torch.zeros(1, 4, 3, dtype=torch.float64), torch.ones(1, 4, dtype=torch.float64)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.robustmax_probs(m, v)
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.robustmax_expect_(torch.zeros(1, 4, 1, dtype=torch.float64), m, v, 1e-3, 1.0, torch.zeros(1, dtype=torch.float64))


def test_check_labels_names_the_first_bad_label():
    from mxfusion_amd.modules.gp_modules import RobustMax
    RobustMax.check_labels(torch.tensor([[0.0], [2.0], [1.0]]), 3)
    for bad in (3.0, -1.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match='flat index 1'):
            RobustMax.check_labels(torch.tensor([[0.0], [bad], [7.0]]), 3)


def test_two_classes_equal_the_closed_form():
    """C = 2: P(f_y > f_c) = Phi((m_y - m_c) / sqrt(2 v)); the 20-node restatement to 1e-9 on m in [-3, 3], v in [1e-3, 4]"""
    rng = np.random.default_rng(0)
    N = 400
    m, v = t64(rng.uniform(-3, 3, (N, 2))), t64(np.exp(rng.uniform(np.log(1e-3), np.log(4.0), N)))
    y = torch.as_tensor(rng.integers(0, 2, N))
    d = torch.gather(m, 1, y[:, None])[:, 0] - torch.gather(m, 1, 1 - y[:, None])[:, 0]
    exact = torch.special.ndtr(d / torch.sqrt(2.0 * v))
    err = float((R.p_correct(y, m, v, 20) - exact).abs().max())
    print('C = 2, 20 nodes against the closed form:', err)
    assert err <= 1e-9
    pr = R.probs(m, v, 20)
    assert float((pr.sum(-1) - 1.0).abs().max()) <= 2e-9


def test_three_classes_twenty_against_two_hundred_nodes():
    rng = np.random.default_rng(1)
    N = 400
    m, v = t64(rng.uniform(-3, 3, (N, 3))), t64(np.exp(rng.uniform(np.log(1e-3), np.log(4.0), N)))
    y = torch.as_tensor(rng.integers(0, 3, N))
    err = float((R.p_correct(y, m, v, 20) - R.p_correct(y, m, v, 200)).abs().max())
    print('C = 3, 20 against 200 nodes:', err)
    assert err <= 1e-6


ROWS = [  # y, m0, m1, m2
    (0, 0.5, 0.5, -0.2),        # an exact tie m_y = m_c
    (1, 0.5, 0.5, 0.5),         # all tied
    (1, 0.49, 0.5, -0.5),       # a gap of 0.01, y the larger
    (0, 0.49, 0.5, -0.5),       # ... y the smaller
    (2, 1.2, 0.2, 0.7),         # y between the others: d of both signs
    (0, 1.0, 0.0, -39.0),       # gaps of 1 and 40, y the largest
    (1, 1.0, 0.0, -39.0),       # ... y in the middle
    (2, 1.0, 0.0, -39.0),       # ... y 40 below: p underflows
]
VARS = (0.0, 1e-12, 1e-8, 0.3, 25.0)
POINTS = [(y, v, a, b, c) for v in VARS for (y, a, b, c) in ROWS]
NQ = 20


def _reference_row(y, v, m, cast):
    """value, dm (3), dv by autograd on the restatement at the argument a precision saw, and the float32 bar of the row (docstring below)"""
    mt = torch.tensor([float(cast(x)) for x in m], dtype=torch.float64, requires_grad=True)
    vt = torch.tensor(float(cast(v)), dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y)
    p = R.p_correct(yt, mt, vt, NQ)
    dm, dv = torch.autograd.grad(p, [mt, vt])
    # the sensitivity of the node terms to z
    with torch.no_grad():
        P, w = R.node_products(yt, mt, vt, NQ)
        x, _ = R.L.rule(NQ)
        d = (mt[y] - mt) / math.sqrt(max(float(vt), R.FLOOR))
        z = d[None, :] + math.sqrt(2.0) * x[:, None]
        lam = torch.exp(-0.5 * z * z - R.L.LOG_SQRT_2PI - torch.special.log_ndtr(z))
        lam[:, y] = 0.0
        dz = d.abs()[None, :] + math.sqrt(2.0) * x.abs()[:, None]
        live = (P * w) >= 1e-9 * float((P * w).sum())
        first = (lam * dz).sum(-1)
        second = torch.where(lam > 1e-30, (z.abs() + lam) * dz, torch.zeros_like(z)).max(-1).values
        sens = float((first + second)[live].max()) if bool(live.any()) else 0.0
    bar = 2.0 ** -24 * (8.0 + 4.0 * sens) + NQ * 1e-9
    return np.array([float(p.detach())] + [float(g) for g in dm] + [float(dv)]), bar


def test_row_functions_against_the_restatement(tmp_path):
    """tests/host/robustmax_check.cpp prints p, dp/dm (3) and dp/dv of mxf_robustmax_row at C = 3 in both precisions, at v = 0, 1e-12, 1e-8, 0.3
    and 25, at exact ties and at gaps of 0.01, 1 and 40; against autograd on the restatement at the argument each precision saw.
    float64: 1e-12 relative or 1e-300 absolute.  float32, from the rounding of z: z = (m_y - m_c) / sqrt(v) + x_k comes out of four rounded
    operations and a rounded node, |dz| <= 4 (|d_c| + |x_k|) 2^-24; a node term w_k P_k then moves by sum_c lambda(z_kc) |dz_kc| relative,
    and its factor lambda(z_kc) in a gradient by (|z_kc| + lambda) |dz_kc| more (lambda' = -lambda (z + lambda)).  The bar of a row is
    2^-24 (8 + 4 max_k [sum_c lambda_kc D_kc + max_c (|z_kc| + lambda_kc) D_kc]), D_kc = |d_c| + |x_k|, over the nodes that carry at least 1e-9
    of the sum, plus nq 1e-9 for the others, the 8 for the roundings of the sums; relative, or 1e-30 absolute (a lambda that underflows in
    float32).  Every value is finite; the v = 0 rows equal the v = 1e-12 rows in p and dm, and their dv is exactly 0."""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path / 'robustmax_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'robustmax_check.cpp'), '-o', exe, '-lm'], check=True)
    x, w = np.polynomial.hermite.hermgauss(NQ)
    lines = ['%d' % NQ, ' '.join('%.17g' % t for t in x), ' '.join('%.17g' % t for t in w)]
    lines += ['%d %.17g %.17g %.17g %.17g' % pt for pt in POINTS]
    out = subprocess.run([exe], input='\n'.join(lines), capture_output=True, text=True, check=True).stdout
    got = np.array([[float(t) for t in line.split()] for line in out.strip().split('\n')])
    assert got.shape == (len(POINTS), 10) and np.isfinite(got).all()
    worst = {'float64': 0.0, 'float32': 0.0}
    for row, pt in zip(got, POINTS):
        y, v, m = pt[0], pt[1], pt[2:]
        for cols, cast in ((row[:5], np.float64), (row[5:], np.float32)):
            ref, bar32 = _reference_row(y, v, m, cast)
            rtol, atol = (1e-12, 1e-300) if cast is np.float64 else (bar32, 1e-30)
            err = np.abs(cols - ref)
            worst[cast.__name__] = max(worst[cast.__name__], float((err / np.maximum(np.abs(ref), 1e-30 if cast is np.float32 else 1e-300)).max()))
            assert (err <= rtol * np.abs(ref) + atol).all(), (pt, cast.__name__, rtol, cols, ref)
    print('worst relative error', worst)
    k = len(ROWS)
    assert (got[:k, [0, 1, 2, 3, 5, 6, 7, 8]] == got[k:2 * k, [0, 1, 2, 3, 5, 6, 7, 8]]).all()
    assert (got[:k, [4, 9]] == 0).all()
