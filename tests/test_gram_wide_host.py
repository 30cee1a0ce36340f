"""Host checks of the wide-input Gram passes (no GPU): the ABI in the header, the binding and the built library, and the pure launch plan that
is the entry points' argument check (csrc/gram_wide_plan.h): every pair owned once, the LDS within 64 KB, each refusal's code and reason."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = 'bwd esize kind S N N2 Q square has_X has_ls has_var has_K ldk'.split()
BASE = dict(bwd=0, esize=4, kind=0, S=1, N=300, N2=200, Q=64, square=0, has_X=1, has_ls=1, has_var=1, has_K=1, ldk=200)
SIZES = (1, 63, 64, 65, 129, 70000)          # around the 64 x 64 tile


def test_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mxf_gram_wide', 'mxf_gram_wide_bwd', 'mxf_gram_wide_configure'):
        assert 'int ' + name + '(' in header and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert len(_lib.SIGNATURES['mxf_gram_wide']) == len(_lib.SIGNATURES['mxf_gram'])             # argument for argument
    assert len(_lib.SIGNATURES['mxf_gram_wide_bwd']) == len(_lib.SIGNATURES['mxf_gram_bwd'])
    assert '#define MXF_GW_MAX_Q %d' % _lib.GW_MAX_Q in header and '#define MXF_GW_MIN_Q %d' % _lib.GW_MIN_Q in header and _lib.GW_MAX_Q >= 1024
    assert set(ops.WIDE_GRAM) == {torch.float32, torch.float64}
    with pytest.raises(_lib.MXFError, match='no CPU'):
        ops.gram_wide('rbf', torch.ones(1, 5, 20), None, torch.ones(1, 1), torch.ones(1, 1), False)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('gram_wide_plan') / 'gram_wide_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'gram_wide_plan_check.cpp'), '-o', exe], check=True)
    line = lambda r: ' '.join(str(int(r[c])) for c in COLS)
    return lambda reqs, text=False: subprocess.run([exe], input=('text 1\n' if text else '') + '\n'.join(line(r) for r in reqs), capture_output=True,
                                                   text=True, check=True).stdout.strip().split('\n')


def test_plan_owns_every_pair_once_within_the_lds(plan):
    reqs = [dict(BASE, bwd=b, esize=e, kind=k, S=S, N=n, N2=n2, Q=q, ldk=n2) for b in (0, 1) for e in (4, 8) for k, q in ((0, 17), (1, 32), (2, 33), (3, 1024))
            for S in (1, 3) for n in SIZES for n2 in SIZES]
    for r, out in zip(reqs, plan(reqs)):
        rc, qc, chunks, gx, gy, gz, lds, rmin, rmax, cmin, cmax = (int(t) for t in out.split())
        assert rc == 0 and (rmin, rmax, cmin, cmax) == (1, 1, 1, 1), (r, out)
        assert qc == (16 if r['esize'] == 4 else 8) and (chunks - 1) * qc < r['Q'] <= chunks * qc, (r, out)
        assert (gy - 1) * 64 < r['N'] <= gy * 64 and (gx - 1) * 64 < r['N2'] <= gx * 64 and gz == r['S'] and gy <= 65535, (r, out)
        e = r['esize']
        want = 4 * qc * (64 + 16 // e) * e + 4 * qc * e                  # two buffers each of xs, zs; of m2, il
        if r['bwd']:
            want += 2 * ((2 * qc * 65 * e + 15) // 16 * 16) + 2 * qc * 8 + 16 + 16 * 8
        assert lds == want and lds <= 64 * 1024, (r, out, want)


NULLS = 'null X, lengthscale, variance or matrix'
REFUSALS = [(dict(Q=16), -3, 'Q <= 16 belongs to the coordinate kernels (mxf_gram, mxf_gram_bwd)'), (dict(Q=16, has_X=0), -3, 'Q <= 16 belongs to the coordinate kernels (mxf_gram, mxf_gram_bwd)'),
            (dict(Q=16385), -3, 'Q above MXF_GW_MAX_Q input dimensions'), (dict(Q=16385, has_X=0), -3, 'Q above MXF_GW_MAX_Q input dimensions'),
            (dict(kind=4), -3, 'stationary kinds only (RBF, Matern12, Matern32, Matern52)'), (dict(kind=4, has_X=0), -3, 'stationary kinds only (RBF, Matern12, Matern32, Matern52)'),
            (dict(N=64 * 65535 + 1), -3, 'grid too large'), (dict(N=64 * 65535 + 1, has_X=0), -3, 'grid too large'), (dict(S=65536), -3, 'grid too large'),
            (dict(has_X=0), -2, NULLS), (dict(has_ls=0), -2, NULLS), (dict(has_var=0), -2, NULLS), (dict(has_K=0), -2, NULLS), (dict(has_K=0, bwd=1), -2, NULLS),
            (dict(N=0), -2, 'S, N, N2 >= 1'), (dict(N2=0), -2, 'S, N, N2 >= 1'), (dict(S=0), -2, 'S, N, N2 >= 1'), (dict(esize=2), -2, 'float32 or float64'),
            (dict(ldk=199), -2, 'negative sample stride or row stride below N2')]


@pytest.mark.parametrize('over,rc,why', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_plan_refusals(plan, over, rc, why):
    code, _, text = plan([dict(BASE, **over)], text=True)[0].partition(' ')
    assert (int(code), text) == (rc, why)
    assert plan([dict(BASE, N=64 * 65535, ldk=200)])[0].split()[4] == '65535'       # the largest grid that fits
    assert plan([dict(BASE, square=1, N=130, N2=0, ldk=130)])[0].split()[:6] == ['0', '16', '4', '3', '3', '1']      # a square Gram ignores N2
