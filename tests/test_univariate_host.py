"""CPU tests of the univariate distributions: the new entry points are declared and exported, the classes refuse to run without a GPU, and
the special functions of mxfusion_amd/csrc/special.h -- host code as well as device code -- agree with SciPy."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_univariate_logpdf', 'mxf_univariate_logpdf_elem', 'mxf_univariate_logpdf_bwd')


def test_new_entry_points_are_declared_bound_and_exported():
    """tests/test_layout.py holds header, loader and library to each other symbol by symbol; this only asserts the new names are among them."""
    from mxfusion_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header and name in _lib.ALL_SYMBOLS and getattr(lib, name, None) is not None, name
    for cite in ('gamma.py:45-59', 'gamma.py:127-159', 'beta.py:46-68', 'laplace.py:37-55', 'uniform.py:38-62'):
        assert cite in header, cite
    assert (_lib.D_GAMMA, _lib.D_GAMMA_MV, _lib.D_BETA, _lib.D_LAPLACE, _lib.D_UNIFORM) == (0, 1, 2, 3, 4)


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_no_cpu_fallback():
    from mxfusion_amd import _lib
    from mxfusion_amd.components.distributions import Gamma, GammaMeanVariance, Beta, Laplace, Uniform, UnivariateDistribution
    for cls in (Gamma, GammaMeanVariance, Beta, Laplace, Uniform):
        f = cls.define_variable(shape=(3,)).factor
        assert isinstance(f, UnivariateDistribution) and [n for n, _ in f.outputs] == ['random_variable']
        t = torch.full((1, 3), 0.5, dtype=torch.float64)
        variables = {f.inputs[0][1].uuid: t * 0.5, f.inputs[1][1].uuid: t * 3, f.random_variable.uuid: t}
        with pytest.raises(_lib.MXFError):
            f.log_pdf(F=None, variables=variables)
        with pytest.raises(_lib.MXFError):
            f.log_pdf_sum(None, variables)


SHAPE_PARAMS = [0.05, 0.5, 1.0, 1.4616, 2.0, 5.9, 6.0, 6.1, 50.0, 1e4]


def test_special_functions_against_scipy(tmp_path):
    """tests/host/special_check.cpp, built with the system C++ compiler, prints mxf_lgamma and mxf_digamma in both precisions over 400
    log-spaced points of [1e-3, 1e5] and the shape parameters of the GPU test.  float64: 1e-12 relative, or 1e-14 absolute (near the zeros
    the value is what is left of a cancellation); float32: 4 * 2^-24 relative, or 1e-6 absolute."""
    from scipy import special
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path / 'special_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'special_check.cpp'), '-o', exe, '-lm'], check=True)
    xs = np.concatenate([np.logspace(-3, 5, 400), SHAPE_PARAMS])
    out = subprocess.run([exe], input='\n'.join('%.17g' % x for x in xs), capture_output=True, text=True, check=True).stdout
    got = np.array([[float(t) for t in line.split()] for line in out.strip().split('\n')])
    assert got.shape == (len(xs), 6) and np.array_equal(got[:, 0], xs)
    xf = xs.astype(np.float32).astype(np.float64)            # the argument the float32 columns were computed at
    assert np.array_equal(got[:, 3].astype(np.float32), xs.astype(np.float32))
    for name, col, x, ref, rtol, atol in (('lgamma<double>', 1, xs, special.gammaln(xs), 1e-12, 1e-14),
                                          ('digamma<double>', 2, xs, special.digamma(xs), 1e-12, 1e-14),
                                          ('lgamma<float>', 4, xf, special.gammaln(xf), 4 * 2.0 ** -24, 1e-6),
                                          ('digamma<float>', 5, xf, special.digamma(xf), 4 * 2.0 ** -24, 1e-6)):
        err = np.abs(got[:, col] - ref)
        ok = (err <= rtol * np.abs(ref)) | (err <= atol)
        i = int(np.argmax(np.where(ok, 0.0, err)))
        assert ok.all(), '%s: %d points off, worst at x = %r: got %r, SciPy %r' % (name, int((~ok).sum()), x[i], got[i, col], ref[i])
