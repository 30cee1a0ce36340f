"""CPU tests of the non-Gaussian SVGP likelihoods: the entry points are declared, bound and exported; nothing runs without a GPU; the link
functions of mxfusion_amd/csrc/likelihood.h -- host code as well as device code -- agree with SciPy over the tails; and the 20-node
Gauss-Hermite rule of the reference (tests/_lik_ref.py) is as good as the closed forms say."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _lik_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mxf_lik_expect', 'mxf_lik_expect_elem', 'mxf_lik_moments')


def test_new_entry_points_are_declared_bound_and_exported():
    from mxfusion_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'mxf_gp.h')).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + '(' in header and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES and getattr(lib, name, None) is not None, name
        decl = header[header.index('int ' + name + '('):].split(';')[0]
        assert len(_lib.SIGNATURES[name]) == len(decl.split(',')) - 1, name
    assert 'No reference counterpart' in header[header.index('MXF_LIK_BERNOULLI_LOGIT') - 3000:header.index('MXF_LIK_BERNOULLI_LOGIT')]
    assert (_lib.LIK_BERNOULLI_LOGIT, _lib.LIK_BERNOULLI_PROBIT, _lib.LIK_POISSON_EXP) == (0, 1, 2)
    assert 'enum { MXF_LIK_BERNOULLI_LOGIT = 0, MXF_LIK_BERNOULLI_PROBIT = 1, MXF_LIK_POISSON_EXP = 2 }' in header
    assert '#define MXF_LIK_MAX_NODES 64' in header and _lib.LIK_MAX_NODES == 64
    assert ops.LIK_KIND == {'bernoulli_logit': 0, 'bernoulli_probit': 1, 'poisson_exp': 2}
    with pytest.raises(ValueError):
        ops.lik_nodes(65)


def test_exports_and_parameter_lists():
    from mxfusion_amd.modules import gp_modules
    from mxfusion_amd.modules.gp_modules import SVGPLikelihood, BernoulliLogit, BernoulliProbit, PoissonExp
    from mxfusion_amd.modules.gp_modules.svgp_likelihood import SVGPLikelihoodLogPdf, SVGPLikelihoodPrediction
    for name in ('SVGPLikelihood', 'BernoulliLogit', 'BernoulliProbit', 'PoissonExp'):
        assert hasattr(gp_modules, name), name
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(SVGPLikelihood.__init__) == ['self', 'X', 'kernel', 'likelihood', 'inducing_inputs', 'num_inducing', 'mean', 'rand_gen',
                                              'dtype', 'ctx']
    assert names(SVGPLikelihood.define_variable) == ['X', 'kernel', 'likelihood', 'shape', 'inducing_inputs', 'num_inducing', 'mean',
                                                     'rand_gen', 'dtype', 'ctx']
    assert inspect.signature(SVGPLikelihood.__init__).parameters['num_inducing'].default == 10
    assert names(SVGPLikelihoodLogPdf.__init__) == ['self', 'model', 'posterior', 'observed', 'jitter']
    assert names(SVGPLikelihoodPrediction.__init__) == ['self', 'model', 'posterior', 'observed', 'latent', 'jitter']
    for cls, kind in ((BernoulliLogit, 'bernoulli_logit'), (BernoulliProbit, 'bernoulli_probit'), (PoissonExp, 'poisson_exp')):
        assert cls().num_nodes == 20 and cls().kind == kind and cls(num_nodes=7).num_nodes == 7
    assert SVGPLikelihood.row_additive is True


def _cpu_module(P=1):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.modules.gp_modules import SVGPLikelihood, BernoulliLogit
    m = Model()
    m.N = Variable()
    m.X = Variable(shape=(m.N, 2))
    m.Z = Variable(shape=(3, 2))
    m.Y = SVGPLikelihood.define_variable(X=m.X, kernel=RBF(input_dim=2, ARD=True, dtype='float64'), likelihood=BernoulliLogit(),
                                         inducing_inputs=m.Z, shape=(m.N, P), dtype='float64')
    return m


def test_module_structure():
    gp = _cpu_module(P=2).Y.factor
    post = gp._extra_graphs[0]
    assert (tuple(post.qU_mean.shape), tuple(post.qU_cov_W.shape), tuple(post.qU_cov_diag.shape)) == ((3, 2), (3, 3), (3,))
    assert post.qU_cov_diag.transformation is not None and post.qU_cov_W.transformation is None
    assert not hasattr(gp._module_graph, 'noise_var') and gp.input_names == ['X', 'inducing_inputs']
    assert gp.svgp_log_pdf.log_pdf_scaling == 1 and gp.svgp_log_pdf.kl_weight == 1.0 and gp.svgp_predict.latent is False
    assert gp._draw_samples_algorithms == {}


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU behaviour')
def test_no_cpu_fallback():
    from mxfusion_amd import _lib, ops
    from mxfusion_amd.util.inference import VariablesDict
    t = torch.zeros(1, 4, 1, dtype=torch.float64)
    with pytest.raises(_lib.MXFError):
        ops.lik_expect_elem('bernoulli_logit', t, t, torch.ones(1, 4, dtype=torch.float64))
    m = _cpu_module()
    gp = m.Y.factor
    post = gp._extra_graphs[0]
    d = lambda *s: torch.ones(*s, dtype=torch.float64)
    variables = VariablesDict({m.X.uuid: d(1, 4, 2), m.Z.uuid: d(1, 3, 2), m.Y.uuid: d(1, 4, 1), post.qU_mean.uuid: d(1, 3, 1),
                               post.qU_cov_W.uuid: d(1, 3, 3), post.qU_cov_diag.uuid: d(1, 3)})
    variables.update({v.uuid: d(1, *v.shape) for v in gp.kernel.parameters.values()})
    with pytest.raises(_lib.MXFError):
        gp.log_pdf(F=None, variables=variables)


BARS = {'double': (1e-12, 1e-14), 'float': (4 * 2.0 ** -24, 1e-6)}


def test_link_functions_against_scipy(tmp_path):
    """tests/host/lik_check.cpp, built with the system C++ compiler, prints g, g', g'' and mu of the three kinds in both precisions: the
    Bernoulli kinds at z = (2y - 1) f on 801 points of [-40, 40] (y = 1 and y = 0 both), the Poisson kind at 401 points of f in [-20, 20] for
    y in {0, 1, 50}.  Against SciPy (tests/_lik_ref.py) at the argument each precision saw.  float64: 1e-12 relative or 1e-14 absolute;
    float32: 4 * 2^-24 relative or 1e-6 absolute; every value finite."""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path / 'lik_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'lik_check.cpp'), '-o', exe, '-lm'], check=True)
    rows = [(k, y, f) for k in (0, 1) for y in (1.0, 0.0) for f in np.linspace(-40.0, 40.0, 801)]
    rows += [(2, y, f) for y in (0.0, 1.0, 50.0) for f in np.linspace(-20.0, 20.0, 401)]
    out = subprocess.run([exe], input='\n'.join('%d %.17g %.17g' % r for r in rows), capture_output=True, text=True, check=True).stdout
    got = np.array([[float(t) for t in line.split()] for line in out.strip().split('\n')])
    assert got.shape == (len(rows), 12) and np.array_equal(got[:, :3], np.array(rows))
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, 7].astype(np.float32), got[:, 2].astype(np.float32))
    for k, kind in enumerate(R.KINDS):
        sel = got[:, 0] == k
        y = got[sel, 1]
        for prec, fcol, col0 in (('double', 2, 3), ('float', 7, 8)):
            f = got[sel, fcol]
            ref = list(R.g_np(kind, y, f)) + [R.mu_np(kind, f)]
            rtol, atol = BARS[prec]
            for j, what in enumerate(('g', "g'", "g''", 'mu')):
                val = got[sel, col0 + j]
                err = np.abs(val - ref[j])
                ok = (err <= rtol * np.abs(ref[j])) | (err <= atol)
                i = int(np.argmax(np.where(ok, 0.0, err)))
                assert ok.all(), '%s %s<%s>: %d points off, worst at y = %r, f = %r: got %r, SciPy %r' % (
                    kind, what, prec, int((~ok).sum()), y[i], f[i], val[i], ref[j][i])
    # log Phi(-40) = -804.6 and the unit slope of lambda there: the tail the forms exist for
    i = rows.index((1, 1.0, -40.0))
    assert abs(got[i, 3] + 804.6084420137538) < 1e-9 and abs(got[i, 5] + 1.0) < 1e-3 and abs(got[i, 8] + 804.6084420137538) < 1e-3


def test_reference_mills_ratio_is_consistent():
    """The reference's own lambda(z) = phi / Phi switches at z = -5 from exp(log phi - log_ndtr) to a continued fraction: where both are
    accurate, z in [-8, -5], they agree (lambda + z carries 1 / 0.12 of lambda's 1e-13 there), and the fraction has converged."""
    z = np.linspace(-8.0, -5.0, 61)
    lam = np.exp(-0.5 * z * z - R.LOG_SQRT_2PI - R.special.log_ndtr(z))
    cf = np.zeros_like(z)
    for k in range(800, 0, -1):
        cf = k / (-z + cf)
    lam_cf, c_cf = R.mills_np(z)
    assert np.allclose(lam_cf, lam, rtol=1e-12, atol=0) and np.allclose(c_cf, lam + z, rtol=1e-10, atol=0)
    assert np.allclose(c_cf[:-1], cf[:-1], rtol=1e-14, atol=0)     # (depth 120 against 800: a few roundings apart; z = -5 itself is the other branch)
    zz = np.array([-40.0, -100.0])
    lam_f, c_f = R.mills_np(zz)
    t = -zz                                             # the asymptotic series lambda + z = 1/t - 2/t^3 + 10/t^5 - 74/t^7 + ...
    assert np.allclose(c_f, 1 / t - 2 / t ** 3 + 10 / t ** 5 - 74 / t ** 7, rtol=1e-9, atol=0)


PRICE_GAP = {'bernoulli_logit': 9.74e-6, 'bernoulli_probit': 3.19e-5, 'poisson_exp': 9.59e-14}       # measured by the test below, which prints them


def test_reference_quadrature_against_closed_forms():
    """The 20-node rule of the reference at 2000 points, m uniform in [-3, 3], v log-uniform in [1e-4, 4]; measured / asserted:
         E[Phi(f)] against Phi(m / sqrt(1 + v))     2.1e-5 / 1e-4 absolute
         E[exp f] against exp(m + v / 2)            9e-16 / 1e-13 relative
         E[log Phi] against a 200-node rule         4.2e-6 / 2e-5 absolute
         E[log sigmoid] against a 200-node rule     1.4e-6 / 1e-5 absolute
    and the Price form of d/dv against autograd through the forward sum (the two differ by the quadrature error): worst absolute
    difference 9.74e-6 (logit), 3.19e-5 (probit), 9.59e-14 (Poisson: exp is integrated exactly, what is left is rounding at |dv| <= 74) with
    y = 1 for the Bernoulli kinds and y in {0, 1, 5} for Poisson -- PRICE_GAP, asserted at four times that."""
    rng = np.random.default_rng(20)
    n = 2000
    m = torch.as_tensor(rng.uniform(-3.0, 3.0, (n, 1)))
    v = torch.as_tensor(np.exp(rng.uniform(np.log(1e-4), np.log(4.0), n)))
    e1, _ = R.moments('bernoulli_probit', m, v)
    assert float((e1[:, 0] - torch.as_tensor(R.special.ndtr(m[:, 0].numpy() / np.sqrt(1.0 + v.numpy())))).abs().max()) <= 1e-4
    e1, _ = R.moments('poisson_exp', m, v)
    exact = torch.exp(m[:, 0] + 0.5 * v)
    assert float(((e1[:, 0] - exact) / exact).abs().max()) <= 1e-13
    one = torch.ones(n, 1, dtype=torch.float64)
    for kind, bar in (('bernoulli_probit', 2e-5), ('bernoulli_logit', 1e-5)):
        assert float((R.expect_elem(kind, one, m, v, 20) - R.expect_elem(kind, one, m, v, 200)).abs().max()) <= bar, kind
    gaps = {}
    ys = {'bernoulli_logit': one, 'bernoulli_probit': one, 'poisson_exp': torch.as_tensor(rng.choice([0.0, 1.0, 5.0], (n, 1)))}
    for kind in R.KINDS:
        vv = v.clone().requires_grad_(True)
        auto, = torch.autograd.grad(R.expect_elem(kind, ys[kind], m, vv).sum(), vv)
        _, price = R.expect_grads(kind, ys[kind], m, v)
        gap = float((auto - price).abs().max())
        print('Price form against autograd, %s: %.3g' % (kind, gap))
        gaps[kind] = gap
    assert all(gaps[k] <= 4 * PRICE_GAP[k] for k in R.KINDS), gaps
