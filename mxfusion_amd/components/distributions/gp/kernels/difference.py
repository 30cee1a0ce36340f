"""Covariances of the per-dimension differences tau_d = x_d - x'_d: Periodic, RationalQuadratic and SpectralMixture (the reference has none
of them; the conventions are GPflow's / scikit-learn's and Wilson & Adams 2013).  K is the HIP difference-form Gram pass and its reverse mode
(mxf_gram_diff / mxf_gram_diff_bwd).  They are NativeKernels without a `_kind`, so fused_spec() stays None and every fused composite, the
two-kernel Gram, the matrix-free product, the psi statistics, pathwise sampling and Vecchia treat them as they treat any kernel they do not
cover: the generic path (materialised Grams combined by torch) or a ModelSpecificationError."""
import numpy as np
import torch

from mxfusion_amd import ops
from mxfusion_amd.common.exceptions import ModelSpecificationError
from mxfusion_amd.components.variables.variable import Variable
from mxfusion_amd.components.variables.var_trans import PositiveTransformation
from .kernel import NativeKernel, _GramDiffFn


def _positive(value, shape):
    return value if isinstance(value, Variable) else Variable(shape=shape, transformation=PositiveTransformation(), initial_value=value)


def _check_dims(kernel, Q, limit):
    if Q > limit:
        raise ModelSpecificationError('%s covers at most %d input dimensions (the difference-form Gram pass keeps them in registers); got %d'
                                      % (type(kernel).__name__, limit, Q))


class Periodic(NativeKernel):
    """k = variance exp(-1/2 sum_d sin^2(pi tau_d / period_d) / lengthscale_d^2); with ARD one lengthscale and one period per dimension."""

    def __init__(self, input_dim, ARD=False, variance=1., lengthscale=1., period=1., name='periodic', active_dims=None, dtype=None, ctx=None):
        super(Periodic, self).__init__(input_dim=input_dim, name=name, active_dims=active_dims, dtype=dtype, ctx=ctx)
        _check_dims(self, input_dim, ops._lib.GD_MAX_Q)
        self.ARD = ARD
        self.variance = _positive(variance, (1,))
        self.lengthscale = _positive(lengthscale, (input_dim if ARD else 1,))
        self.period = _positive(period, (input_dim if ARD else 1,))

    def _compute_K(self, F, X, variance, lengthscale, period, X2=None):
        _check_dims(self, X.shape[-1], ops._lib.GD_MAX_Q)
        return _GramDiffFn.apply('periodic', bool(self.ARD), X, X2, variance, lengthscale, period)

    def _compute_Kdiag(self, F, X, variance, lengthscale, period):
        return torch.zeros(X.shape[:-1], dtype=X.dtype, device=X.device) + variance


class RationalQuadratic(NativeKernel):
    """k = variance (1 + r^2 / (2 alpha))^-alpha, r^2 = sum_d tau_d^2 / lengthscale_d^2 (the GPflow / scikit-learn convention)."""

    def __init__(self, input_dim, ARD=False, variance=1., lengthscale=1., alpha=1., name='rq', active_dims=None, dtype=None, ctx=None):
        super(RationalQuadratic, self).__init__(input_dim=input_dim, name=name, active_dims=active_dims, dtype=dtype, ctx=ctx)
        _check_dims(self, input_dim, ops._lib.GD_MAX_Q)
        self.ARD = ARD
        self.variance = _positive(variance, (1,))
        self.lengthscale = _positive(lengthscale, (input_dim if ARD else 1,))
        self.alpha = _positive(alpha, (1,))

    def _compute_K(self, F, X, variance, lengthscale, alpha, X2=None):
        _check_dims(self, X.shape[-1], ops._lib.GD_MAX_Q)
        return _GramDiffFn.apply('rq', bool(self.ARD), X, X2, variance, lengthscale, alpha)

    def _compute_Kdiag(self, F, X, variance, lengthscale, alpha):
        return torch.zeros(X.shape[:-1], dtype=X.dtype, device=X.device) + variance


class SpectralMixture(NativeKernel):
    """k = sum_a weights_a exp(-2 pi^2 sum_d tau_d^2 scales_ad^2) prod_d cos(2 pi tau_d means_ad) (Wilson & Adams 2013): weights (A,), means
    (A, Q) in cycles per unit of input, scales (A, Q).

    Defaults differ between the components, so that a fit does not start at a point where they are interchangeable (and stay so: equal
    components receive equal gradients): weights 1 / A each; means_ad = (a + 1) / (2 A), evenly spaced up to half a cycle per unit of input,
    the Nyquist frequency of unit-spaced data; scales_ad = 1 / (2 pi (a + 1)), i.e. an envelope of lengthscale a + 1."""

    def __init__(self, input_dim, num_mixtures, weights=None, means=None, scales=None, name='sm', active_dims=None, dtype=None, ctx=None):
        super(SpectralMixture, self).__init__(input_dim=input_dim, name=name, active_dims=active_dims, dtype=dtype, ctx=ctx)
        A, Q = int(num_mixtures), int(input_dim)
        _check_dims(self, Q, ops._lib.GD_SM_MAX_Q)
        if not 1 <= A <= ops._lib.GD_SM_MAX_A:
            raise ModelSpecificationError('SpectralMixture takes 1 to %d mixture components; got %d' % (ops._lib.GD_SM_MAX_A, A))
        self.num_mixtures = A
        a = np.arange(1, A + 1, dtype=np.float64)
        self.weights = _positive(np.full(A, 1.0 / A) if weights is None else weights, (A,))
        self.means = _positive(np.repeat((a / (2 * A))[:, None], Q, 1) if means is None else means, (A, Q))
        self.scales = _positive(np.repeat((1.0 / (2 * np.pi * a))[:, None], Q, 1) if scales is None else scales, (A, Q))

    def _compute_K(self, F, X, weights, means, scales, X2=None):
        _check_dims(self, X.shape[-1], ops._lib.GD_SM_MAX_Q)
        return _GramDiffFn.apply('sm', True, X, X2, weights, means, scales)

    def _compute_Kdiag(self, F, X, weights, means, scales):
        total = weights[..., 0]
        for a in range(1, weights.shape[-1]):        # in the order the Gram pass adds the components: the diagonal of K, bit for bit
            total = total + weights[..., a]
        return torch.zeros(X.shape[:-1], dtype=X.dtype, device=X.device) + total[..., None]
