"""Wishart (mxfusion/components/distributions/wishart.py:24-182).

The random variable and the scale are (S|1, ..., n, n); the degrees of freedom are (S|1,), one value per sample as in the reference, or
(S|1, ...) broadcastable against the leading dimensions, which are flattened into one batch axis B.  Up to order 32 the log-pdf is one
autograd function over the fused small-matrix kernels (mxf_wishart_logpdf / mxf_wishart_logpdf_bwd, wishart.hip): an operand shared over
an axis is passed as a broadcast, never copied, and its gradient comes back summed.  Larger orders take the blocked dense calls
(mxf_potrf / mxf_trsm / mxf_coldot / mxf_sumlogdiag through gp/_linalg.py), the matrices flattened onto the sample axis those calls batch
over.  Draws are the Bartlett decomposition (L A)(L A)^T, vectorised, through the rand_gen seam, differentiable in the scale."""
import math

import torch

from ... import ops
from ...common import config
from .distribution import Distribution
from .gp._linalg import chol, coldot, gemm, trsm
from ._fused import _flatten, _numel, carved_grads, replicate


class _WishartLogPdfFn(torch.autograd.Function):
    """scale * log W(X[s,b] | V, nu) (S, B) for n <= 32 and the info words; X (S|1, B, n, n), nu (S|1, B|1), V (S|1, B|1, n, n).  The
    reverse mode accumulates into one zero-filled buffer carved into the gradients that are wanted."""

    @staticmethod
    def forward(ctx, scale, X, nu, V):
        out, info = ops.wishart_logpdf(X, nu, V, scale)
        ctx.scale = float(scale)
        ctx.save_for_backward(X, nu, V)
        ctx.mark_non_differentiable(info)
        return out, info

    @staticmethod
    def backward(ctx, g, _):
        X, nu, V = ctx.saved_tensors
        grads = carved_grads((X.shape, nu.shape, V.shape), ctx.needs_input_grad[1:4], X)
        ops.wishart_logpdf_bwd_(X, nu, V, g.contiguous(), ctx.scale, *grads)
        return (None,) + tuple(grads)


class _SumLogDiagFn(torch.autograd.Function):
    """sum_i log L_ii (M,) of lower factors L (M, n, n) through mxf_sumlogdiag; dL = g / L_ii on the diagonal."""

    @staticmethod
    def forward(ctx, L):
        ctx.save_for_backward(L)
        return ops.sumlogdiag(L)

    @staticmethod
    def backward(ctx, g):
        L, = ctx.saved_tensors
        return torch.diag_embed(g.reshape(-1, 1) / torch.diagonal(L, dim1=-2, dim2=-1))


def _dense_log_pdf(X, nu, V):
    """The log-pdf (S, B) and the info words (the fused kernels' convention) for any order on the blocked dense calls (wishart.py:83-96):
    one factor of V when it is shared by every row, otherwise one per row on the sample axis."""
    S, B, n = max(X.shape[0], nu.shape[0], V.shape[0]), X.shape[1], X.shape[-1]
    Lx, info_x = chol(X.expand(S, B, n, n).reshape(S * B, n, n))
    Lv, info_v = chol(V.reshape(1, n, n) if V.shape[0] == 1 and V.shape[1] == 1 else V.expand(S, B, n, n).reshape(S * B, n, n))
    Y = trsm(Lv, Lx)                                                                    # tr(V^-1 X) = |L_V^-1 L_X|_F^2
    tr = coldot(Y, Y).sum(-1)
    logdet_x, logdet_v = 2.0 * _SumLogDiagFn.apply(Lx), 2.0 * _SumLogDiagFn.apply(Lv)
    nu = nu.expand(S, B).reshape(S * B)
    low = ~(nu > n - 1)                                                                 # mvlgamma refuses such an argument
    nu = torch.where(low, torch.full_like(nu, float(n)), nu)
    out = 0.5 * ((nu - n - 1) * logdet_x - tr - nu * (n * math.log(2.0)) - nu * logdet_v) - torch.mvlgamma(0.5 * nu, n)
    info_x, info_v = info_x.reshape(-1), info_v.reshape(-1).expand(S * B)
    info = torch.where(info_v > 0, info_v, torch.where(info_x > 0, info_x + n, low.to(info_x.dtype) * (2 * n + 1)))
    out = torch.where(info != 0, torch.full_like(out, float('nan')), out)               # a failed row is NaN, as from the fused kernel
    return out.reshape(S, B), info.reshape(S, B)


class Wishart(Distribution):
    def __init__(self, degrees_of_freedom, scale, rand_gen=None, dtype=None, ctx=None):
        inputs = [('degrees_of_freedom', self._as_variable(degrees_of_freedom)), ('scale', self._as_variable(scale))]
        super(Wishart, self).__init__(inputs=inputs, outputs=None, input_names=['degrees_of_freedom', 'scale'],
                                      output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def replicate_self(self, attribute_map=None):
        """wishart.py:49-60"""
        return replicate(self)

    def _dof(self, degrees_of_freedom, like):
        """the degrees of freedom as a floating tensor with a sample axis; an integer one is cast to the distribution's dtype (wishart.py:82)"""
        nu = torch.as_tensor(degrees_of_freedom, device=like.device)
        if not nu.is_floating_point():
            nu = nu.to(self.torch_dtype() if self.dtype is not None else like.dtype)
        return nu.reshape(1) if nu.dim() == 0 else nu

    def log_pdf_impl(self, degrees_of_freedom, scale, random_variable, F=None):
        """wishart.py:62-96, multiplied by log_pdf_scaling as there."""
        n = int(scale.shape[-1])
        nu = self._dof(degrees_of_freedom, scale)
        lead = tuple(torch.broadcast_shapes(tuple(random_variable.shape[1:-2]), tuple(scale.shape[1:-2]), tuple(nu.shape[1:])))
        X = _flatten(random_variable, lead, (n, n), full=True)
        V, nu = _flatten(scale, lead, (n, n)), _flatten(nu, lead, ())
        if n <= ops.MVN_MAX_ORDER:
            out, info = _WishartLogPdfFn.apply(float(self.log_pdf_scaling), X, nu, V)
        else:
            out, info = _dense_log_pdf(X, nu, V)
            out = out * self.log_pdf_scaling
        self._last_info = info
        return out.reshape((out.shape[0],) + lead)

    def draw_samples_impl(self, degrees_of_freedom, scale, rv_shape, num_samples=1, F=None):
        """wishart.py:98-147, the Bartlett decomposition X = (L A)(L A)^T with V = L L^T and A lower triangular.  Two draws, in this order:
        first eps = sample_normal(shape=(num_samples,) + rv_shape), whose strict lower triangle gives A's off-diagonal entries; then
        c = sample_gamma(alpha=(nu - j) / 2 for the diagonal index j = 0..n-1, expanded to (num_samples,) + rv_shape[:-1], beta=1/2,
        shape=()), a chi-squared draw of nu - j degrees of freedom, whose square root is A's diagonal.  nu need not be an integer."""
        rv_shape = tuple(int(s) for s in rv_shape)
        n, lead = rv_shape[-1], rv_shape[:-2]
        full = (num_samples,) + lead
        nu = _flatten(self._dof(degrees_of_freedom, scale), lead, ()).to(scale.dtype)
        eps = self._rand_gen.sample_normal(shape=(num_samples,) + rv_shape, dtype=scale.dtype, ctx=scale.device)
        alpha = 0.5 * (nu.reshape((nu.shape[0],) + (lead if nu.shape[1] > 1 else (1,) * len(lead)) + (1,))
                       - torch.arange(n, dtype=scale.dtype, device=scale.device))
        c = self._rand_gen.sample_gamma(alpha=alpha.expand(full + (n,)), beta=0.5, shape=(), dtype=scale.dtype, ctx=scale.device)
        A = (torch.tril(eps, -1) + torch.diag_embed(torch.sqrt(c))).reshape(_numel(full), n, n)
        Vf = _flatten(scale, lead, (n, n))
        L, info = chol(Vf.reshape(-1, n, n))
        self._last_info = info
        if Vf.shape[0] * Vf.shape[1] > 1:
            L = L.reshape(tuple(Vf.shape)).expand(full[0], _numel(lead), n, n).reshape(_numel(full), n, n)
        LA = gemm(L, A)
        return gemm(LA, LA, transB=True).reshape((num_samples,) + rv_shape)

    @staticmethod
    def define_variable(shape, degrees_of_freedom=0, scale=None, rand_gen=None, minibatch_ratio=1., dtype=None, ctx=None):
        """wishart.py:149-173: the default scale is the identity of order shape[-1]; minibatch_ratio is accepted and unused, as there."""
        if scale is None:
            scale = torch.eye(int(shape[-1]), dtype=config.torch_dtype(dtype))
        dist = Wishart(degrees_of_freedom=degrees_of_freedom, scale=scale, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        dist._generate_outputs(shape=shape)
        return dist.random_variable
