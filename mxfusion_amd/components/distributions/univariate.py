"""UnivariateDistribution (mxfusion/components/distributions/univariate.py:20-55): the base of the elementwise two-parameter
distributions.  The reference's class is a thin constructor; here it also carries what Gamma, GammaMeanVariance, Beta, Laplace and Uniform
share: the log-pdf as HIP kernels (mxf_univariate_logpdf*, univariate.hip) with fused reverse mode.  A subclass names its kernel (`_kind`)
and whether the reference multiplies its log-pdf by `log_pdf_scaling` (`_scaled`)."""
import torch

from ... import ops
from . import _fused
from ._fused import _carve, carved_grads
from .distribution import Distribution


class _UnivariateLogPdfSumFn(torch.autograd.Function):
    """sum_i mean_s log p(x[s,i] | a[i], b[i]) * scaling -- the quantity FactorGraph.log_pdf adds (models/factor_graph.py:221-224); value
    and gradients in one kernel pass.  a, b: flat, 1 or n elements."""

    @staticmethod
    def forward(ctx, kind, x, a, b, scaling):
        S = x.shape[0]
        need = [ctx.needs_input_grad[i] for i in (1, 2, 3)]
        out, dx, da, db = _carve([1, x.numel() if need[0] else 0, a.numel() if need[1] else 0, b.numel() if need[2] else 0], x)
        if dx is not None:
            dx = dx.view(x.shape)
        ops.univariate_logpdf_(kind, x, a, b, float(scaling) / S, out, dx, da, db)
        ctx.grads = (dx, da, db)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        have = [t for t in ctx.grads if t is not None]
        prod = iter(torch._foreach_mul(have, g) if have else [])          # one multi-tensor launch instead of one per gradient
        return (None,) + tuple(next(prod) if t is not None else None for t in ctx.grads) + (None,)


class _UnivariateLogPdfFn(torch.autograd.Function):
    """scale * log p(x[s,i] | a, b) per element (S, n...); a, b: 1 or n elements, or (S, n...) with a sample axis of their own.  The
    reverse mode is the reduced kernel's gradient logic with the cotangent in the place of its scale (mxf_univariate_logpdf_bwd)."""

    @staticmethod
    def forward(ctx, kind, scale, x, a, b):
        ctx.kind, ctx.scale = kind, float(scale)
        ctx.save_for_backward(x, a, b)
        return ops.univariate_logpdf_elem(kind, x, a, b, scale)

    @staticmethod
    def backward(ctx, g):
        x, a, b = ctx.saved_tensors
        grads = carved_grads((x.shape, a.shape, b.shape), ctx.needs_input_grad[2:5], x)
        ops.univariate_logpdf_bwd_(ctx.kind, x, a, b, g.contiguous(), ctx.scale, *grads)
        return (None, None) + tuple(grads)


class UnivariateDistribution(Distribution):
    _kind = None        # key of ops.D_KIND
    _scaled = False     # whether log_pdf_impl multiplies by log_pdf_scaling (the reference does for Laplace and Uniform only)

    def __init__(self, inputs, input_names, output_names, outputs=None, rand_gen=None, dtype=None, ctx=None):
        inputs = [(n, self._as_variable(v)) for n, v in inputs]
        super(UnivariateDistribution, self).__init__(inputs=inputs, outputs=outputs, input_names=input_names, output_names=output_names,
                                                     rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def _scale(self):
        return float(self.log_pdf_scaling) if self._scaled else 1.0

    @staticmethod
    def _per_element(p, x):
        """a parameter with the sample axis, (1, ...) broadcastable against x (S, ...) -> flat single element or per element; None: sampled"""
        if p.numel() == 1:
            return p.reshape(1)
        if p.shape[0] == 1 and tuple(p.shape[1:]) == tuple(x.shape[1:]):
            return p[0].reshape(-1)
        return None

    def log_pdf_sum(self, F, variables):
        """sum(mean_S(log_pdf)) fused (log_pdf_impl + factor_graph.py:223): the MAP / prior case, parameters without a sample axis."""
        x = variables[self.random_variable.uuid]
        a, b = (variables[v.uuid] for _, v in self.inputs)
        pa, pb = self._per_element(a, x), self._per_element(b, x)
        if pa is None or pb is None:
            return self.log_pdf(F, variables).mean(dim=0).sum()
        return _UnivariateLogPdfSumFn.apply(self._kind, x.contiguous(), pa.contiguous(), pb.contiguous(), self._scale())

    def _log_pdf(self, a, b, random_variable):
        """(S, ...) log-pdf of random_variable (S|1, ...) under a, b (S|1, ...), each broadcastable against it."""
        return _UnivariateLogPdfFn.apply(self._kind, self._scale(), *_fused.spread_operands(random_variable, a, b))

    def _per_sample_operands(self, variables):
        """(a, b, x) as log_pdf_impl receives them"""
        a, b = (variables[v.uuid] for _, v in self.inputs)
        return a, b, variables[self.random_variable.uuid]

    def log_pdf_per_sample(self, F, variables):
        """(S,) sums of log_pdf over every axis but the first in one kernel (mxf_univariate_logpdf_ps), `log_pdf_scaling` where log_pdf_impl
        applies it."""
        if self._kind is None:                # a subclass without a kernel of this family
            return super(UnivariateDistribution, self).log_pdf_per_sample(F, variables)
        a, b, x = self._per_sample_operands(variables)
        S = max(int(x.shape[0]), int(a.shape[0]), int(b.shape[0]))
        if not _fused.per_sample_kernels(S, x.numel() // int(x.shape[0])):
            return super(UnivariateDistribution, self).log_pdf_per_sample(F, variables)
        return _fused.log_pdf_per_sample(self._kind, self._scale(), x, a, b)

    def _sample_inputs(self, p):
        return dict(dtype=p.dtype if isinstance(p, torch.Tensor) else self.dtype, ctx=p.device if isinstance(p, torch.Tensor) else self.ctx)
