"""Dirichlet (mxfusion/components/distributions/dirichlet.py:21-134).

The random variable is (S|1, ..., K) and alpha (S|1, ..., K) broadcastable against its leading dimensions, which are flattened into one
batch axis B; the class axis is the last one (the reference hard-codes axis 2, the same for its (S, B, K) case).  The log-pdf is one
autograd function over the row-wise kernels (mxf_dirichlet_logpdf / mxf_dirichlet_logpdf_bwd, simplex.hip): an operand shared over an axis
is passed as a broadcast, never copied, and its gradient comes back summed.  As in the reference, `log_pdf_scaling` is not applied
(dirichlet.py:64)."""
import torch

from ... import ops
from .distribution import Distribution
from ._fused import _flatten, carved_grads


class _DirichletLogPdfFn(torch.autograd.Function):
    """log Dir(x[s,b] | alpha) (S, B); x (S|1, B, K), alpha (S|1, B|1, K).  The reverse mode accumulates into one zero-filled buffer carved
    into the gradients that are wanted."""

    @staticmethod
    def forward(ctx, normalize, x, alpha):
        ctx.normalize = bool(normalize)
        ctx.save_for_backward(x, alpha)
        return ops.dirichlet_logpdf(x, alpha, normalize)

    @staticmethod
    def backward(ctx, g):
        x, alpha = ctx.saved_tensors
        grads = carved_grads((x.shape, alpha.shape), ctx.needs_input_grad[1:3], x)
        ops.dirichlet_logpdf_bwd_(x, alpha, g.contiguous(), ctx.normalize, 1.0, *grads)
        return (None,) + tuple(grads)


class Dirichlet(Distribution):
    def __init__(self, alpha, normalization=True, rand_gen=None, dtype=None, ctx=None):
        super(Dirichlet, self).__init__(inputs=[('alpha', self._as_variable(alpha))], outputs=None, input_names=['alpha'],
                                        output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        self.normalization = normalization

    def log_pdf_impl(self, alpha, random_variable, F=None):
        """dirichlet.py:43-65, with lgamma where the reference takes the log of a quotient of gamma products."""
        K = int(random_variable.shape[-1])
        lead = tuple(torch.broadcast_shapes(tuple(random_variable.shape[1:-1]), tuple(alpha.shape[1:-1])))
        out = _DirichletLogPdfFn.apply(self.normalization, _flatten(random_variable, lead, (K,), full=True), _flatten(alpha, lead, (K,)))
        return out.reshape((out.shape[0],) + lead)

    def draw_samples_impl(self, alpha, rv_shape, num_samples=1, F=None):
        """dirichlet.py:67-85: Gamma(alpha, 1) draws divided by their sum along the class axis (the reference divides by the sum over the
        whole array, :85).  alpha without a sample axis is expanded to (num_samples,) + rv_shape first."""
        full = (num_samples,) + tuple(int(s) for s in rv_shape)
        alpha = alpha.expand(full)
        y = self._rand_gen.sample_gamma(alpha=alpha, beta=torch.ones_like(alpha), shape=(), dtype=alpha.dtype, ctx=alpha.device, F=F)
        return y / y.sum(dim=-1, keepdim=True)

    @staticmethod
    def define_variable(alpha, shape=None, normalization=True, rand_gen=None, dtype=None, ctx=None):
        dirichlet = Dirichlet(alpha=alpha, normalization=normalization, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        dirichlet._generate_outputs(shape=shape)
        return dirichlet.random_variable
