"""Categorical (mxfusion/components/distributions/categorical.py:20-169).

log_prob is (S|1, ..., K) with the random variable's leading dimensions, or (S|1, K) without any: the batch-shared case.  The random
variable is (S|1, ..., 1), class indices (integer tensors are cast to log_prob's dtype), or with one_hot_encoding (S|1, ..., K).  The
leading dimensions are flattened into one batch axis B, and the log-pdf is one autograd function over the row-wise kernels
(mxf_categorical_logpdf / mxf_categorical_logpdf_bwd, simplex.hip): an operand shared over an axis is passed as a broadcast, never copied,
and its gradient comes back summed.  The result is (S, ...) without the class axis, as pick and sum(axis=-1) give it there."""
import torch

from ... import ops
from ._fused import _flatten, carved_grads
from .univariate import UnivariateDistribution


class _CategoricalLogPdfFn(torch.autograd.Function):
    """scale * log p(x[s,b] | logp) (S, B); logp (S|1, B|1, K), x (S|1, B) or, one-hot, (S|1, B, K).  The reverse mode accumulates into one
    zero-filled buffer carved into the gradients that are wanted; a class index has none."""

    @staticmethod
    def forward(ctx, one_hot, normalize, scale, logp, x):
        ctx.one_hot, ctx.normalize, ctx.scale = bool(one_hot), bool(normalize), float(scale)
        ctx.save_for_backward(logp, x)
        return ops.categorical_logpdf(logp, x, one_hot, normalize, scale)

    @staticmethod
    def backward(ctx, g):
        logp, x = ctx.saved_tensors
        grads = carved_grads((logp.shape, x.shape), (ctx.needs_input_grad[3], ctx.needs_input_grad[4] and ctx.one_hot), logp)
        ops.categorical_logpdf_bwd_(logp, x, g.contiguous(), ctx.one_hot, ctx.normalize, ctx.scale, *grads)
        return (None, None, None) + tuple(grads)


class Categorical(UnivariateDistribution):
    def __init__(self, log_prob, num_classes, one_hot_encoding=False, normalization=True, axis=-1, rand_gen=None, dtype=None, ctx=None):
        super(Categorical, self).__init__(inputs=[('log_prob', log_prob)], outputs=None, input_names=['log_prob'],
                                          output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        if axis != -1:
            raise NotImplementedError("The Categorical distribution currently only supports the last dimension to be "
                                      "the class label dimension, i.e., axis == -1.")
        self.axis = axis
        self.normalization = normalization
        self.one_hot_encoding = one_hot_encoding
        self.num_classes = num_classes

    def log_pdf_sum(self, F, variables):
        """sum(mean_S(log_pdf)) (factor_graph.py:223) over the row-wise kernel."""
        return self.log_pdf(F, variables).mean(dim=0).sum()

    def log_pdf_impl(self, log_prob, random_variable, F=None):
        """categorical.py:83-106, multiplied by log_pdf_scaling as there (:102, :105)."""
        K = int(log_prob.shape[-1])
        x = random_variable
        if x.dtype != log_prob.dtype:
            x = x.to(log_prob.dtype)
        lead = tuple(x.shape[1:-1])
        x = _flatten(x, lead, (K,) if self.one_hot_encoding else (1,), full=True)
        if not self.one_hot_encoding:
            x = x.reshape(x.shape[0], x.shape[1])
        out = _CategoricalLogPdfFn.apply(self.one_hot_encoding, self.normalization, float(self.log_pdf_scaling),
                                         _flatten(log_prob, lead, (K,)), x)
        return out.reshape((out.shape[0],) + lead)

    def draw_samples_impl(self, log_prob, rv_shape, num_samples=1, F=None):
        """categorical.py:108-135, drawn from softmax(log_prob) (normalization) or exp(log_prob): the reference hands the
        log-probabilities to a sampler that takes probabilities (:131).  Class indices come back in log_prob's dtype,
        (num_samples,) + rv_shape with its trailing 1; one-hot rows through torch.nn.functional.one_hot."""
        rv_shape = tuple(int(s) for s in rv_shape)
        K = int(self.num_classes)
        prob = torch.softmax(log_prob, dim=-1) if self.normalization else torch.exp(log_prob)
        if prob.dim() < 1 + len(rv_shape):
            prob = prob.reshape((prob.shape[0],) + (1,) * (1 + len(rv_shape) - prob.dim()) + tuple(prob.shape[1:]))
        prob = prob.expand((num_samples,) + rv_shape[:-1] + (K,))
        samples = self._rand_gen.sample_multinomial(prob, dtype=log_prob.dtype, F=F)
        if self.one_hot_encoding:
            samples = torch.nn.functional.one_hot(samples.long(), K).to(log_prob.dtype)
        return samples.reshape((num_samples,) + rv_shape)

    @staticmethod
    def define_variable(log_prob, num_classes, shape=None, one_hot_encoding=False, normalization=True, axis=-1, rand_gen=None, dtype=None,
                        ctx=None):
        cat = Categorical(log_prob=log_prob, num_classes=num_classes, one_hot_encoding=one_hot_encoding, normalization=normalization,
                          axis=axis, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        cat._generate_outputs(shape=shape)
        return cat.random_variable
