"""Beta (mxfusion/components/distributions/beta.py:20-135); log-pdf on mxf_univariate_logpdf*.  As in the reference, `log_pdf_scaling`
is not applied."""
import torch

from .univariate import UnivariateDistribution


class Beta(UnivariateDistribution):
    _kind = 'beta'

    def __init__(self, alpha, beta, rand_gen=None, dtype=None, ctx=None):
        super(Beta, self).__init__(inputs=[('alpha', alpha), ('beta', beta)], outputs=None, input_names=['alpha', 'beta'],
                                   output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def log_pdf_impl(self, alpha, beta, random_variable, F=None):
        """beta.py:46-68."""
        return self._log_pdf(alpha, beta, random_variable)

    def draw_samples_impl(self, alpha, beta, rv_shape, num_samples=1, F=None):
        """beta.py:70-111: X ~ Gamma(alpha, 1), Y ~ Gamma(beta, 1), X / (X + Y); the output shape is the inputs'."""
        if tuple(alpha.shape) != (num_samples,) + tuple(rv_shape):
            raise ValueError("Shape mismatch between inputs {} and random variable {}".format(
                tuple(alpha.shape), (num_samples,) + tuple(rv_shape)))
        ones = torch.ones_like(alpha)
        kw = self._sample_inputs(alpha)
        x = self._rand_gen.sample_gamma(alpha=alpha, beta=ones, shape=(), F=F, **kw)
        y = self._rand_gen.sample_gamma(alpha=beta, beta=ones, shape=(), F=F, **kw)
        return x / (x + y)

    @staticmethod
    def define_variable(alpha=1., beta=1., shape=None, rand_gen=None, dtype=None, ctx=None):
        beta = Beta(alpha=alpha, beta=beta, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        beta._generate_outputs(shape=shape)
        return beta.random_variable
