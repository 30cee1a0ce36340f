"""Gamma and GammaMeanVariance (mxfusion/components/distributions/gamma.py:20-196); log-pdf on mxf_univariate_logpdf*.  As in the
reference, neither applies `log_pdf_scaling`."""
from .univariate import UnivariateDistribution


class Gamma(UnivariateDistribution):
    _kind = 'gamma'

    def __init__(self, alpha, beta, rand_gen=None, dtype=None, ctx=None):
        super(Gamma, self).__init__(inputs=[('alpha', alpha), ('beta', beta)], outputs=None, input_names=['alpha', 'beta'],
                                    output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def log_pdf_impl(self, alpha, beta, random_variable, F=None):
        """gamma.py:45-59."""
        return self._log_pdf(alpha, beta, random_variable)

    def draw_samples_impl(self, alpha, beta, rv_shape, num_samples=1, F=None):
        """gamma.py:61-74, through the rand_gen seam: one draw per element of (num_samples,) + rv_shape, beta a rate as in log_pdf_impl."""
        out_shape = (num_samples,) + tuple(rv_shape)
        return self._rand_gen.sample_gamma(alpha=alpha.expand(out_shape), beta=beta.expand(out_shape), shape=(),
                                           F=F, **self._sample_inputs(alpha))

    @staticmethod
    def define_variable(alpha=0., beta=1., shape=None, rand_gen=None, dtype=None, ctx=None):
        dist = Gamma(alpha=alpha, beta=beta, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        dist._generate_outputs(shape=shape)
        return dist.random_variable


class GammaMeanVariance(UnivariateDistribution):
    _kind = 'gamma_mv'

    def __init__(self, mean, variance, rand_gen=None, dtype=None, ctx=None):
        super(GammaMeanVariance, self).__init__(inputs=[('mean', mean), ('variance', variance)], outputs=None,
                                                input_names=['mean', 'variance'], output_names=['random_variable'],
                                                rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def _get_alpha_beta(self, a, b):
        """gamma.py:127-138."""
        beta = a / b
        alpha = a * beta
        return alpha, beta

    def log_pdf_impl(self, mean, variance, random_variable, F=None):
        """gamma.py:140-159; the change of parameters and its chain rule run inside the kernel."""
        return self._log_pdf(mean, variance, random_variable)

    def draw_samples_impl(self, mean, variance, rv_shape, num_samples=1, F=None):
        """gamma.py:161-175."""
        out_shape = (num_samples,) + tuple(rv_shape)
        alpha, beta = self._get_alpha_beta(mean, variance)
        return self._rand_gen.sample_gamma(alpha=alpha.expand(out_shape), beta=beta.expand(out_shape), shape=(),
                                           F=F, **self._sample_inputs(mean))

    @staticmethod
    def define_variable(mean=0., variance=1., shape=None, rand_gen=None, dtype=None, ctx=None):
        dist = GammaMeanVariance(mean=mean, variance=variance, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        dist._generate_outputs(shape=shape)
        return dist.random_variable
