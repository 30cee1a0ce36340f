"""Laplace (mxfusion/components/distributions/laplace.py:23-99); log-pdf on mxf_univariate_logpdf*, times `log_pdf_scaling` as in the
reference."""
from .univariate import UnivariateDistribution


class Laplace(UnivariateDistribution):
    _kind = 'laplace'
    _scaled = True

    def __init__(self, location, scale, rand_gen=None, dtype=None, ctx=None):
        super(Laplace, self).__init__(inputs=[('location', location), ('scale', scale)], outputs=None, input_names=['location', 'scale'],
                                      output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def log_pdf_impl(self, location, scale, random_variable, F=None):
        """laplace.py:37-55."""
        return self._log_pdf(location, scale, random_variable)

    def draw_samples_impl(self, location, scale, rv_shape, num_samples=1, F=None):
        """laplace.py:57-77: location + scale * standard Laplace noise."""
        out_shape = (num_samples,) + tuple(rv_shape)
        return self._rand_gen.sample_laplace(shape=out_shape, F=F, **self._sample_inputs(location)) * scale + location

    @staticmethod
    def define_variable(location=0., scale=1., shape=None, rand_gen=None, dtype=None, ctx=None):
        var = Laplace(location=location, scale=scale, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        var._generate_outputs(shape=shape)
        return var.random_variable
