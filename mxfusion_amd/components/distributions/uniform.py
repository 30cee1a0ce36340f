"""Uniform on [low, high) (mxfusion/components/distributions/uniform.py:24-107); log-pdf on mxf_univariate_logpdf*, times
`log_pdf_scaling` as in the reference."""
from .univariate import UnivariateDistribution


class Uniform(UnivariateDistribution):
    _kind = 'uniform'
    _scaled = True

    def __init__(self, low, high, rand_gen=None, dtype=None, ctx=None):
        super(Uniform, self).__init__(inputs=[('low', low), ('high', high)], outputs=None, input_names=['low', 'high'],
                                      output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def log_pdf_impl(self, low, high, random_variable, F=None):
        """uniform.py:38-62: -log(high - low) on low <= x < high, -inf elsewhere."""
        return self._log_pdf(low, high, random_variable)

    def draw_samples_impl(self, low, high, rv_shape, num_samples=1, F=None):
        """uniform.py:64-84."""
        out_shape = (num_samples,) + tuple(rv_shape)
        return self._rand_gen.sample_uniform(low=low, high=high, shape=out_shape, F=F, **self._sample_inputs(low))

    @staticmethod
    def define_variable(low=0, high=1, shape=None, rand_gen=None, dtype=None, ctx=None):
        var = Uniform(low=low, high=high, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        var._generate_outputs(shape=shape)
        return var.random_variable
