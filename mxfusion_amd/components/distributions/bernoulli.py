"""Bernoulli (mxfusion/components/distributions/bernoulli.py:20-119); log-pdf on mxf_univariate_logpdf* (kind 'bernoulli'), times
`log_pdf_scaling` as in the reference (:77).  The kernels' second parameter slot is unused: prob_true is passed again, detached, and its
zero gradient is dropped."""
from .univariate import UnivariateDistribution, _UnivariateLogPdfSumFn


class Bernoulli(UnivariateDistribution):
    _kind = 'bernoulli'
    _scaled = True

    def __init__(self, prob_true, rand_gen=None, dtype=None, ctx=None):
        super(Bernoulli, self).__init__(inputs=[('prob_true', prob_true)], outputs=None, input_names=['prob_true'],
                                        output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    @staticmethod
    def _observed(random_variable, prob_true):
        """boolean and integer observations in the parameter's dtype"""
        return random_variable if random_variable.dtype == prob_true.dtype else random_variable.to(prob_true.dtype)

    def log_pdf_sum(self, F, variables):
        """sum(mean_S(log_pdf)) fused, as UnivariateDistribution.log_pdf_sum with the one parameter in both slots."""
        p = variables[self.inputs[0][1].uuid]
        x = self._observed(variables[self.random_variable.uuid], p)
        pa = self._per_element(p, x)
        if pa is None:
            return self.log_pdf(F, variables).mean(dim=0).sum()
        pa = pa.contiguous()
        return _UnivariateLogPdfSumFn.apply(self._kind, x.contiguous(), pa, pa.detach(), self._scale())

    def _per_sample_operands(self, variables):
        p = variables[self.inputs[0][1].uuid]
        return p, p.detach(), self._observed(variables[self.random_variable.uuid], p)

    def log_pdf_impl(self, prob_true, random_variable, F=None):
        """bernoulli.py:62-78."""
        return self._log_pdf(prob_true, prob_true.detach(), self._observed(random_variable, prob_true))

    def draw_samples_impl(self, prob_true, rv_shape, num_samples=1, F=None):
        """bernoulli.py:80-96."""
        return self._rand_gen.sample_bernoulli(prob_true, shape=(num_samples,) + tuple(rv_shape), dtype=prob_true.dtype, F=F)

    @staticmethod
    def define_variable(prob_true, shape=None, rand_gen=None, dtype=None, ctx=None):
        bernoulli = Bernoulli(prob_true=prob_true, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        bernoulli._generate_outputs(shape=shape)
        return bernoulli.random_variable
