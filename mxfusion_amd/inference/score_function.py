"""ScoreFunctionInference / ScoreFunctionRBInference (mxfusion/inference/score_function.py:24-194): black-box variational inference
(Ranganath, Gerrish, Blei 2014) -- the stochastic algorithm for latent variables whose draws cannot be reparameterised (Bernoulli,
Categorical).

This is the estimator of the paper, NOT the reference's expression.  The reference multiplies two values that are sample means already,
mean_0(q_bar * stop(p_bar - q_bar)) over one element (score_function.py:70-77: FactorGraph.log_pdf returns the scalar sum(mean_S(.)),
factor_graph.py:223), which is not the mean over the samples of log q(z_s) * (log p(x, z_s) - log q(z_s)); it marks the class "still in
development" and tests it with atol=1.  Here every sample keeps its own weight: FactorGraph.log_pdf_per_sample returns the (S,) vectors
on the per-sample HIP reductions (mxf_normal_logpdf_ps*, mxf_univariate_logpdf_ps*), whose reverse mode takes the weights.

With z_s ~ q, s < S, DETACHED (the estimator must not also carry the pathwise term; discrete draws have none),
p_s = log p(x, z_s), q_s = log q(z_s), f_s = p_s - q_s:
    loss              = -mean_s f_s                                   (the number StochasticVariationalInference returns for the same noise)
    loss_for_gradient = -[ mean_s(q_s * stop(f_s - b_s)) + mean_s(p_s - stop(q_s)) ]
The first term differentiates to the score-function gradient of the posterior parameters, the second to the gradient of the model
parameters.  baseline=None: b_s = 0, Algorithm 1 of the paper.  baseline='loo': b_s = (sum_t f_t - f_s) / (S - 1), the mean of the OTHER
samples -- independent of z_s, hence unbiased; needs S >= 2."""
import torch

from ..common.exceptions import InferenceError
from ..components.variables.variable import VariableType
from .variational import StochasticVariationalInference


def _per_sample(v, S):
    """a (S,) vector of a graph's per-sample log-density; (1,) -- nothing in it carries samples -- is broadcast"""
    return v.expand(S) if v.shape[0] != S else v


class ScoreFunctionInference(StochasticVariationalInference):
    """score_function.py:24-81.  No Rao-Blackwellisation: works for posteriors that are not mean-field."""

    def __init__(self, num_samples, model, posterior, observed, baseline=None):
        super(ScoreFunctionInference, self).__init__(num_samples=num_samples, model=model, posterior=posterior, observed=observed)
        if baseline not in (None, 'loo'):
            raise InferenceError("baseline must be None or 'loo', not %r" % (baseline,))
        if baseline == 'loo' and int(num_samples) < 2:
            raise InferenceError("baseline='loo' is the mean over the other samples: it needs num_samples >= 2")
        self.baseline = baseline

    def _draw(self, F, variables):
        samples = self.posterior.draw_samples(F=F, variables=variables, num_samples=self.num_samples)
        variables.update({k: v.detach() for k, v in samples.items()})

    def _centred(self, f):
        """stop(f_s - b_s)"""
        f = f.detach()
        if self.baseline is None:
            return f
        S = f.shape[0]
        return f - (f.sum() - f) / (S - 1)

    def _posterior_term(self, F, variables, p, q):
        """mean_s(q_s * stop(f_s - b_s))"""
        return (q * self._centred(p - q)).mean()

    def compute(self, F, variables):
        S = int(self.num_samples)
        self._draw(F, variables)
        p = _per_sample(self.model.log_pdf_per_sample(F=F, variables=variables), S)
        q = _per_sample(self.posterior.log_pdf_per_sample(F=F, variables=variables), S)
        for_gradient = self._posterior_term(F, variables, p, q) + (p - q.detach()).mean()
        return -(p - q).mean().detach(), -for_gradient


class ScoreFunctionRBInference(ScoreFunctionInference):
    """score_function.py:84-194: Rao-Blackwellised (section 3.1 of the paper).  For every latent variable v_i of the posterior the weight of
    its score is f_i = p_i - q_i, with q_i the log-density of the posterior factor that generates v_i and p_i the model's log-density over
    v_i and every random variable that descends from it in the model graph: the factors that do not involve v_i have a zero-mean product
    with its score and only add variance.  Requires a mean-field posterior (checked at construction)."""

    def __init__(self, num_samples, model, posterior, observed, baseline=None):
        super(ScoreFunctionRBInference, self).__init__(num_samples=num_samples, model=model, posterior=posterior, observed=observed,
                                                       baseline=baseline)
        self._latent = list(posterior.get_latent_variables(self.observed_variable_UUIDs))
        latent = {v.uuid for v in self._latent}
        for v in self._latent:
            todo, seen = [u for _, u in v.factor.inputs], set()
            while todo:                                   # the factor's inputs, through the functions that produce them
                u = todo.pop()
                if id(u) in seen:
                    continue
                seen.add(id(u))
                if u.uuid in latent:
                    raise InferenceError('ScoreFunctionRBInference needs a mean-field posterior: the factor of %s has the latent variable %s '
                                         'among its inputs' % (v, u))
                if u.type == VariableType.FUNCVAR:
                    todo.extend(w for _, w in u.factor.inputs)
        self._model_targets = {}
        for v in self._latent:
            self._model_targets[v.uuid] = [d.uuid for d in model.get_descendants(model[v]) if d.type == VariableType.RANDVAR]

    def _posterior_term(self, F, variables, p, q):
        """sum_i mean_s(q_{i,s} * stop(p_{i,s} - q_{i,s} - b_{i,s}))"""
        S = int(self.num_samples)
        total = 0.
        for v in self._latent:
            q_i = _per_sample(self.posterior.log_pdf_per_sample(F=F, variables=variables, targets=[v.uuid]), S)
            with torch.no_grad():                         # p_i only weights the score
                p_i = _per_sample(self.model.log_pdf_per_sample(F=F, variables=variables, targets=self._model_targets[v.uuid]), S)
            total = total + (q_i * self._centred(p_i - q_i)).mean()
        return total
