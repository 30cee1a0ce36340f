"""SVGPLikelihood: the sparse variational GP of svgp_regression.py under a non-Gaussian likelihood (likelihoods.py) -- GP classification
and Poisson regression on the Gram, Cholesky, solve and product kernels of the regression module.  No reference counterpart.

  ELBO = c sum_{n,p} E_{N(f; m[n,p], v[n])}[log p(y[n,p] | f)] - KL(q(u) || p(u))        (Hensman, Matthews, Ghahramani 2015)

  SVGPLikelihoodLogPdf.compute     -> kern.K + the differentiable mxf_potrf / mxf_trsm / mxf_gemm / mxf_coldot bridges (gp/_linalg.py) for the
                                      marginals of q(f) and the KL term, mxf_lik_expect for the data term and its reverse mode
  SVGPLikelihoodPrediction.compute -> the same marginals at the test inputs, mxf_lik_moments for E[y], Var[y]
"""
from types import SimpleNamespace

import numpy as np
import torch

from ... import ops
from ...common.exceptions import ModelSpecificationError
from ...components.variables.variable import Variable
from ...components.variables.var_trans import PositiveTransformation
from ...components.distributions.gp import _linalg as lin
from ...inference.inference_alg import SamplingAlgorithm
from ...inference.variational import VariationalInference
from ..module import Module, ModuleGraph
from .likelihoods import Likelihood


def _over(t, S):
    """t with its shared sample axis expanded to S (mxf_trsm solves in place: its right-hand side carries every sample)"""
    return t.expand((S,) + tuple(t.shape[1:])) if t.shape[0] == 1 and S > 1 else t


def _sumsq(t):
    return (t * t).reshape(t.shape[0], -1).sum(-1)


def _logdiag(L):
    return torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)


def q_f_marginals(F, kern, kern_params, X, Z, mu, S_W, S_diag, jitter, mean=None):
    """Mean m (S, N, P) and variance v (S, N) of q(f) at the rows of X, and what the KL term needs of the factors:
         L = chol(Kuu + jitter I),  A = L^-1 Kuf,  m = A^T L^-1 mu (+ mean),
         v = kdiag - coldot(A, A) + coldot(L^-1 S L^-T A, A),  S = W W^T + diag(d) = Ls Ls^T
    the last term as coldot(D, D) with D = (L^-1 Ls)^T A, a sum of squares.  Every operand may carry a sample axis; gradients reach all
    of them through the reverse modes of gp/_linalg.py."""
    M = Z.shape[-2]
    Kuu = kern.K(F, Z, **kern_params)
    if jitter > 0.:
        Kuu = Kuu + torch.eye(M, dtype=Z.dtype, device=Z.device) * jitter
    L, info = lin.chol(Kuu)
    Ls, info_s = lin.chol(lin.gemm(S_W, S_W, transB=True) + torch.diag_embed(S_diag))
    Kuf = kern.K(F, Z, X, **kern_params)
    S = max(t.shape[0] for t in (L, Ls, Kuf, mu))
    A = lin.trsm(L, _over(Kuf, S))
    Lmu = lin.trsm(L, _over(mu, S))
    C = lin.trsm(L, _over(Ls, S))
    m = lin.gemm(A, Lmu, transA=True)
    if mean is not None:
        m = m + mean
    D = lin.gemm(C, A, transA=True)
    v = kern.Kdiag(F, X, **kern_params) - lin.coldot(A, A) + lin.coldot(D, D)
    return m, v, SimpleNamespace(L=L, Ls=Ls, Lmu=Lmu, C=C, info=ops.merge_info(info, info_s))


class SVGPLikelihoodLogPdf(VariationalInference):
    """The bound above for the rows handed in.  `log_pdf_scaling` multiplies the data term only and `kl_weight` the KL term, as in
    SVGPRegressionLogPdf, so the minibatch and the row-sharded loops work unchanged."""

    kl_weight = 1.0

    def __init__(self, model, posterior, observed, jitter=0.):
        super(SVGPLikelihoodLogPdf, self).__init__(model=model, posterior=posterior, observed=observed)
        self.log_pdf_scaling = 1
        self.jitter = jitter

    def compute(self, F, variables):
        """c * (data term over the rows handed in) + kl_weight * (-KL): with kl_weight = w evaluated as w * (c / w * data - KL)"""
        w = float(self.kl_weight)
        g = self.model
        X, Y, Z = variables[g.X], variables[g.Y], variables[g.inducing_inputs]
        mu, S_W, S_diag = variables[self.posterior.qU_mean], variables[self.posterior.qU_cov_W], variables[self.posterior.qU_cov_diag]
        kern_params = g.kernel.fetch_parameters(variables)
        mean = variables[g.mean] if g.F.factor.has_mean else None
        ops._require_gpu(X)
        # a float32 model is evaluated in float64 inside (inputs widened, result narrowed), as SVGPRegressionLogPdf._compute_materialised and
        # every prediction do: the (M x M) factorisations lose cond(Kuu) 2^-24 in float32
        narrow = X.dtype == torch.float32
        if narrow:
            X, Y, Z, mu, S_W, S_diag = [t.double() for t in (X, Y, Z, mu, S_W, S_diag)]
            kern_params = {k: t.double() for k, t in kern_params.items()}
            mean = None if mean is None else mean.double()
        m, v, q = q_f_marginals(F, g.kernel, kern_params, X, Z, mu, S_W, S_diag, float(self.jitter), mean)
        self._last_info = q.info
        M, P = Z.shape[-2], mu.shape[-1]
        kl = 0.5 * (P * _sumsq(q.C) + _sumsq(q.Lmu) - P * M + 2.0 * P * (_logdiag(q.L) - _logdiag(q.Ls)))
        data = g.likelihood.expected_log_pdf_sum(Y, m, v, scale=float(self.log_pdf_scaling) / w)
        out = w * (data - kl)
        return out.float() if narrow else out


class SVGPLikelihoodPrediction(SamplingAlgorithm):
    """latent=True: mean (S, N, P) and variance (S, N, 1) of q(f) at the test inputs; otherwise (E[y], Var[y]), each (S, N, P), through the
    likelihood's inverse link (mxf_lik_moments)."""

    def __init__(self, model, posterior, observed, latent=False, jitter=0.):
        super(SVGPLikelihoodPrediction, self).__init__(model=model, observed=observed, extra_graphs=[posterior])
        self.latent = latent
        self.jitter = jitter

    def compute(self, F, variables):
        g, post = self.model, self.graphs[1]
        X, Z = variables[g.X], variables[g.inducing_inputs]
        mu, S_W, S_diag = variables[post.qU_mean], variables[post.qU_cov_W], variables[post.qU_cov_diag]
        kern_params = g.kernel.fetch_parameters(variables)
        mean = variables[g.mean] if g.F.factor.has_mean else None
        ops._require_gpu(X)
        narrow = X.dtype == torch.float32
        if narrow:
            X, Z, mu, S_W, S_diag = [t.double() for t in (X, Z, mu, S_W, S_diag)]
            kern_params = {k: t.double() for k, t in kern_params.items()}
            mean = None if mean is None else mean.double()
        with torch.no_grad():
            m, v, q = q_f_marginals(F, g.kernel, kern_params, X, Z, mu, S_W, S_diag, float(self.jitter), mean)
            self._last_info = q.info
            res = (m, v.unsqueeze(-1)) if self.latent else g.likelihood.predictive_moments(m, v)
        if narrow:
            res = tuple(t.float() for t in res)
        outcomes = {g.Y.uuid: res}
        if self.target_variables:
            return tuple(outcomes[t] for t in self.target_variables)
        return outcomes


class SVGPLikelihood(Module):
    """y[n, p] ~ likelihood(f_p(x_n)), f_p ~ GP(mean, kernel) through M inducing points with q(u_p) = N(qU_mean[:, p], W W^T + diag(d)).  A
    likelihood with `num_latent` set (RobustMax) has that many latent functions over one label column: y[n, 0] ~ likelihood(f_1..C(x_n))."""

    row_additive = True      # the bound is a sum over data rows plus -KL(q(u) || p(u)): row shards add up

    def __init__(self, X, kernel, likelihood, inducing_inputs=None, num_inducing=10, mean=None, rand_gen=None, dtype=None, ctx=None):
        if not isinstance(likelihood, Likelihood):
            raise TypeError('SVGPLikelihood: likelihood must be a BernoulliLogit, BernoulliProbit, PoissonExp or RobustMax, got %r' % (likelihood,))
        if not isinstance(X, Variable):
            X = Variable(value=X)
        if inducing_inputs is None:
            inducing_inputs = Variable(shape=(num_inducing, kernel.input_dim), initial_value=np.random.randn(num_inducing, kernel.input_dim))
        inputs = [('X', X), ('inducing_inputs', inducing_inputs)]
        if mean is not None:
            inputs.append(('mean', mean))
        self._has_mean = mean is not None
        object.__setattr__(self, 'kernel', kernel)
        object.__setattr__(self, 'likelihood', likelihood)
        super(SVGPLikelihood, self).__init__(inputs=inputs, outputs=None, input_names=[k for k, _ in inputs],
                                             output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def _generate_outputs(self, output_shapes=None):
        shape = output_shapes['random_variable']
        Y_shape = tuple(self.X.shape[:-1]) + (1,) if shape is None else shape
        self.set_outputs([Variable(shape=Y_shape)])

    def _build_module_graphs(self):
        Y = self.random_variable
        graph = ModuleGraph(name='svgp_likelihood')
        graph.X = self.X
        graph.inducing_inputs = self.inducing_inputs
        M = self.inducing_inputs.shape[0]
        if self._has_mean:
            graph.mean = self.mean
        graph.F = SimpleNamespace(factor=SimpleNamespace(has_mean=self._has_mean, dtype=self.dtype, kernel=self.kernel))
        graph.Y = Y
        graph.kernel = self.kernel
        graph.likelihood = self.likelihood
        for n, v in self.kernel.parameters.items():
            setattr(graph, n, v)
        post = ModuleGraph(name='svgp_posterior')
        post.qU_cov_diag = Variable(shape=(M,), transformation=PositiveTransformation())
        post.qU_cov_W = Variable(shape=(M, M))
        if self.likelihood.num_latent is not None and Y.shape[-1] != 1:
            raise ModelSpecificationError('SVGPLikelihood: %s takes its labels in one column, so the last axis of the output shape must be 1; '
                                          'got %s' % (type(self.likelihood).__name__, tuple(Y.shape)))
        post.qU_mean = Variable(shape=(M, self.likelihood.num_latent or Y.shape[-1]))
        return graph, [post]

    def _attach_default_inference_algorithms(self):
        observed = [v for _, v in self.inputs] + [v for _, v in self.outputs]
        self.attach_log_pdf_algorithms(targets=self.output_names, conditionals=self.input_names,
                                       algorithm=SVGPLikelihoodLogPdf(self._module_graph, self._extra_graphs[0], observed),
                                       alg_name='svgp_log_pdf')
        observed = [v for _, v in self.inputs]
        self.attach_prediction_algorithms(targets=self.output_names, conditionals=self.input_names,
                                          algorithm=SVGPLikelihoodPrediction(self._module_graph, self._extra_graphs[0], observed),
                                          alg_name='svgp_predict')

    @staticmethod
    def define_variable(X, kernel, likelihood, shape=None, inducing_inputs=None, num_inducing=10, mean=None, rand_gen=None, dtype=None,
                        ctx=None):
        gp = SVGPLikelihood(X=X, kernel=kernel, likelihood=likelihood, inducing_inputs=inducing_inputs, num_inducing=num_inducing,
                            mean=mean, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        gp._generate_outputs({'random_variable': shape})
        return gp.random_variable

    @property
    def random_variable(self):
        return self._outputs[0][1]
