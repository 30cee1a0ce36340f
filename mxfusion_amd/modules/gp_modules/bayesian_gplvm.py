"""BayesianGPLVM: the sparse GP of sparsegp_regression.py whose inputs are uncertain, x_n ~ q(x_n) = N(X_mean[n], diag(X_var[n])) -- the
Bayesian GP latent variable model when q(X) is learnt, GP regression with noisy inputs when X_var is observed.  No reference counterpart:
the reference averages the bound over draws of X.

The collapsed bound of Titsias & Lawrence (2010) is the bound of SparseGPRegressionLogPdf._compute_materialised with the kernel matrices
replaced by their expectations under q(X), the psi statistics (closed form for the RBF kernel: RBF.psi_statistics, csrc/psi.hip):

  L  = chol(Kuu + jitter I),  B = L^-1 Psi2 L^-T,  LA = chol(I + B / s2),  c = LA^-1 L^-1 Psi1 Y
  F  = -P sum log diag LA - 1/2 sum(Y^2 / s2 + log 2 pi + log s2) + sum c^2 / (2 s2^2) - P psi0 / (2 s2) + P tr(B) / (2 s2)
       - KL(q(X) || N(0, I))       (latent_prior)

one deterministic evaluation with exact gradients.  The posterior over the inducing outputs has the form of the sparse GP's, so
prediction at deterministic test inputs is SparseGPRegressionMeanVariancePrediction unchanged: the module graph exposes X_mean as graph.X.
Prediction at uncertain test inputs is BayesianGPLVMUncertainInputPrediction (gp.gplvm_predict_uncertain, attached by the user).

  BayesianGPLVMLogPdf.compute -> mxf_psi_rbf_fwd / mxf_psi_rbf_bwd for the statistics in the model's dtype, kern.K + the differentiable
                                 mxf_potrf / mxf_trsm / mxf_gemm bridges (gp/_linalg.py) for the M x M chain, in float64
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from ... import ops
from ...common.exceptions import InferenceError, ModelSpecificationError
from ...components.variables.variable import Variable
from ...components.variables.var_trans import PositiveTransformation
from ...components.distributions.gp import _linalg as lin
from ...inference.inference_alg import SamplingAlgorithm
from ...inference.variational import VariationalInference
from ..module import Module, ModuleGraph
from .sparsegp_regression import SparseGPRegressionMeanVariancePrediction


class BayesianGPLVMLogPdf(VariationalInference):
    """The bound above.  It is not a sum over data rows (Psi2 sits inside a log-determinant): `log_pdf_scaling` must stay 1."""

    def __init__(self, model, posterior, observed, latent_prior=True, jitter=0.):
        super(BayesianGPLVMLogPdf, self).__init__(model=model, posterior=posterior, observed=observed)
        self.log_pdf_scaling = 1
        self.latent_prior = latent_prior
        self.jitter = jitter

    def compute(self, F, variables):
        g = self.model
        mu, s, Y, Z, noise_var = (variables[v] for v in (g.X, g.X_var, g.Y, g.inducing_inputs, g.noise_var))
        kern_params = g.kernel.fetch_parameters(variables)
        ops._require_gpu(mu)
        if Y.shape[-2] != mu.shape[-2]:
            raise InferenceError('BayesianGPLVM: %d rows of Y against %d rows of q(X) -- the bound is not a sum over data rows and cannot '
                                 'be evaluated on a minibatch' % (Y.shape[-2], mu.shape[-2]))
        if g.F.factor.has_mean:
            Y = Y - variables[g.mean]
        psi0, Psi1, Psi2 = g.kernel.psi_statistics(F, mu, s, Z, **kern_params)          # in the model's dtype
        # the M x M chain of a float32 model runs in float64 (SVGPLikelihoodLogPdf.compute: two Cholesky factorisations in a row lose
        # cond(Kuu) 2^-24 of the bound in float32), and the result is narrowed
        narrow = mu.dtype == torch.float32
        if narrow:
            psi0, Psi1, Psi2, Y, Z, noise_var = [t.double() for t in (psi0, Psi1, Psi2, Y, Z, noise_var)]
            kern_params = {k: v.double() for k, v in kern_params.items()}
        P, M = Y.shape[-1], Z.shape[-2]
        eye = torch.eye(M, dtype=Z.dtype, device=Z.device).unsqueeze(0)
        nv = noise_var.unsqueeze(-2)                                    # (S, 1, 1)
        Kuu = g.kernel.K(F, Z, **kern_params)
        if self.jitter > 0.:
            Kuu = Kuu + eye * self.jitter
        L, info = lin.chol(Kuu)
        S = max(t.shape[0] for t in (L, Psi1, Psi2, Y, nv))
        over = lambda t: t.expand((S,) + tuple(t.shape[1:])) if t.shape[0] == 1 and S > 1 else t
        B = lin.trsm(L, lin.trsm(L, over(Psi2)).transpose(-1, -2).contiguous())       # L^-1 (L^-1 Psi2)^T = L^-1 Psi2 L^-T
        LA, info2 = lin.chol(eye + B / nv)
        c = lin.trsm(LA, lin.trsm(L, lin.gemm(over(Psi1), over(Y))))
        logL = -P * torch.log(torch.diagonal(LA, dim1=-2, dim2=-1)).sum(-1)
        logL = logL - ((Y ** 2) / nv + math.log(2 * math.pi) + torch.log(nv)).sum(-1).sum(-1) / 2
        logL = logL + ((c ** 2) / (2 * nv ** 2)).sum(-1).sum(-1)
        logL = logL - P * psi0 / (2 * noise_var[:, 0])
        logL = logL + P * torch.diagonal(B, dim1=-2, dim2=-1).sum(-1) / (2 * noise_var[:, 0])
        if self.latent_prior:                                           # KL(N(mu, diag s) || N(0, I)), in the model's dtype like its operands
            kl = 0.5 * (s + mu * mu - 1.0 - torch.log(s)).sum(-1).sum(-1)
            logL = logL - (kl.double() if narrow else kl)
        self._last_info = ops.merge_info(info, info2)
        with torch.no_grad():      # persist sample 0 only, as SparseGPRegressionLogPdf does: wv = L^-T LA^-T c / s2
            wv = ops.trsm_(L[:1].contiguous(), ops.trsm_(LA[:1].contiguous(), c[:1].detach().contiguous().clone(), transpose=True),
                           transpose=True) / nv[:1]
            nf = (lambda t: t.float()) if narrow else (lambda t: t)
            self.set_parameter(variables, self.graphs[1].wv, nf(wv[0]))
            self.set_parameter(variables, self.graphs[1].L, nf(L[0].detach()))
            self.set_parameter(variables, self.graphs[1].LA, nf(LA[0].detach()))
        return logL.float() if narrow else logL


class BayesianGPLVMUncertainInputPrediction(SamplingAlgorithm):
    """The exact first two moments of the prediction at uncertain test inputs x*_n ~ N(X_mean[n], diag(X_var[n])), X_var >= 0 (the one step
    of moment-matched multi-step prediction).  With the persisted L, LA, wv and C = L^-T (I - LA^-T LA^-1) L^-1:

      mean[n, p] = sum_m Psi1*[m, n] wv[m, p]                        (+ the mean function)
      var[n, p]  = variance + sum_{m,m'} A_p[m,m'] psi2n*[n,m,m'] - (sum_m Psi1*[m, n] wv[m, p])^2,    A_p = wv_p wv_p^T - C

    (+ noise_var unless noise_free).  The variance differs per output column, because the spread of the mean under q(x*) does: both moments
    are (S, N*, P).  Only per-point variances; no reverse mode in the test inputs.

      compute -> mxf_psi_rbf_fwd (Psi1*) and mxf_psi_rbf_quad (the contraction, N* x P numbers from N* M^2 / 2 terms that are never stored) in
                 the model's dtype; C, A and the final cancellation in float64 through the mxf_trsm / mxf_gemm bridges
    """

    def __init__(self, model, posterior, observed, target_variables=None, noise_free=True):
        super(BayesianGPLVMUncertainInputPrediction, self).__init__(model=model, observed=observed, extra_graphs=[posterior],
                                                                    target_variables=target_variables)
        self.noise_free = noise_free

    def compute(self, F, variables):
        g, post = self.model, self.graphs[1]
        mu, s, Z, noise_var = (variables[v] for v in (g.X, g.X_var, g.inducing_inputs, g.noise_var))
        L, LA, wv = (variables[v].double() for v in (post.L, post.LA, post.wv))
        kern = g.kernel
        kern_params = kern.fetch_parameters(variables)
        ops._require_gpu(mu)
        with torch.no_grad():
            p = kern._strip(kern_params)
            stat = [t.contiguous() for t in (mu, s, Z, p['lengthscale'], p['variance'])]
            Psi1, _ = ops.psi_rbf(*stat, bool(kern.ARD), want_psi2=False)                     # (S, M, N*), in the model's dtype
            M = Z.shape[-2]
            eye = torch.eye(M, dtype=torch.float64, device=mu.device).unsqueeze(0)
            Linv = lin.trsm(L, eye.expand(L.shape[0], M, M))
            LAinvLinv = lin.trsm(LA, Linv)
            C = lin.gemm(Linv, Linv, transA=True) - lin.gemm(LAinvLinv, LAinvLinv, transA=True)
            wvt = wv.transpose(-1, -2)                                                         # (S|1, P, M)
            A = wvt.unsqueeze(-1) * wvt.unsqueeze(-2) - C.unsqueeze(1)                         # (S|1, P, M, M)
            R = kern.psi2_quadratic(F, mu, s, Z, A.to(mu.dtype), **kern_params).double()       # (S, N*, P)
            m0 = lin.gemm(Psi1.double(), wv, transA=True)                                      # (S, N*, P)
            var = p['variance'].double().unsqueeze(-1) + R - m0 * m0
            if not self.noise_free:
                var = var + noise_var.double().unsqueeze(-1)
            mean = m0 + variables[g.mean].double() if g.F.factor.has_mean else m0
            mean, var = mean.to(mu.dtype), var.to(mu.dtype)
        outcomes = {g.Y.uuid: (mean, var)}
        if self.target_variables:
            return tuple(outcomes[v] for v in self.target_variables)
        return outcomes


class BayesianGPLVM(Module):
    """Y[n, :] ~ N(f(x_n), noise_var), f_p ~ GP(mean, kernel) through M inducing points, x_n ~ q(x_n) = N(X_mean[n], diag(X_var[n])).

    X_mean / X_var not given: parameters of the module, (shape[0], kernel.input_dim), X_var positive; the prior on X is N(0, I)
    (latent_prior).  Given: variables of the outer model -- parameters, or observed data (an observed X_var is regression with noisy
    inputs; pass latent_prior=False there)."""

    row_additive = False     # Psi2 sits inside a log-determinant: the bound is not a sum over data rows

    def __init__(self, kernel, noise_var, X_mean, X_var, latent_prior=True, inducing_inputs=None, num_inducing=10, mean=None, rand_gen=None,
                 dtype=None, ctx=None):
        from ...components.distributions.gp.kernels.kernel import Kernel
        if type(kernel).psi_statistics is Kernel.psi_statistics or kernel.active_dims is not None or kernel.input_dim > ops._lib.PSI_MAX_Q:
            Kernel.psi_statistics(kernel, None, None, None, None)        # raises, naming what is supported
        if not isinstance(noise_var, Variable):
            noise_var = Variable(value=noise_var)
        if inducing_inputs is None:
            inducing_inputs = Variable(shape=(num_inducing, kernel.input_dim), initial_value=np.random.randn(num_inducing, kernel.input_dim))
        inputs = [('inducing_inputs', inducing_inputs), ('noise_var', noise_var)]
        self._q = {}             # q(X): the module's own parameters (define_variable made them) or inputs from the outer model
        for name, v in (('X_mean', X_mean), ('X_var', X_var)):
            v = v if isinstance(v, Variable) else Variable(value=v)
            if not getattr(v, '_gplvm_own', False):
                inputs.append((name, v))
            self._q[name] = v
        if mean is not None:
            inputs.append(('mean', mean))
        self._has_mean = mean is not None
        self._latent_prior = bool(latent_prior)
        object.__setattr__(self, 'kernel', kernel)
        super(BayesianGPLVM, self).__init__(inputs=inputs, outputs=None, input_names=[k for k, _ in inputs], output_names=['random_variable'],
                                            rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def _generate_outputs(self, output_shapes=None):
        self.set_outputs([Variable(shape=output_shapes['random_variable'])])

    def _build_module_graphs(self):
        Y = self.random_variable
        graph = ModuleGraph(name='bayesian_gplvm')
        graph.X = self._q['X_mean']            # under the name the sparse GP's prediction reads
        graph.X_var = self._q['X_var']
        graph.inducing_inputs = self.inducing_inputs
        M = self.inducing_inputs.shape[0]
        graph.noise_var = self.noise_var
        if self._has_mean:
            graph.mean = self.mean
        graph.F = SimpleNamespace(factor=SimpleNamespace(has_mean=self._has_mean, dtype=self.dtype, kernel=self.kernel))
        graph.Y = Y
        graph.kernel = self.kernel
        for n, v in self.kernel.parameters.items():
            setattr(graph, n, v)
        post = ModuleGraph(name='bayesian_gplvm_posterior')
        post.L = Variable(shape=(M, M))
        post.LA = Variable(shape=(M, M))
        post.wv = Variable(shape=(M, Y.shape[-1]))
        for v in (post.L, post.LA, post.wv):
            v.is_posterior_cache = True
        return graph, [post]

    def _attach_default_inference_algorithms(self):
        observed = [v for _, v in self.inputs] + [v for _, v in self.outputs]
        self.attach_log_pdf_algorithms(targets=self.output_names, conditionals=self.input_names,
                                       algorithm=BayesianGPLVMLogPdf(self._module_graph, self._extra_graphs[0], observed, self._latent_prior),
                                       alg_name='gplvm_log_pdf')
        observed = [v for _, v in self.inputs]
        self.attach_prediction_algorithms(targets=self.output_names, conditionals=self.input_names,
                                          algorithm=SparseGPRegressionMeanVariancePrediction(self._module_graph, self._extra_graphs[0], observed),
                                          alg_name='gplvm_predict')
        # not registered: the default prediction stays gplvm_predict.  A user re-attaches it under that name to predict at uncertain inputs.
        object.__setattr__(self, 'gplvm_predict_uncertain',
                           BayesianGPLVMUncertainInputPrediction(self._module_graph, self._extra_graphs[0], observed))

    def prepare_executor(self, rv_scaling=None, global_weight=None):
        if rv_scaling is not None and any(v.uuid in rv_scaling for _, v in self.outputs):
            raise InferenceError('BayesianGPLVM: the bound is not a sum over data rows (Psi2 sits inside a log-determinant) -- it cannot be '
                                 'evaluated on minibatches or row shards; use the full-batch loop')
        return super(BayesianGPLVM, self).prepare_executor(rv_scaling=rv_scaling, global_weight=global_weight)

    @staticmethod
    def define_variable(kernel, noise_var, shape, X_mean=None, X_var=None, latent_prior=True, inducing_inputs=None, num_inducing=10, mean=None,
                        rand_gen=None, dtype=None, ctx=None):
        def own(v, **kw):
            if v is not None:
                return v
            if shape is None or not isinstance(shape[0], (int, np.integer)):
                raise ModelSpecificationError('BayesianGPLVM: without X_mean / X_var the module creates them as (shape[0], %d) parameters, so '
                                              'shape[0] must be an integer; got shape = %r' % (kernel.input_dim, shape))
            v = Variable(shape=(int(shape[0]), kernel.input_dim), **kw)
            v._gplvm_own = True
            return v
        gp = BayesianGPLVM(kernel=kernel, noise_var=noise_var, X_mean=own(X_mean), X_var=own(X_var, transformation=PositiveTransformation(),
                                                                                               initial_value=0.5),
                           latent_prior=latent_prior, inducing_inputs=inducing_inputs, num_inducing=num_inducing, mean=mean, rand_gen=rand_gen,
                           dtype=dtype, ctx=ctx)
        gp._generate_outputs({'random_variable': shape})
        return gp.random_variable

    @property
    def X_mean(self):
        return self._q['X_mean']

    @property
    def X_var(self):
        return self._q['X_var']

    @property
    def random_variable(self):
        return self._outputs[0][1]
