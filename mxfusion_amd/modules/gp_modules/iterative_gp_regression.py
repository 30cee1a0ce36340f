"""IterativeGPRegression: exact GP regression without the N x N covariance matrix (Gardner et al. 2018; Wang et al. 2019, "Exact Gaussian
processes on a million data points").  No reference counterpart; the model-side surface is GPRegression's (the same variables, the same
sign and scaling of log_pdf, usable under MAP / GradBasedInference).

  IterativeGPRegressionLogPdf.compute                 -> one batched CG solve of (K + noise I) [Y | Z] on mxf_kmv, one mxf_kmv_bwd
  IterativeGPRegressionMeanVariancePrediction.compute -> mxf_kmv for the mean, CG on chunks of test columns for the variance

What is estimated.  With Khat = K + noise I, alpha = Khat^-1 Y, T probes z_i ~ N(0, P), P the pivoted-Cholesky preconditioner, U = Khat^-1 Z
and W = P^-1 Z:
  value     -1/2 sum_p y_p^T alpha_p - 1/2 P logdet_SLQ - 1/2 N P log 2 pi.  logdet_SLQ is a stochastic Lanczos QUADRATURE estimate of
            log|Khat| (slq_logdet): consistent in the probes and the CG iterations, not unbiased at a finite number of iterations.
  gradient  1/2 sum_p alpha_p^T dKhat alpha_p - P / (2 T) sum_i u_i^T dKhat w_i: an UNBIASED estimate of the gradient of the exact log-pdf
            (E[u_i^T dKhat w_i] = tr(Khat^-1 dKhat)), up to the CG tolerance.  It is not the derivative of the value's estimate.
The probes and the preconditioner are constants of an evaluation: nothing is differentiated through them.

The draw contract.  Per evaluation and per sample of the parameters, ONE call rand_gen.sample_normal(shape=(N + r, num_probes)), r the rank
the pivoted Cholesky reached (<= precond_rank; r = 0: P = noise I): Z = sqrt(noise) eps[:N] + L_r eps[N:].  A rand_gen that replays recorded
draws reproduces a run."""
import math
from types import SimpleNamespace

import torch

from ... import ops
from ...common.exceptions import ModelSpecificationError
from ...components.variables.variable import Variable
from ...components.distributions.gp import _iterative as it
from ...components.distributions.random_gen import TorchRandomGenerator
from ...inference.inference_alg import SamplingAlgorithm
from ...inference.variational import VariationalInference
from ..module import Module, ModuleGraph
from .gp_regression import GPRegressionSampling


def _require_fused(kernel):
    if kernel.fused_spec() is None:
        kernel.matvec(None, None, None)         # raises ModelSpecificationError, naming what is supported
    return kernel.fused_spec()


def _preconditioner(kind, ard, X, ls, var, noise, rank):
    """P = L_r L_r^T + noise I from the pivoted Cholesky of K(X, X); X (1, N, Q); rows of K through ops.gram with one row."""
    N = X.shape[1]
    row = lambda i: ops.gram(kind, X.index_select(1, i.reshape(1)), X, ls, var, ard)[0, 0]
    diag = var.reshape(()).expand(N).contiguous()
    return it.Preconditioner(it.pivoted_cholesky(row, diag, rank), float(noise), N)


class _IterativeLogPdfFn(torch.autograd.Function):
    """log N(Y | 0, K + noise I) of ONE sample of the parameters: X (1, N, Q), Y (1, N, P), noise (1, 1), ls (1, Q|1), var (1, 1).  Saves only
    alpha, U = Khat^-1 Z and W = P^-1 Z."""

    @staticmethod
    def forward(ctx, cfg, X, Y, noise, ls, var):
        kind, ard = cfg.kind, cfg.ard
        X, Y, noise, ls, var = [t.detach().contiguous() for t in (X, Y, noise, ls, var)]
        N, P, T = Y.shape[1], Y.shape[2], cfg.num_probes
        pre = _preconditioner(kind, ard, X, ls, var, noise, cfg.precond_rank)
        eps = cfg.rand_gen.sample_normal(shape=(N + pre.rank, T), dtype=X.dtype, ctx=X.device)
        Z = pre.sample(eps.to(device=X.device, dtype=X.dtype))
        B = torch.cat([Y[0], Z], dim=1)
        matvec = lambda V: ops.kernel_matvec(kind, X, None, ls, var, ard, V.unsqueeze(0).contiguous(), noise)[0]
        sol, iters, a, b = it.pcg(matvec, B, pre, tol=cfg.cg_tol, max_iter=cfg.max_cg_iter, check_every=cfg.check_every)
        alpha, U = sol[:, :P], sol[:, P:]
        W = pre.solve(Z)
        logdet = it.slq_logdet(a[:, P:], b[:, P:], iters[P:], (Z * W).sum(0), pre.logdet)
        cfg.last = SimpleNamespace(iterations=iters, logdet=logdet, rank=pre.rank)
        ctx.cfg = cfg
        ctx.save_for_backward(X, ls, var, alpha, U, W)
        value = -0.5 * (Y[0] * alpha).sum() - 0.5 * P * logdet - 0.5 * N * P * math.log(2.0 * math.pi)
        ctx.mark_non_differentiable(alpha)
        return value.reshape(1), alpha

    @staticmethod
    def backward(ctx, g, _):
        X, ls, var, alpha, U, W = ctx.saved_tensors
        cfg = ctx.cfg
        if ctx.needs_input_grad[1]:
            raise NotImplementedError('IterativeGPRegression has no reverse mode in X')
        P, T = alpha.shape[1], U.shape[1]
        w = [0.5] * P + [-0.5 * P / T] * T
        g = g.reshape(())
        dY = -g * alpha.unsqueeze(0) if ctx.needs_input_grad[2] else None
        dnoise = None
        if ctx.needs_input_grad[3]:
            dnoise = (g * (0.5 * (alpha * alpha).sum() - 0.5 * P / T * (U * W).sum())).reshape(1, 1)
        dls = torch.zeros_like(ls) if ctx.needs_input_grad[4] else None
        dvar = torch.zeros_like(var) if ctx.needs_input_grad[5] else None
        if dls is not None or dvar is not None:
            A = torch.cat([alpha, U], dim=1).unsqueeze(0).contiguous()
            V = torch.cat([alpha, W], dim=1).unsqueeze(0).contiguous()
            ops.kernel_matvec_bwd_(cfg.kind, X, None, ls, var, cfg.ard, A, V, w, dls, dvar)
            dls = None if dls is None else dls * g
            dvar = None if dvar is None else dvar * g
        return None, None, dY, dnoise, dls, dvar


def _sample(t, s):
    """sample s of a runtime array with the sample axis (extent 1: shared), keeping the axis"""
    return t[s:s + 1] if t.shape[0] > 1 else t


class IterativeGPRegressionLogPdf(VariationalInference):
    """log N(Y | mean, K + noise_var I) by conjugate gradients and stochastic Lanczos quadrature (the module docstring says what is estimated
    and how the probes are drawn).  alpha = Khat^-1 (Y - mean) of sample 0 is persisted for prediction, the analogue of GPRegression's LinvY."""

    def __init__(self, model, posterior, observed, num_probes=10, precond_rank=15, cg_tol=1e-8, max_cg_iter=1000, check_every=10,
                 rand_gen=None):
        super(IterativeGPRegressionLogPdf, self).__init__(model=model, posterior=posterior, observed=observed)
        self.log_pdf_scaling = 1
        self.cfg = SimpleNamespace(num_probes=int(num_probes), precond_rank=int(precond_rank), cg_tol=float(cg_tol),
                                   max_cg_iter=int(max_cg_iter), check_every=int(check_every),
                                   rand_gen=TorchRandomGenerator if rand_gen is None else rand_gen, last=None)

    def compute(self, F, variables):
        X = variables[self.model.X]
        Y = variables[self.model.Y]
        noise_var = variables[self.model.noise_var]
        kern = self.model.kernel
        self.cfg.kind, self.cfg.ard = _require_fused(kern)
        kern_params = kern.fetch_parameters(variables)
        ls, var = kern_params[kern.name + '_lengthscale'], kern_params[kern.name + '_variance']
        if self.model.F.factor.has_mean:
            Y = Y - variables[self.model.mean]
        if X.shape[-1] > ops._lib.KMV_MAX_Q:
            kern.matvec(F, X, Y)            # raises, naming the limit
        S = max(t.shape[0] for t in (X, Y, noise_var, ls, var))
        logL, alpha0 = [], None
        for s in range(S):
            val, alpha = _IterativeLogPdfFn.apply(self.cfg, *[_sample(t, s) for t in (X, Y, noise_var, ls, var)])
            logL.append(val)
            alpha0 = alpha if alpha0 is None else alpha0
        with torch.no_grad():           # only sample 0 is persisted, as GPRegressionLogPdf does
            self.set_parameter(variables, self.posterior.X, X[0].detach())
            self.set_parameter(variables, self.posterior.alpha, alpha0.detach())
        return torch.cat(logL)


class IterativeGPRegressionMeanVariancePrediction(SamplingAlgorithm):
    """mean = K(X*, X) alpha (+ mean function) by the matrix-free product in chunks of `chunk_rows` test rows; the diagonal variance
    k** - diag(K*^T Khat^-1 K*) by CG on chunks of at most `chunk_cols` test columns, each an N x chunk_cols right-hand side from ops.gram."""

    def __init__(self, model, posterior, observed, noise_free=True, precond_rank=15, cg_tol=1e-8, max_cg_iter=1000, check_every=10,
                 chunk_cols=256, chunk_rows=1 << 20):
        super(IterativeGPRegressionMeanVariancePrediction, self).__init__(model=model, observed=observed, extra_graphs=[posterior])
        self.noise_free = noise_free
        self.diagonal_variance = True
        self.precond_rank, self.cg_tol, self.max_cg_iter, self.check_every = int(precond_rank), float(cg_tol), int(max_cg_iter), int(check_every)
        self.chunk_cols, self.chunk_rows = int(chunk_cols), int(chunk_rows)

    def compute(self, F, variables):
        with torch.no_grad():
            Xt = variables[self.model.X]
            noise_var = variables[self.model.noise_var]
            X = variables[self.graphs[1].X]
            alpha = variables[self.graphs[1].alpha]
            kern = self.model.kernel
            kind, ard = _require_fused(kern)
            kern_params = kern.fetch_parameters(variables)
            ls, var = kern_params[kern.name + '_lengthscale'], kern_params[kern.name + '_variance']
            X, alpha = [t if t.dim() == 3 else t.unsqueeze(0) for t in (X, alpha)]
            if any(t.shape[0] != 1 for t in (Xt, X, alpha, noise_var, ls, var)):
                raise NotImplementedError('IterativeGPRegression predicts from one sample of the parameters and the test inputs')
            X, Xt, alpha, noise_var, ls, var = [t.contiguous() for t in (X, Xt, alpha, noise_var, ls, var)]
            Nt = Xt.shape[1]
            mu = torch.cat([kern.matvec(F, Xt[:, r:r + self.chunk_rows], alpha, X2=X, **kern_params) for r in range(0, Nt, self.chunk_rows)], dim=1)
            if self.model.F.factor.has_mean:
                mu = mu + variables[self.model.mean]
            pre = _preconditioner(kind, ard, X, ls, var, noise_var, self.precond_rank)
            matvec = lambda V: ops.kernel_matvec(kind, X, None, ls, var, ard, V.unsqueeze(0).contiguous(), noise_var)[0]
            v = []
            for c in range(0, Nt, self.chunk_cols):
                B = ops.gram(kind, X, Xt[:, c:c + self.chunk_cols].contiguous(), ls, var, ard)[0].contiguous()
                sol = it.pcg(matvec, B, pre, tol=self.cg_tol, max_iter=self.max_cg_iter, check_every=self.check_every)[0]
                v.append(var.reshape(()) - (B * sol).sum(0))
            v = torch.cat(v).unsqueeze(0)
            if not self.noise_free:
                v = v + noise_var
        outcomes = {self.model.Y.uuid: (mu, v)}
        if self.target_variables:
            return tuple(outcomes[v] for v in self.target_variables)
        return outcomes


class IterativeGPRegression(Module):
    """GPRegression's model, evaluated matrix-free: a single stationary kernel (RBF, Matern12 / 32 / 52, ARD or not) over all input
    dimensions, at most 16 of them; anything else is a ModelSpecificationError."""

    def __init__(self, X, kernel, noise_var, mean=None, num_probes=10, precond_rank=15, cg_tol=1e-8, max_cg_iter=1000, rand_gen=None, dtype=None,
                 ctx=None):
        _require_fused(kernel)
        if not isinstance(X, Variable):
            X = Variable(value=X)
        if not isinstance(noise_var, Variable):
            noise_var = Variable(value=noise_var)
        inputs = [('X', X), ('noise_var', noise_var)]
        if mean is not None:
            inputs.append(('mean', mean))
        self._has_mean = mean is not None
        self._solver = dict(num_probes=num_probes, precond_rank=precond_rank, cg_tol=cg_tol, max_cg_iter=max_cg_iter)
        object.__setattr__(self, 'kernel', kernel)
        super(IterativeGPRegression, self).__init__(inputs=inputs, outputs=None, input_names=[k for k, _ in inputs],
                                                    output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def _generate_outputs(self, output_shapes):
        shape = output_shapes['random_variable']
        Y_shape = tuple(self.X.shape[:-1]) + (1,) if shape is None else shape
        self.set_outputs([Variable(shape=Y_shape)])

    def _build_module_graphs(self):
        Y = self.random_variable
        graph = ModuleGraph(name='iterative_gp_regression')
        graph.X = self.X
        graph.noise_var = self.noise_var
        if self._has_mean:
            graph.mean = self.mean
        graph.F = SimpleNamespace(factor=SimpleNamespace(has_mean=self._has_mean, dtype=self.dtype, kernel=self.kernel))
        graph.Y = Y
        graph.kernel = self.kernel
        for n, v in self.kernel.parameters.items():
            setattr(graph, n, v)
        post = ModuleGraph(name='iterative_gp_regression_posterior')      # what prediction needs
        post.alpha = Variable(shape=tuple(self.X.shape[:-1]) + tuple(Y.shape[-1:]))
        post.X = Variable(shape=self.X.shape)
        for v in (post.alpha, post.X):
            v.is_posterior_cache = True
        return graph, [post]

    def _attach_default_inference_algorithms(self):
        observed = [v for _, v in self.inputs] + [v for _, v in self.outputs]
        s = self._solver
        self.attach_log_pdf_algorithms(targets=self.output_names, conditionals=self.input_names,
                                       algorithm=IterativeGPRegressionLogPdf(self._module_graph, self._extra_graphs[0], observed,
                                                                             rand_gen=self._rand_gen, **s),
                                       alg_name='iterative_gp_log_pdf')
        observed = [v for _, v in self.inputs]
        self.attach_draw_samples_algorithms(targets=self.output_names, conditionals=self.input_names,
                                            algorithm=GPRegressionSampling(self._module_graph, observed, rand_gen=self._rand_gen),
                                            alg_name='gp_sampling')
        self.attach_prediction_algorithms(targets=self.output_names, conditionals=self.input_names,
                                          algorithm=IterativeGPRegressionMeanVariancePrediction(
                                              self._module_graph, self._extra_graphs[0], observed, precond_rank=s['precond_rank'],
                                              cg_tol=s['cg_tol'], max_cg_iter=s['max_cg_iter']),
                                          alg_name='iterative_gp_predict')

    @staticmethod
    def define_variable(X, kernel, noise_var, shape=None, mean=None, num_probes=10, precond_rank=15, cg_tol=1e-8, max_cg_iter=1000, rand_gen=None,
                        dtype=None, ctx=None):
        gp = IterativeGPRegression(X=X, kernel=kernel, noise_var=noise_var, mean=mean, num_probes=num_probes, precond_rank=precond_rank,
                                   cg_tol=cg_tol, max_cg_iter=max_cg_iter, rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        gp._generate_outputs({'random_variable': shape})
        return gp.random_variable

    @property
    def random_variable(self):
        return self._outputs[0][1]
