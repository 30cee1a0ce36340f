"""VecchiaGPRegression: nearest-neighbour (Vecchia) GP regression (Vecchia 1988; Datta et al. 2016, "NNGP"; Katzfuss & Guinness 2021).  No
reference counterpart; the model-side surface is GPRegression's (the same variables, the same sign and scaling of log_pdf, usable under
MAP / GradBasedInference).

  VecchiaGPRegressionLogPdf.compute                 -> mxf_knn (causal, once per data set) and mxf_vecchia_logpdf / _bwd
  VecchiaGPRegressionMeanVariancePrediction.compute -> mxf_knn (not causal) and mxf_vecchia_cond on chunks of test rows

What is computed.  Rows are taken in a fixed order: the order given (ordering='given') or one seeded random permutation of it
(ordering='random', the default: a random order spreads each row's conditioning set over all length scales).  Row i is conditioned on the
num_neighbours <= 32 nearest rows that precede it, nearest in the metric of the kernel, |x - x'| / lengthscale:
    log p(Y | X) ~= sum_i log N(y_i | y_c(i)),
a deterministic approximation with an exact gradient, O(N k^3) work, and the exact log-pdf once num_neighbours >= N - 1.

The neighbour sets are found once per data set, at the first evaluation, with the lengthscale of that evaluation, and cached: they are
constants of an evaluation and nothing is differentiated through them.  refresh_neighbours() drops the cache (after the lengthscale has
moved far); a change of X's shape or storage drops it too.  A prediction conditions every test row on its num_neighbours nearest training
rows, with no ordering constraint."""
from types import SimpleNamespace

import torch

from ... import ops
from ...common.exceptions import ModelSpecificationError
from ...components.variables.variable import Variable
from ...inference.inference_alg import SamplingAlgorithm
from ...inference.variational import VariationalInference
from ..module import Module, ModuleGraph
from .gp_regression import GPRegressionSampling


def _require_fused(kernel):
    spec = kernel.fused_spec()
    if spec is None or kernel.input_dim > ops._lib.KNN_MAX_Q:
        raise ModelSpecificationError('VecchiaGPRegression is supported for a single stationary kernel (RBF, Matern12, Matern32, Matern52; ARD or '
                                      'not) over all input dimensions, at most %d of them; got %s over %d dimensions%s'
                                      % (ops._lib.KNN_MAX_Q, type(kernel).__name__, kernel.input_dim,
                                         ' with active_dims' if getattr(kernel, 'active_dims', None) is not None else ''))
    return spec


def _sample(t, s):
    """sample s of a runtime array with the sample axis (extent 1: shared), keeping the axis"""
    return t[s:s + 1] if t.shape[0] > 1 else t


def _scaled(X, ls):
    """X (N, Q) / lengthscale (Q|1 elements): the metric of the neighbour search"""
    return (X / ls.reshape(1, -1)).contiguous()


class VecchiaGPRegressionLogPdf(VariationalInference):
    """sum_i log N(y_i | y_c(i)) with mean function, the Vecchia approximation of log N(Y | mean, K + noise_var I).  The ordered X and
    Y - mean of sample 0 are persisted for prediction."""

    def __init__(self, model, posterior, observed, num_neighbours=16, ordering='random', seed=0):
        super(VecchiaGPRegressionLogPdf, self).__init__(model=model, posterior=posterior, observed=observed)
        self.log_pdf_scaling = 1
        self.num_neighbours, self.ordering, self.seed = int(num_neighbours), ordering, int(seed)
        self._cache = None

    def __deepcopy__(self, memo):
        """A cloned module finds its own neighbour sets."""
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            setattr(new, k, None if k == '_cache' else copy.deepcopy(v, memo))
        return new

    def refresh_neighbours(self):
        """Drop the cached neighbour sets: the next evaluation searches again, with its own lengthscale."""
        self._cache = None

    def permutation(self, N, device):
        if self.ordering == 'given':
            return None
        g = torch.Generator()
        g.manual_seed(self.seed)
        return torch.randperm(N, generator=g).to(device)

    def neighbours(self, X, ls):
        """(perm or None, nbr (N, k) int32 in the permuted order) of X (N, Q), from the cache where it still describes X"""
        key = (X.data_ptr(), tuple(X.shape), X.dtype, X.device)
        if self._cache is None or self._cache.key != key:
            with torch.no_grad():
                perm = self.permutation(X.shape[0], X.device)
                Xo = X if perm is None else X.index_select(0, perm)
                nbr, _ = ops.knn(_scaled(Xo, ls), None, self.num_neighbours, causal=True, want_d2=False)
            self._cache = SimpleNamespace(key=key, perm=perm, nbr=nbr)
        return self._cache.perm, self._cache.nbr

    def compute(self, F, variables):
        X = variables[self.model.X]
        Y = variables[self.model.Y]
        noise_var = variables[self.model.noise_var]
        kern = self.model.kernel
        kind, ard = _require_fused(kern)
        if X.shape[-1] > ops._lib.KNN_MAX_Q:
            raise ModelSpecificationError('VecchiaGPRegression: at most %d input dimensions; got %d' % (ops._lib.KNN_MAX_Q, X.shape[-1]))
        if torch.is_grad_enabled() and X.requires_grad:
            raise NotImplementedError('VecchiaGPRegression has no reverse mode in X: detach it')
        kern_params = kern.fetch_parameters(variables)
        ls, var = kern_params[kern.name + '_lengthscale'], kern_params[kern.name + '_variance']
        if self.model.F.factor.has_mean:
            Y = Y - variables[self.model.mean]
        perm, nbr = self.neighbours(X[0].detach(), ls[0].detach())
        if perm is not None:
            X, Y = X.index_select(1, perm), Y.index_select(1, perm)
        S = max(t.shape[0] for t in (X, Y, noise_var, ls, var))
        logL = []
        for s in range(S):
            Xs, Ys, ns, ls_s, vs = [_sample(t, s)[0] for t in (X, Y, noise_var, ls, var)]
            logL.append(ops.VecchiaLogPdf.apply(kind, ard, Xs, Ys, nbr, ns.reshape(1), ls_s.reshape(-1), vs.reshape(1)))
        with torch.no_grad():           # only sample 0 is persisted, as GPRegressionLogPdf does
            self.set_parameter(variables, self.posterior.X, X[0].detach())
            self.set_parameter(variables, self.posterior.Yc, Y[0].detach())
        return torch.cat(logL)


class VecchiaGPRegressionMeanVariancePrediction(SamplingAlgorithm):
    """mean = kappa^T (K_cc + noise I)^-1 (Y - mean)_c (+ mean function) and the diagonal variance k** - kappa^T (K_cc + noise I)^-1 kappa
    (+ noise unless noise_free), c the num_neighbours nearest training rows of each test row, in chunks of `chunk_rows` test rows."""

    def __init__(self, model, posterior, observed, noise_free=True, num_neighbours=16, chunk_rows=1 << 18):
        super(VecchiaGPRegressionMeanVariancePrediction, self).__init__(model=model, observed=observed, extra_graphs=[posterior])
        self.noise_free = noise_free
        self.diagonal_variance = True
        self.num_neighbours, self.chunk_rows = int(num_neighbours), int(chunk_rows)

    def compute(self, F, variables):
        with torch.no_grad():
            Xt = variables[self.model.X]
            noise_var = variables[self.model.noise_var]
            X = variables[self.graphs[1].X]
            Yc = variables[self.graphs[1].Yc]
            kern = self.model.kernel
            kind, ard = _require_fused(kern)
            kern_params = kern.fetch_parameters(variables)
            ls, var = kern_params[kern.name + '_lengthscale'], kern_params[kern.name + '_variance']
            X, Yc = [t if t.dim() == 3 else t.unsqueeze(0) for t in (X, Yc)]
            if any(t.shape[0] != 1 for t in (Xt, X, Yc, noise_var, ls, var)):
                raise NotImplementedError('VecchiaGPRegression predicts from one sample of the parameters and the test inputs')
            X, Xt, Yc, ls, var, noise = [t[0].contiguous() for t in (X, Xt, Yc, ls, var, noise_var)]
            ls, var, noise = ls.reshape(-1), var.reshape(1), noise.reshape(1)
            Xs = _scaled(X, ls)
            mu, v = [], []
            for r in range(0, Xt.shape[0], self.chunk_rows):
                xt = Xt[r:r + self.chunk_rows].contiguous()
                nbr, _ = ops.knn(_scaled(xt, ls), Xs, self.num_neighbours, causal=False, want_d2=False)
                m_, v_ = ops.vecchia_cond(kind, xt, X, Yc, nbr, ls, var, noise, ard)
                mu.append(m_)
                v.append(v_)
            mu, v = torch.cat(mu).unsqueeze(0), torch.cat(v).unsqueeze(0)
            if self.model.F.factor.has_mean:
                mu = mu + variables[self.model.mean]
            if not self.noise_free:
                v = v + noise_var
        outcomes = {self.model.Y.uuid: (mu, v)}
        if self.target_variables:
            return tuple(outcomes[v] for v in self.target_variables)
        return outcomes


class VecchiaGPRegression(Module):
    """GPRegression's model under the Vecchia approximation: a single stationary kernel (RBF, Matern12 / 32 / 52, ARD or not) over all input
    dimensions, at most 16 of them, and 1 <= num_neighbours <= 32; anything else is a ModelSpecificationError."""

    def __init__(self, X, kernel, noise_var, mean=None, num_neighbours=16, ordering='random', seed=0, rand_gen=None, dtype=None, ctx=None):
        _require_fused(kernel)
        if not 1 <= int(num_neighbours) <= ops._lib.KNN_MAX_K:
            raise ModelSpecificationError('VecchiaGPRegression: 1 <= num_neighbours <= %d; got %s' % (ops._lib.KNN_MAX_K, num_neighbours))
        if ordering not in ('random', 'given'):
            raise ModelSpecificationError("VecchiaGPRegression: ordering is 'random' or 'given'; got %r" % (ordering,))
        if not isinstance(X, Variable):
            X = Variable(value=X)
        if not isinstance(noise_var, Variable):
            noise_var = Variable(value=noise_var)
        inputs = [('X', X), ('noise_var', noise_var)]
        if mean is not None:
            inputs.append(('mean', mean))
        self._has_mean = mean is not None
        self._vecchia = dict(num_neighbours=int(num_neighbours), ordering=ordering, seed=int(seed))
        object.__setattr__(self, 'kernel', kernel)
        super(VecchiaGPRegression, self).__init__(inputs=inputs, outputs=None, input_names=[k for k, _ in inputs],
                                                  output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def _generate_outputs(self, output_shapes):
        shape = output_shapes['random_variable']
        Y_shape = tuple(self.X.shape[:-1]) + (1,) if shape is None else shape
        self.set_outputs([Variable(shape=Y_shape)])

    def _build_module_graphs(self):
        Y = self.random_variable
        graph = ModuleGraph(name='vecchia_gp_regression')
        graph.X = self.X
        graph.noise_var = self.noise_var
        if self._has_mean:
            graph.mean = self.mean
        graph.F = SimpleNamespace(factor=SimpleNamespace(has_mean=self._has_mean, dtype=self.dtype, kernel=self.kernel))
        graph.Y = Y
        graph.kernel = self.kernel
        for n, v in self.kernel.parameters.items():
            setattr(graph, n, v)
        post = ModuleGraph(name='vecchia_gp_regression_posterior')      # what prediction needs: the ordered X and Y - mean
        post.Yc = Variable(shape=tuple(self.X.shape[:-1]) + tuple(Y.shape[-1:]))
        post.X = Variable(shape=self.X.shape)
        for v in (post.Yc, post.X):
            v.is_posterior_cache = True
        return graph, [post]

    def _attach_default_inference_algorithms(self):
        observed = [v for _, v in self.inputs] + [v for _, v in self.outputs]
        self.attach_log_pdf_algorithms(targets=self.output_names, conditionals=self.input_names,
                                       algorithm=VecchiaGPRegressionLogPdf(self._module_graph, self._extra_graphs[0], observed, **self._vecchia),
                                       alg_name='vecchia_gp_log_pdf')
        observed = [v for _, v in self.inputs]
        self.attach_draw_samples_algorithms(targets=self.output_names, conditionals=self.input_names,
                                            algorithm=GPRegressionSampling(self._module_graph, observed, rand_gen=self._rand_gen),
                                            alg_name='gp_sampling')
        self.attach_prediction_algorithms(targets=self.output_names, conditionals=self.input_names,
                                          algorithm=VecchiaGPRegressionMeanVariancePrediction(
                                              self._module_graph, self._extra_graphs[0], observed,
                                              num_neighbours=self._vecchia['num_neighbours']),
                                          alg_name='vecchia_gp_predict')

    def refresh_neighbours(self):
        """Drop the cached neighbour sets of the log-pdf: the next evaluation searches again, with its own lengthscale."""
        self.vecchia_gp_log_pdf.refresh_neighbours()

    @staticmethod
    def define_variable(X, kernel, noise_var, shape=None, mean=None, num_neighbours=16, ordering='random', seed=0, rand_gen=None, dtype=None,
                        ctx=None):
        gp = VecchiaGPRegression(X=X, kernel=kernel, noise_var=noise_var, mean=mean, num_neighbours=num_neighbours, ordering=ordering, seed=seed,
                                 rand_gen=rand_gen, dtype=dtype, ctx=ctx)
        gp._generate_outputs({'random_variable': shape})
        return gp.random_variable

    @property
    def random_variable(self):
        return self._outputs[0][1]
