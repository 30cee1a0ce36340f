"""Pathwise posterior sampling for the three GP regression modules (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process
posteriors").  No reference counterpart: the reference's *SamplingPrediction algorithms draw point by point or through an Nt x Nt factor.

A sample is a FUNCTION: a prior draw expanded in D random Fourier features per kernel plus a kernel-basis update that conditions it,

    f(x) = ft(x) + K(x, B) V,      ft(x) = sum_d sqrt(2 var / D) w_d cos(omega_d . x + b_d),

with w ~ N(0, 1), b ~ U[0, 2 pi), omega_d = omegat_d / lengthscale, omegat ~ N(0, I) for the RBF kernel and omegat = z sqrt(2 nu / g), z ~ N(0, I),
g ~ Gamma(nu, rate 1/2) for Matern-nu.  B and V (xi, eps standard normal):

    SVGPRegression        B = Z,  V = Kuu^-1 (u - ft(Z)),  u = m + chol(S_W S_W^T + diag(S_diag)) xi
    GPRegression          B = X,  V = L^-T (L^-1 Y - L^-1 (ft(X) + sqrt(noise) eps))             (L, L^-1 Y: the persisted posterior)
    SparseGPRegression    B = Z,  V = wv + L^-T (LA^-T xi - L^-1 ft(Z))                          (L, LA, wv: the persisted posterior)

One basis (Omega, b) serves all samples and output columns: ft is one call of mxf_rff_eval with S = 1 and J = num_samples * P, which evaluates
every cosine once and stores nothing of size N x D.  K(x, B) V is mxf_gram and mxf_gemm.  Evaluation costs O(Nt (D + M)) per sample path and
can be repeated at new points (`PathwiseSamples.__call__`), where it is differentiable in them (mxf_rff_eval_bwd, mxf_gram_bwd).

Order of the draws, a contract (a generator that records what it hands out reproduces a run): per sub-kernel the normals (D, Q), for Matern the
gamma draw (D,), the uniform phases (D,); then the weights, normal (num_samples, D_total, P); then xi (num_samples, M, P) or eps (num_samples, N, P);
then, unless noise_free, normals (num_samples, Nt, P)."""
import math

import torch

from ... import ops
from ...common.exceptions import ModelSpecificationError
from ...components.distributions.gp import _linalg as lin
from ...components.distributions.gp.kernels.kernel import AddKernel
from ...components.distributions.gp.kernels.stationary import StationaryKernel
from ...inference.inference_alg import SamplingAlgorithm
from .gp_regression import _grad_mode

MATERN_NU = {'rbf': None, 'matern12': 0.5, 'matern32': 1.5, 'matern52': 2.5}


def spectral_blocks(kernel):
    """[(sub-kernel, prefix of its parameter names)] of a kernel with a random-feature expansion here; anything else raises, naming what is
    supported."""
    def ok(k):
        return isinstance(k, StationaryKernel) and k._kind in MATERN_NU and k.active_dims is None and k.input_dim <= ops._lib.RFF_MAX_Q

    if ok(kernel):
        return [(kernel, kernel.name + '_')]
    if isinstance(kernel, AddKernel) and kernel.active_dims is None and all(ok(k) and k.input_dim == kernel.input_dim for k in kernel.sub_kernels):
        return [(k, kernel.name + '_' + k.name + '_') for k in kernel.sub_kernels]
    raise ModelSpecificationError(
        'pathwise sampling is supported for a single RBF / Matern12 / Matern32 / Matern52 kernel over all input dimensions (ARD or not, at most '
        '%d of them) and for an AddKernel of such kernels; got %s%s' % (ops._lib.RFF_MAX_Q, _describe(kernel),
                                                                        ' with active_dims' if kernel.active_dims is not None else ''))


def _describe(kernel):
    subs = getattr(kernel, 'sub_kernels', None)
    return type(kernel).__name__ + ('' if subs is None else '(%s)' % ', '.join(_describe(k) for k in subs))


def _columns(t):
    """(num_samples, R, P) -> (1, R, num_samples * P): sample s, output p in column s * P + p"""
    return t.permute(1, 0, 2).reshape(1, t.shape[1], t.shape[0] * t.shape[2]).contiguous()


class PathwiseSamples(object):
    """num_samples drawn posterior functions: the basis Omega (1, D, Q) and phase (1, D), the weights W (1, D, num_samples * P), the update
    weights V (1, M, num_samples * P) on the kernel basis at B (1, M, Q), and the kernel with its parameters.  paths(Xnew), Xnew (N, Q) or
    (1, N, Q), is (num_samples, N, P): the same functions wherever they are evaluated, differentiable in Xnew.  Rows go through in chunks of
    `chunk_rows`.  A float32 model that records no autograd graph evaluates the update in float64 and the features in float32."""

    def __init__(self, kernel, kern_params, Omega, phase, W, B, V, num_samples, dtype, chunk_rows=65536):
        self.kernel, self.kern_params = kernel, kern_params
        self.Omega, self.phase, self.W, self.B, self.V = Omega, phase, W, B, V
        self.num_samples, self.dtype, self.chunk_rows = int(num_samples), dtype, int(chunk_rows)
        self._cast = {}

    def _in(self, dtype):
        """the stored operands in `dtype` (converted once)"""
        if dtype not in self._cast:
            c = lambda t: t.to(dtype).contiguous()
            self._cast[dtype] = (c(self.Omega), c(self.phase), c(self.W), c(self.B), c(self.V), {k: c(v) for k, v in self.kern_params.items()})
        return self._cast[dtype]

    def __call__(self, Xnew):
        X = Xnew if Xnew.dim() == 3 else Xnew.unsqueeze(0)
        if X.dim() != 3 or X.shape[0] != 1 or X.shape[-1] != self.Omega.shape[-1]:
            raise ValueError('pathwise samples are evaluated at deterministic inputs (N, %d) or (1, N, %d); got %s'
                             % (self.Omega.shape[-1], self.Omega.shape[-1], tuple(Xnew.shape)))
        with _grad_mode(X):
            graph = torch.is_grad_enabled()
            feat_dt = X.dtype                                          # the features run in the model's dtype
            upd_dt = X.dtype if graph else self.V.dtype                # the update in the dtype it was drawn in (float64 for a float32 model)
            Om, ph, W = self._in(feat_dt)[:3]
            _, _, _, B, V, kp = self._in(upd_dt)
            parts = []
            for r0 in range(0, X.shape[1], self.chunk_rows):
                Xc = X[:, r0:r0 + self.chunk_rows].contiguous()
                prior = ops.RFFEval.apply(Xc, Om, ph, W)                                   # (1, n, J)
                K = self.kernel.K(None, Xc.to(upd_dt), B, **kp)                            # (1, n, M)
                parts.append((prior.to(upd_dt) + lin.gemm(K, V)).to(self.dtype))
            f = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
            N, J = f.shape[1], f.shape[2]
            return f.reshape(N, self.num_samples, J // self.num_samples).permute(1, 0, 2).contiguous()


class _PathwiseSampling(SamplingAlgorithm):
    """The shared part of the three algorithms: the draws, the basis, the evaluation.  A subclass supplies `_update(variables, kern, kp, ft, dt)` -> (B, V); `paths`
    holds the PathwiseSamples of the last `compute`."""

    def __init__(self, model, posterior, observed, num_features=1024, rand_gen=None, noise_free=True, jitter=0., chunk_rows=65536,
                 target_variables=None):
        super(_PathwiseSampling, self).__init__(model=model, observed=observed, extra_graphs=[posterior], target_variables=target_variables)
        from ...components.distributions.random_gen import TorchRandomGenerator
        self._rand_gen = TorchRandomGenerator if rand_gen is None else rand_gen
        self.num_features, self.noise_free, self.jitter, self.chunk_rows = int(num_features), noise_free, jitter, int(chunk_rows)
        if self.num_features < 1 or self.chunk_rows < 1:
            raise ValueError('num_features and chunk_rows must be at least 1')
        spectral_blocks(self.model.kernel)       # an unsupported kernel is refused when the algorithm is built

    def _normal(self, shape, dt, device):
        return self._rand_gen.sample_normal(shape=tuple(shape), dtype=dt, ctx=device).to(dt)

    def _basis(self, kern_params, Q, P, dt, device):
        """Omega (1, D_total, Q), phase (1, D_total) and W (1, D_total, num_samples * P), the amplitude sqrt(2 var / D) of each block in W"""
        D, Om, ph, amp = self.num_features, [], [], []
        for k, prefix in spectral_blocks(self.model.kernel):
            ls, var = kern_params[prefix + 'lengthscale'].reshape(-1), kern_params[prefix + 'variance'].reshape(-1)
            w = self._normal((D, Q), dt, device)
            nu = MATERN_NU[k._kind]
            if nu is not None:
                g = self._rand_gen.sample_gamma(alpha=nu, beta=0.5, shape=(D,), dtype=dt, ctx=device).to(dt)
                w = w * torch.sqrt(2.0 * nu / g).reshape(D, 1)
            Om.append(w / ls)
            ph.append(self._rand_gen.sample_uniform(low=0., high=2.0 * math.pi, shape=(D,), dtype=dt, ctx=device).to(dt))
            amp.append(torch.sqrt(2.0 * var / D).expand(D))
        amp = torch.cat(amp)
        w = self._normal((self.num_samples, amp.shape[0], P), dt, device)
        return torch.cat(Om).unsqueeze(0).contiguous(), torch.cat(ph).unsqueeze(0).contiguous(), _columns(w * amp.reshape(1, -1, 1))

    def draw(self, F, variables):
        """Draw num_samples posterior functions: PathwiseSamples.  Everything here is independent of the test inputs and runs without an
        autograd graph; a float32 model on the GPU is widened to float64 for it, as the predictions of the modules are."""
        X = variables[self.model.X]
        kern = self.model.kernel
        kern_params = kern.fetch_parameters(variables)
        if any(t.shape[0] != 1 for t in kern_params.values()):
            raise ValueError('pathwise sampling needs one set of kernel parameters, not samples of them')
        Q, P = int(X.shape[-1]), int(self.model.Y.shape[-1])
        dt = torch.float64 if (X.dtype == torch.float32 and X.is_cuda) else X.dtype
        with torch.no_grad():
            kp = {k: v.detach().to(dt) for k, v in kern_params.items()}
            Omega, phase, W = self._basis(kp, Q, P, dt, X.device)
            ft = lambda pts: ops.rff_eval(pts.contiguous(), Omega, phase, W)
            B, V = self._update(variables, kern, kp, ft, dt)
        return PathwiseSamples(kern, kp, Omega, phase, W, B.contiguous(), V.contiguous(), self.num_samples, X.dtype, self.chunk_rows)

    def compute(self, F, variables):
        X = variables[self.model.X]
        with _grad_mode(X):
            self.paths = self.draw(F, variables)       # kept: alg.paths(Xnew) evaluates the same functions elsewhere
            samples = self.paths(X)
            if self.model.F.factor.has_mean:
                samples = samples + variables[self.model.mean]
            if not self.noise_free:
                noise = variables[self.model.noise_var].reshape(1, -1, 1)
                samples = samples + torch.sqrt(noise) * self._normal(samples.shape, samples.dtype, samples.device)
        outcomes = {self.model.Y.uuid: samples}
        if self.target_variables:
            return tuple(outcomes[v] for v in self.target_variables)
        return outcomes


class SVGPRegressionPathwiseSampling(_PathwiseSampling):
    """Sample paths of an SVGPRegression posterior: u ~ q(u) = N(m, S_W S_W^T + diag(S_diag)), f = ft + K(., Z) Kuu^-1 (u - ft(Z)).  `jitter` goes
    on Kuu, as in the module's predictions."""

    def _update(self, variables, kern, kp, ft, dt):
        post = self.graphs[1]
        Z, m, S_W, S_diag = [variables[v].detach().to(dt) for v in (self.model.inducing_inputs, post.qU_mean, post.qU_cov_W, post.qU_cov_diag)]
        M = Z.shape[-2]
        S = ops.gemm(S_W, S_W, transB=True) + ops.make_diagonal(S_diag)
        Ls, _ = ops.potrf_(S.contiguous())
        Kuu = kern.K(None, Z, **kp).contiguous().clone()
        if self.jitter > 0.:
            Kuu = Kuu + torch.eye(M, dtype=dt, device=Z.device) * self.jitter
        L, info = ops.potrf_(Kuu)
        self._last_info = info
        xi = _columns(self._normal((self.num_samples, M, m.shape[-1]), dt, Z.device))
        u = m.repeat(1, 1, self.num_samples) + ops.gemm(Ls, xi)
        r = (u - ft(Z)).contiguous()
        return Z, ops.trsm_(L, ops.trsm_(L, r), transpose=True)


class GPRegressionPathwiseSampling(_PathwiseSampling):
    """Sample paths of a GPRegression posterior from the factors its log-pdf persisted: f = ft + K(., X) (K + noise I)^-1 (Y - ft(X) - sqrt(noise) eps).
    `jitter` is not used: K + noise I is not factored again."""

    def _update(self, variables, kern, kp, ft, dt):
        post = self.graphs[1]
        Xc, L, LinvY, noise = [variables[v].detach().to(dt) for v in (post.X, post.L, post.LinvY, self.model.noise_var)]
        N = Xc.shape[-2]
        eps = _columns(self._normal((self.num_samples, N, LinvY.shape[-1]), dt, Xc.device))
        r = (ft(Xc) + torch.sqrt(noise.reshape(1, -1, 1)) * eps).contiguous()
        t = (LinvY.repeat(1, 1, self.num_samples) - ops.trsm_(L.contiguous(), r)).contiguous()
        return Xc, ops.trsm_(L.contiguous(), t, transpose=True)


class SparseGPRegressionPathwiseSampling(_PathwiseSampling):
    """Sample paths of a SparseGPRegression (or BayesianGPLVM, at deterministic inputs) posterior from the persisted L, LA, wv:
    f = ft + K(., Z) (wv + L^-T (LA^-T xi - L^-1 ft(Z))).  `jitter` is not used: Kuu is not factored again."""

    def _update(self, variables, kern, kp, ft, dt):
        post = self.graphs[1]
        Z, L, LA, wv = [variables[v].detach().to(dt).contiguous() for v in (self.model.inducing_inputs, post.L, post.LA, post.wv)]
        M = Z.shape[-2]
        xi = _columns(self._normal((self.num_samples, M, wv.shape[-1]), dt, Z.device))
        t = (ops.trsm_(LA, xi, transpose=True) - ops.trsm_(L, ft(Z).contiguous())).contiguous()
        return Z, wv.repeat(1, 1, self.num_samples) + ops.trsm_(L, t, transpose=True)
