"""Non-Gaussian likelihoods of the sparse variational GP (svgp_likelihood.py): the expected log-likelihood under the Gaussian marginals
of q(f) by Gauss-Hermite quadrature, value and reverse mode in one HIP pass (mxf_lik_expect), and the predictive moments
(mxf_lik_moments); RobustMax, the multi-class likelihood over C latent functions per label column, on the row-wise kernel
(mxf_robustmax_expect, mxf_robustmax_probs).  No reference counterpart: the reference's SVGP has Gaussian noise only."""
import math

import torch

from ... import ops


class LikExpectFn(torch.autograd.Function):
    """out[s] = scale * sum_{n,p} E_{N(f; m, v)}[log p(y | f)], (S,).  The gradients in m and v (Price's theorem: ops.lik_expect_) are
    computed in the forward call and scaled by the upstream gradient in backward; y is not differentiated."""

    @staticmethod
    def forward(ctx, kind, num_nodes, scale, y, m, v):
        S = ops.num_samples(y, m, v)
        out = torch.zeros(S, dtype=m.dtype, device=m.device)
        want_m, want_v = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        dm = torch.zeros((S,) + tuple(m.shape[1:]), dtype=m.dtype, device=m.device) if want_m else None
        dv = torch.zeros((S,) + tuple(v.shape[1:]), dtype=m.dtype, device=m.device) if want_v else None
        ops.lik_expect_(kind, y.contiguous(), m.contiguous(), v.contiguous(), scale, out, dm_acc=dm, dv_acc=dv, num_nodes=num_nodes)
        ctx.grads, ctx.shared = (dm, dv), (m.shape[0] == 1 and S > 1, v.shape[0] == 1 and S > 1)
        return out

    @staticmethod
    def backward(ctx, g):
        out = []
        for d, shared, need in zip(ctx.grads, ctx.shared, ctx.needs_input_grad[4:]):
            if d is None or not need:
                out.append(None)
                continue
            d = d * g.reshape((-1,) + (1,) * (d.dim() - 1))       # (the upstream gradient may weight each sample differently)
            out.append(d.sum(0, keepdim=True) if shared else d)   # primal broadcast over S: its gradient sums over samples
        return (None, None, None, None) + tuple(out)


class Likelihood(object):
    """log p(y | f) of one observation given the latent function value, named by a kind of ops.LIK_KIND; `num_nodes` Gauss-Hermite nodes."""

    kind = None
    num_latent = None       # latent functions per label column; None: one per column of y
    count_like = False      # Var[y | f] = mu(f) (Poisson) instead of mu(f) (1 - mu(f)) (Bernoulli)

    def __init__(self, num_nodes=20):
        ops.lik_nodes(num_nodes)            # (refuses an order the kernel does not take)
        self.num_nodes = int(num_nodes)

    def expected_log_pdf_sum(self, y, m, v, scale=1.0):
        """scale * sum_{n,p} E_{N(f; m, v)}[log p(y | f)] per sample, (S,): y, m (S|1, N, P), v (S|1, N); differentiable in m and v"""
        return LikExpectFn.apply(self.kind, self.num_nodes, float(scale), y, m, v)

    def expected_log_pdf(self, y, m, v):
        """E_{N(f; m, v)}[log p(y | f)] per point, (S, N, P); not differentiable"""
        return ops.lik_expect_elem(self.kind, y.contiguous(), m.contiguous(), v.contiguous(), num_nodes=self.num_nodes)

    def predictive_moments(self, m, v):
        """(E[y], Var[y]) under f ~ N(m, v), each (S, N, P): E[mu], and E[Var[y | f]] + Var[mu(f)]"""
        e1, e2 = ops.lik_moments(self.kind, m.contiguous(), v.contiguous(), num_nodes=self.num_nodes)
        return e1, (e1 + e2 - e1 * e1 if self.count_like else e1 - e1 * e1)


class RobustMaxExpectFn(torch.autograd.Function):
    """out[s] = scale * sum_n E[log p(y | f)] of the robust-max likelihood, (S,).  The gradients in m and v (the exact derivatives of the
    quadrature sum: ops.robustmax_expect_) are computed in the forward call and scaled by the upstream gradient in backward; y is not
    differentiated."""

    @staticmethod
    def forward(ctx, eps, num_nodes, scale, y, m, v):
        S = ops.num_samples(y, m, v)
        out = torch.zeros(S, dtype=m.dtype, device=m.device)
        want_m, want_v = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        dm = torch.zeros((S,) + tuple(m.shape[1:]), dtype=m.dtype, device=m.device) if want_m else None
        dv = torch.zeros((S,) + tuple(v.shape[1:]), dtype=m.dtype, device=m.device) if want_v else None
        ops.robustmax_expect_(y.contiguous(), m.contiguous(), v.contiguous(), eps, scale, out, dm_acc=dm, dv_acc=dv, num_nodes=num_nodes)
        ctx.grads, ctx.shared = (dm, dv), (m.shape[0] == 1 and S > 1, v.shape[0] == 1 and S > 1)
        return out

    backward = staticmethod(LikExpectFn.backward)      # the same scaling and sample-axis sums


class BernoulliLogit(Likelihood):
    """y in {0, 1}, p(y = 1 | f) = sigmoid(f)"""
    kind = 'bernoulli_logit'


class BernoulliProbit(Likelihood):
    """y in {0, 1}, p(y = 1 | f) = Phi(f)"""
    kind = 'bernoulli_probit'


class PoissonExp(Likelihood):
    """y = 0, 1, 2, ..., y | f ~ Poisson(exp(f))"""
    kind = 'poisson_exp'
    count_like = True


class RobustMax(Likelihood):
    """y in {0, ..., C - 1} over C latent functions per row: p(y | f) = 1 - epsilon where f_y is the largest, epsilon / (C - 1) otherwise
    (Hernandez-Lobato et al. 2011).  The labels sit in one column, (S|1, N, 1), and m is (S|1, N, C).  The kernel reads a label clamped to
    [0, C - 1]; check_labels() validates them once, off the hot path."""

    def __init__(self, num_classes, epsilon=1e-3, num_nodes=20):
        super(RobustMax, self).__init__(num_nodes=num_nodes)
        if int(num_classes) != num_classes or not 2 <= int(num_classes) <= ops._lib.ROBUSTMAX_MAX_C:
            raise ValueError('RobustMax: 2 <= num_classes <= %d, got %r' % (ops._lib.ROBUSTMAX_MAX_C, num_classes))
        if not 0.0 < float(epsilon) < 1.0:
            raise ValueError('RobustMax: epsilon must lie in (0, 1), got %r' % (epsilon,))
        self.num_classes = self.num_latent = int(num_classes)
        self.epsilon = float(epsilon)

    @staticmethod
    def check_labels(y, num_classes):
        """Raises ValueError naming the first label that is not an integer in [0, num_classes - 1].  Reads y back (a device sync)."""
        flat = torch.as_tensor(y).detach().reshape(-1).double().cpu()
        bad = ~((flat == torch.floor(flat)) & (flat >= 0) & (flat <= num_classes - 1))
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            raise ValueError('RobustMax: label %r at flat index %d is not an integer in [0, %d]' % (float(flat[i]), i, num_classes - 1))

    def _check_m(self, m):
        if m.shape[-1] != self.num_classes:
            raise ValueError('RobustMax(%d): m carries %d latent functions' % (self.num_classes, m.shape[-1]))

    def expected_log_pdf_sum(self, y, m, v, scale=1.0):
        """scale * sum_n E[log p(y | f)] per sample, (S,): y (S|1, N, 1), m (S|1, N, C), v (S|1, N); differentiable in m and v"""
        self._check_m(m)
        return RobustMaxExpectFn.apply(self.epsilon, self.num_nodes, float(scale), y, m, v)

    def expected_log_pdf(self, y, m, v):
        """E[log p(y | f)] per point, (S, N, 1); not differentiable"""
        self._check_m(m)
        probs = ops.robustmax_probs(m.contiguous(), v.contiguous(), num_nodes=self.num_nodes)
        S = max(y.shape[0], probs.shape[0])
        idx = y.clamp(0, self.num_classes - 1).long().expand(S, -1, -1)      # (the label as the kernel reads it)
        l0, l1 = math.log(self.epsilon / (self.num_classes - 1)), math.log1p(-self.epsilon)
        return l0 + (l1 - l0) * torch.gather(probs.expand(S, -1, -1), -1, idx)

    def predictive_moments(self, m, v):
        """(probs, probs (1 - probs)), each (S, N, C): mean and variance of the one-hot indicator of the class whose f is the largest"""
        self._check_m(m)
        probs = ops.robustmax_probs(m.contiguous(), v.contiguous(), num_nodes=self.num_nodes)
        return probs, probs * (1.0 - probs)
