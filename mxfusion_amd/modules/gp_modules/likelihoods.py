"""Non-Gaussian likelihoods of the sparse variational GP (svgp_likelihood.py): the expected log-likelihood under the Gaussian marginals
of q(f) by Gauss-Hermite quadrature, value and reverse mode in one HIP pass (mxf_lik_expect), and the predictive moments
(mxf_lik_moments).  No reference counterpart: the reference's SVGP has Gaussian noise only."""
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
