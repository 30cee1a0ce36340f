"""MultivariateNormal and MultivariateNormalMeanPrecision (mxfusion/components/distributions/normal.py:119-237, :332-456).

The random variable is (S|1, ..., n), the mean (S|1, ..., n) and the matrix (S|1, ..., n, n), each broadcastable against the variable's
leading dimensions; those are flattened into one batch axis B.  Up to order 32 the log-pdf is one autograd function over the fused
small-matrix kernels (mxf_mvn_factor / mxf_mvn_logpdf / mxf_mvn_logpdf_bwd, mvn.hip): an operand shared over an axis is passed as a
broadcast, never copied, and its gradient comes back summed.  Larger orders take the blocked dense path that the GP distributions use
(mxf_potrf / mxf_trsm / mxf_sumlogdiag through gp/_linalg.py), the matrices flattened onto the sample axis those calls batch over.
Draws are mean + L eps (covariance) or mean + L^-T eps (precision), one factorisation, differentiable through _linalg.CholFn."""
import math

import torch

from ... import ops
from ...common import config
from .distribution import Distribution
from .gp._linalg import CholLogPdfFn, chol, gemm, trsm
from ._fused import _flatten, _numel, carved_grads, replicate


class _MvnLogPdfFn(torch.autograd.Function):
    """scale * log N(x[s,b] | mean, A) (S, B) for n <= 32 and the factor stage's info words; x (S|1, B, n), mean (S|1, B|1, n),
    A (S|1, B|1, n, n) the covariance (form 0) or the precision (form 1).  The factor stage runs once, in forward; the reverse mode
    accumulates into one zero-filled buffer carved into the gradients that are wanted."""

    @staticmethod
    def forward(ctx, form, scale, x, mean, A):
        F, logdet, info = ops.mvn_factor(A, form)
        out = ops.mvn_logpdf(x, mean, F, logdet, form, scale)
        ctx.form, ctx.scale = form, float(scale)
        ctx.save_for_backward(x, mean, F)
        ctx.mark_non_differentiable(info)
        return out, info

    @staticmethod
    def backward(ctx, g, _):
        x, mean, F = ctx.saved_tensors
        grads = carved_grads((x.shape, mean.shape, F.shape), ctx.needs_input_grad[2:5], x)
        ops.mvn_logpdf_bwd_(x, mean, F, g.contiguous(), ctx.form, ctx.scale, *grads)
        return (None, None) + tuple(grads)


class _SpdLogDetFn(torch.autograd.Function):
    """log det K (S,) of symmetric positive definite K (S, n, n) through mxf_potrf and mxf_sumlogdiag; dK = g K^-1 (mxf_trtri, mxf_gemm)."""

    @staticmethod
    def forward(ctx, K):
        L, info = ops.potrf_(K.contiguous().clone())
        ctx.save_for_backward(L)
        ctx.mark_non_differentiable(info)
        return 2.0 * ops.sumlogdiag(L), info

    @staticmethod
    def backward(ctx, g, _):
        L, = ctx.saved_tensors
        Linv = ops.trtri(L)
        return ops.gemm(Linv, Linv, transA=True) * g.reshape(-1, 1, 1)


def _dense_log_pdf(form, x, mean, A):
    """The log-pdf (S, B) and the potrf info words for any order on the blocked dense calls: one matrix when A is shared by every row,
    otherwise one per row on the sample axis."""
    S, B, n = max(x.shape[0], mean.shape[0], A.shape[0]), x.shape[1], x.shape[2]
    d = (x - mean).expand(S, B, n).reshape(S * B, n, 1).contiguous()
    K = A.reshape(1, n, n) if A.shape[0] == 1 and A.shape[1] == 1 else A.expand(S, B, n, n).reshape(S * B, n, n)
    if form == 0:
        logL, _, _, info = CholLogPdfFn.apply(K, d)                                       # normal.py:172-178
    else:
        logdet, info = _SpdLogDetFn.apply(K)                                              # normal.py:384-394
        logL = -0.5 * (d * gemm(K, d)).reshape(S * B, n).sum(-1) + 0.5 * logdet - 0.5 * n * math.log(2 * math.pi)
    return logL.reshape(S, B), info


def _per_matrix(op, L, E):
    """op(L[s,b], E[s,b]) for L (S|1, B|1, n, n) and E (S, B, n) -> (S, B, n), op batched over a sample axis with L (S'|1, n, n) against
    (S', n, columns).  Matrices shared over the batch axis take its entries as the columns of one right-hand side."""
    (S_A, B_A, n), (S, B) = (L.shape[0], L.shape[1], L.shape[-1]), (E.shape[0], E.shape[1])
    if B_A == 1 and S_A == 1:
        R = E.reshape(S * B, n).transpose(0, 1).reshape(1, n, S * B).contiguous()
        return op(L.reshape(1, n, n), R).reshape(n, S * B).transpose(0, 1).reshape(S, B, n)
    if B_A == 1:
        return op(L.reshape(S_A, n, n), E.transpose(1, 2).contiguous()).transpose(1, 2)
    return op(L.expand(S, B, n, n).reshape(S * B, n, n), E.reshape(S * B, n, 1).contiguous()).reshape(S, B, n)


class _MultivariateNormalBase(Distribution):
    """What the two parameterisations share; `_form` is the kernels' form argument, `_matrix` the name of the second input."""
    _form = None
    _matrix = None

    def __init__(self, mean, matrix, rand_gen=None, minibatch_ratio=1., dtype=None, ctx=None):
        inputs = [('mean', self._as_variable(mean)), (self._matrix, self._as_variable(matrix))]
        super(_MultivariateNormalBase, self).__init__(inputs=inputs, outputs=None, input_names=['mean', self._matrix],
                                                      output_names=['random_variable'], rand_gen=rand_gen, dtype=dtype, ctx=ctx)

    def replicate_self(self, attribute_map=None):
        """normal.py:144-155, :356-367"""
        return replicate(self)

    def _log_pdf(self, mean, matrix, random_variable):
        n = int(matrix.shape[-1])
        lead = tuple(torch.broadcast_shapes(tuple(random_variable.shape[1:-1]), tuple(mean.shape[1:-1]), tuple(matrix.shape[1:-2])))
        x = _flatten(random_variable, lead, (n,), full=True)
        mean, matrix = _flatten(mean, lead, (n,)), _flatten(matrix, lead, (n, n))
        if n <= ops.MVN_MAX_ORDER:
            out, info = _MvnLogPdfFn.apply(self._form, float(self.log_pdf_scaling), x, mean, matrix)
        else:
            out, info = _dense_log_pdf(self._form, x, mean, matrix)
            out = out * self.log_pdf_scaling
        self._last_info = info
        return out.reshape((out.shape[0],) + lead)

    def _draw(self, mean, matrix, rv_shape, num_samples):
        rv_shape = tuple(int(s) for s in rv_shape)
        n = int(matrix.shape[-1])
        eps = self._rand_gen.sample_normal(shape=(num_samples,) + rv_shape + (1,), dtype=matrix.dtype, ctx=matrix.device)
        A = _flatten(matrix, rv_shape[:-1], (n, n))
        L, info = chol(A.reshape(-1, n, n))
        self._last_info = info
        E = eps.reshape(num_samples, _numel(rv_shape[:-1]), n)
        op = gemm if self._form == 0 else (lambda Lm, R: trsm(Lm, R, transpose=True))      # linalg.trmm(L, eps); precision: L^-T eps
        return _per_matrix(op, L.reshape(tuple(A.shape)), E).reshape((num_samples,) + rv_shape) + mean

    @classmethod
    def _define(cls, shape, mean, matrix, rand_gen, minibatch_ratio, dtype, ctx):
        if matrix is None:
            matrix = torch.eye(int(shape[-1]), dtype=config.torch_dtype(dtype))
        dist = cls(mean, matrix, rand_gen=rand_gen, minibatch_ratio=minibatch_ratio, dtype=dtype, ctx=ctx)
        dist._generate_outputs(shape=shape)
        return dist.random_variable


class MultivariateNormal(_MultivariateNormalBase):
    _form, _matrix = 0, 'covariance'

    def __init__(self, mean, covariance, rand_gen=None, minibatch_ratio=1., dtype=None, ctx=None):
        super(MultivariateNormal, self).__init__(mean, covariance, rand_gen=rand_gen, minibatch_ratio=minibatch_ratio, dtype=dtype, ctx=ctx)

    def log_pdf_impl(self, mean, covariance, random_variable, F=None):
        """normal.py:157-178, multiplied by log_pdf_scaling as there."""
        return self._log_pdf(mean, covariance, random_variable)

    def draw_samples_impl(self, mean, covariance, rv_shape, num_samples=1, F=None):
        """normal.py:180-202: mean + L eps, eps drawn in the shape (num_samples,) + rv_shape + (1,)."""
        return self._draw(mean, covariance, rv_shape, num_samples)

    @staticmethod
    def define_variable(shape, mean=0., covariance=None, rand_gen=None, minibatch_ratio=1., dtype=None, ctx=None):
        """normal.py:204-227: the default covariance is the identity of order shape[-1]."""
        return MultivariateNormal._define(shape, mean, covariance, rand_gen, minibatch_ratio, dtype, ctx)


class MultivariateNormalMeanPrecision(_MultivariateNormalBase):
    _form, _matrix = 1, 'precision'

    def __init__(self, mean, precision, rand_gen=None, minibatch_ratio=1., dtype=None, ctx=None):
        super(MultivariateNormalMeanPrecision, self).__init__(mean, precision, rand_gen=rand_gen, minibatch_ratio=minibatch_ratio,
                                                              dtype=dtype, ctx=ctx)

    def log_pdf_impl(self, mean, precision, random_variable, F=None):
        """normal.py:369-394: -1/2 (d^T P d + n log 2 pi - log det P), multiplied by log_pdf_scaling as there."""
        return self._log_pdf(mean, precision, random_variable)

    def draw_samples_impl(self, mean, precision, rv_shape, num_samples=1, F=None):
        """normal.py:396-421 as it is meant: mean + L^-T eps with P = L L^T, whose covariance is P^-1 (DESIGN.md section 1 on the
        reference's own line)."""
        return self._draw(mean, precision, rv_shape, num_samples)

    @staticmethod
    def define_variable(shape, mean=0., precision=None, rand_gen=None, minibatch_ratio=1., dtype=None, ctx=None):
        """normal.py:423-447: the default precision is the identity of order shape[-1]."""
        return MultivariateNormalMeanPrecision._define(shape, mean, precision, rand_gen, minibatch_ratio, dtype, ctx)
