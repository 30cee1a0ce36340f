"""Coregionalize: the covariance between the outputs of a multi-output GP (GPy's Coregionalize, GPflow's Coregion, GPyTorch's IndexKernel;
the reference has none).  It acts on ONE input column that holds the output index t(x) in {0, .., T-1} of each row:

    k(x, x') = B[t(x), t(x')],   B = W W^T + diag(kappa),   W (T, rank) free, kappa (T,) positive.

Times a stationary kernel on the data columns it is the intrinsic coregionalisation model, cov(f_a(x), f_b(x')) = k(x, x') B[a, b]; a sum of
such products is the linear model of coregionalisation.  MultiplyKernel evaluates the product of a stationary kernel and a Coregionalize
kernel in one fused HIP pass (mxf_gram_icm / mxf_gram_icm_bwd; kernel.py: _GramICMFn).  Standing alone the kernel is plumbing -- a T x T
matrix formed and gathered by torch -- and runs on CPU tensors too.

It is a NativeKernel without a `_kind`, so fused_spec() stays None and every fused composite, the matrix-free product, the psi statistics,
pathwise sampling and Vecchia treat it as they treat any kernel they do not cover.  Inducing-point modules are not supported with an index
column: their inducing inputs are free real parameters and leave the integers, which the validation below reports."""
import numpy as np
import torch

from mxfusion_amd.common.exceptions import ModelSpecificationError
from mxfusion_amd.components.variables.variable import Variable
from mxfusion_amd.components.variables.var_trans import PositiveTransformation
from .kernel import NativeKernel


class Coregionalize(NativeKernel):
    """Coregionalize(num_outputs, rank=1, W=None, kappa=None): B = W W^T + diag(kappa) over `num_outputs` outputs.

    rank = 0: no W at all, B = diag(kappa) -- independent outputs with their own scales.
    Defaults: kappa = 1; W small, deterministic, different in every entry and of full column rank,
    W[t, r] = 0.1 cos(pi (t + 1/2) (r + 1/2) / T) exp(-t / (2 T)) / (r + 1): the DCT-IV basis, whose first min(T, rank) columns are mutually
    orthogonal, with every row scaled by exp(-t / (2 T)) and every column by 1 / (r + 1) -- scalings that keep the columns linearly
    independent and keep apart the entries that the basis alone has equal (W[t, r] and W[r, t]; a column of +-sqrt(1/2)).  Equal or
    merely proportional columns would span a subspace
    that dL/dW = 2 G W never leaves under SGD or momentum, so a rank >= 2 model would stay rank 1 for ever (the concern of
    SpectralMixture's defaults); and W = 0 is a stationary point of every objective that depends on W through W W^T."""

    def __init__(self, num_outputs, rank=1, W=None, kappa=None, name='coreg', active_dims=None, dtype=None, ctx=None):
        super(Coregionalize, self).__init__(input_dim=1, name=name, active_dims=active_dims, dtype=dtype, ctx=ctx)
        T, R = int(num_outputs), int(rank)
        if T < 1 or R < 0:
            raise ModelSpecificationError('Coregionalize takes num_outputs >= 1 and rank >= 0; got %d, %d' % (T, R))
        if active_dims is not None and len(list(active_dims)) != 1:
            raise ModelSpecificationError('Coregionalize acts on ONE column, the output index; got active_dims = %s' % (list(active_dims),))
        self.num_outputs, self.rank = T, R
        if R > 0:
            if W is None:
                t, r = np.arange(T, dtype=np.float64)[:, None], np.arange(R, dtype=np.float64)[None, :]
                W = 0.1 * np.cos(np.pi * (t + 0.5) * (r + 0.5) / T) * np.exp(-t / (2.0 * T)) / (r + 1.0)
            self.W = W if isinstance(W, Variable) else Variable(shape=(T, R), initial_value=np.asarray(W, dtype=np.float64).reshape(T, R))
        elif W is not None:
            raise ModelSpecificationError('Coregionalize(rank=0) has no W')
        if not isinstance(kappa, Variable):
            kappa = Variable(shape=(T,), transformation=PositiveTransformation(), initial_value=np.ones(T) if kappa is None else np.asarray(kappa, dtype=np.float64).reshape(T))
        self.kappa = kappa

    # ---- the pieces the fused product shares ------------------------------------------------------------------------------------------------
    def coregionalization_matrix(self, kappa, W=None):
        """B (S|1, T, T) = W W^T + diag(kappa) from the runtime parameters (sample axis first)."""
        B = torch.diag_embed(kappa)
        if W is not None:
            B = B + W @ W.transpose(-1, -2)
        return B

    def output_index(self, X):
        """The int32 index vector (N,) of the index column X (S|1, N, 1), validated: every value an integer in [0, T).  The indices are data
        and are shared by the samples.  Costs one small device reduction (and its synchronisation) per call."""
        col = X[..., 0]
        if col.shape[0] > 1:
            if not bool((col == col[:1]).all()):
                raise ModelSpecificationError('Coregionalize: the output index column differs between the samples')
        col = col[0]
        idx = col.to(torch.int32)
        bad = (idx.to(col.dtype) != col) | (col < 0) | (col >= self.num_outputs)
        if col.numel() and bool(bad.any()):
            v = float(col[bad][0])
            raise ModelSpecificationError('Coregionalize: the output index column holds %r; every value must be an integer in [0, %d) (inducing '
                                          'inputs and other free real-valued inputs cannot carry an output index)' % (v, self.num_outputs))
        return idx

    def _compute_K(self, F, X, kappa, W=None, X2=None):
        """B[idx[:, None], idx2[None, :]] (S, N, N2) by torch indexing; the gradient with respect to the index column is zero.  Validates
        the index column(s): one small device reduction per call (see output_index)."""
        B = self.coregionalization_matrix(kappa, W)
        idx = self.output_index(X).long()
        idx2 = idx if X2 is None else self.output_index(X2).long()
        return B[..., idx[:, None], idx2[None, :]]

    def _compute_Kdiag(self, F, X, kappa, W=None):
        B = self.coregionalization_matrix(kappa, W)
        idx = self.output_index(X).long()
        return B[..., idx, idx]

    # ---- data layout ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def stack(Xs, Ys=None):
        """The augmented inputs of heterotopic data: Xs a list of per-output inputs (N_t, Q) -> X (sum N_t, Q + 1) whose last column is
        the output index t of each row; with Ys, a list of per-output targets (N_t, 1), also the stacked Y (sum N_t, 1).  numpy arrays or
        torch tensors (the result is what the first input is)."""
        if len(Xs) == 0 or (Ys is not None and len(Ys) != len(Xs)):
            raise ValueError('Coregionalize.stack: one (N_t, Q) input (and one (N_t, 1) target) per output')
        is_torch = isinstance(Xs[0], torch.Tensor)
        cat = (lambda ts: torch.cat(ts, 0)) if is_torch else (lambda ts: np.concatenate(ts, 0))
        cols = []
        for t, x in enumerate(Xs):
            if x.ndim != 2 or x.shape[1] != Xs[0].shape[1]:
                raise ValueError('Coregionalize.stack: input %d is %s where (N_t, %d) is expected' % (t, tuple(x.shape), Xs[0].shape[1]))
            if Ys is not None and tuple(Ys[t].shape) != (x.shape[0], 1):
                raise ValueError('Coregionalize.stack: target %d is %s where (%d, 1) is expected' % (t, tuple(Ys[t].shape), x.shape[0]))
            index = torch.full((x.shape[0], 1), float(t), dtype=x.dtype, device=x.device) if is_torch else np.full((x.shape[0], 1), float(t), dtype=x.dtype)
            cols.append(torch.cat([x, index], 1) if is_torch else np.concatenate([x, index], 1))
        X = cat(cols)
        return X if Ys is None else (X, cat(list(Ys)))
