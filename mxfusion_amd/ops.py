"""Tensor-level wrappers over the C ABI (include/mxf_gp.h).  PyTorch is used for device memory and
streams only; every array computation is a HIP kernel in libmxf_gp.so."""
import torch

from . import _lib
from ._lib import F32, F64, WRITE, ACC_ADD, ACC_MUL  # noqa: F401

KIND = {'rbf': _lib.K_RBF, 'matern12': _lib.K_MATERN12, 'matern32': _lib.K_MATERN32,
        'matern52': _lib.K_MATERN52, 'linear': _lib.K_LINEAR, 'bias': _lib.K_BIAS, 'white': _lib.K_WHITE}


def _require_gpu(t):
    if not t.is_cuda:
        raise _lib.MXFError('mxfusion_amd ops need device (HIP) tensors; got a %s tensor. There is no CPU '
                            'fallback.' % t.device)


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise TypeError('mxfusion_amd supports float32/float64, got %s' % t.dtype)


def _h(t):
    _require_gpu(t)
    return _lib.handle(t.device.index if t.device.index is not None else torch.cuda.current_device())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _ss(t):
    """sample stride in elements (0 => broadcast over S); the per-sample block must be contiguous."""
    if t is None:
        return 0
    return 0 if t.shape[0] == 1 else t.stride(0)


def _c(t):
    return None if t is None else (t if t.is_contiguous() else t.contiguous())


def num_samples(*ts):
    return max([t.shape[0] for t in ts if t is not None] + [1])


def _same_kind(what, ref, *others, contiguous=False):
    """The entry points take raw pointers: ref on a GPU and float32 or float64, every other operand (None: absent) on its device and of
    its dtype; with `contiguous`, all of them contiguous.  `what` names the family in the message."""
    _require_gpu(ref)
    _dt(ref)
    for t in (ref,) + others:
        if t is None:
            continue
        if t.dtype != ref.dtype or t.device != ref.device:
            raise TypeError('%s: every operand must have the dtype and device of the first (%s, %s); got %s, %s'
                            % (what, ref.dtype, ref.device, t.dtype, t.device))
        if contiguous and not t.is_contiguous():
            raise ValueError('%s: operands must be contiguous' % what)


def _shared_axes(t, axes, fits=torch.Tensor.is_contiguous):
    """(t, [(extent, stride in elements) for each of `axes`]) of an operand that may be shared over those leading axes.  An axis of extent
    1 or an expanded one (stride 0) is shared and reported as (1, 0); an expanded one is narrowed to extent 1 first, so that the copy made
    where t does not fit the kernel's layout (`fits`; None: every layout does) never materialises a shared axis.  An operand that fits is
    passed as it is."""
    for d in axes:
        if t.shape[d] > 1 and t.stride(d) == 0:
            t = t.narrow(d, 0, 1)
    if fits is not None and not fits(t):
        t = t.contiguous()
    return t, [(1, 0) if t.shape[d] == 1 else (int(t.shape[d]), int(t.stride(d))) for d in axes]


def _check_buffers(what, *pairs):
    """(buffer or None, shape) pairs -- the cotangent, and each gradient buffer against its operand's shape with the shared axes at extent
    1: contiguous and of that shape"""
    for t, shape in pairs:
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError('%s: the cotangent and the gradient buffers must be contiguous' % what)
        if tuple(t.shape) != tuple(shape):
            raise ValueError('%s: a buffer of shape %s where the operands ask for %s' % (what, tuple(t.shape), tuple(shape)))


def gram(kind, X, X2, lengthscale, variance, ard, diag_add=None, jitter=0.0, out=None, mode=WRITE):
    """K(X, X2) with the sample axis: X (S|1,N,Q), X2 (S|1,N2,Q) or None, lengthscale (S|1,Q|1),
    variance (S|1,1), diag_add (S|1,1) -> (S,N,N2).  Kernel.K (kernels/kernel.py:96-123)."""
    X, X2, lengthscale, variance, diag_add = _c(X), _c(X2), _c(lengthscale), _c(variance), _c(diag_add)
    S = num_samples(X, X2, lengthscale, variance, diag_add)
    N, Q = X.shape[-2], X.shape[-1]
    N2 = N if X2 is None else X2.shape[-2]
    if out is None:
        out = torch.empty((S, N, N2), dtype=X.dtype, device=X.device)
    if N == 0 or N2 == 0:       # empty operand: nothing to compute (an empty tensor has a null data pointer, which the ABI reads as "no X2")
        return out
    _lib.call('mxf_gram', _h(X), KIND[kind] if isinstance(kind, str) else kind, _dt(X), S, N, N2, Q,
              _p(X), _ss(X), _p(X2), _ss(X2), _p(lengthscale), int(bool(ard)), _ss(lengthscale),
              _p(variance), _ss(variance), _p(diag_add), _ss(diag_add), float(jitter), mode,
              _p(out), out.stride(-2), out.stride(0) if out.dim() == 3 else 0, _stream())
    return out


def gram2(kind1, kind2, op, X, X2, ls1, var1, ard1, ls2, var2, ard2, diag_add=None, jitter=0.0, out=None):
    """k1(X, X2) + k2(X, X2) (op = ACC_ADD) or their product (ACC_MUL) for two stationary kernels in ONE pass and one write (mxf_gram2):
    AddKernel / MultiplyKernel._compute_K (add_kernel.py:44-68, multiply_kernel.py:44-67).  Shapes as gram()."""
    X, X2, ls1, var1, ls2, var2, diag_add = _c(X), _c(X2), _c(ls1), _c(var1), _c(ls2), _c(var2), _c(diag_add)
    S = num_samples(X, X2, ls1, var1, ls2, var2, diag_add)
    N, Q = X.shape[-2], X.shape[-1]
    N2 = N if X2 is None else X2.shape[-2]
    if out is None:
        out = torch.empty((S, N, N2), dtype=X.dtype, device=X.device)
    if N == 0 or N2 == 0:
        return out
    k = lambda kk: KIND[kk] if isinstance(kk, str) else kk
    _lib.call('mxf_gram2', _h(X), k(kind1), k(kind2), op, _dt(X), S, N, N2, Q, _p(X), _ss(X), _p(X2), _ss(X2), _p(ls1), int(bool(ard1)), _ss(ls1),
              _p(var1), _ss(var1), _p(ls2), int(bool(ard2)), _ss(ls2), _p(var2), _ss(var2), _p(diag_add), _ss(diag_add), float(jitter),
              _p(out), out.stride(-2), out.stride(0) if out.dim() == 3 else 0, _stream())
    return out


def gemm(A, B, transA=False, transB=False, alpha=1.0, beta=0.0, out=None):
    """Batched C = alpha op(A) op(B) + beta C on (S|1, m, k) operands -- linalg.gemm2 / syrk."""
    A, B = _c(A), _c(B)
    S = num_samples(A, B)
    M = A.shape[-1] if transA else A.shape[-2]
    K = A.shape[-2] if transA else A.shape[-1]
    N = B.shape[-2] if transB else B.shape[-1]
    if out is None:
        out = torch.empty((S, M, N), dtype=A.dtype, device=A.device)
    _lib.call('mxf_gemm', _h(A), _dt(A), int(transA), int(transB), M, N, K, float(alpha), _p(A), A.stride(-2), _ss(A),
              _p(B), B.stride(-2), _ss(B), float(beta), _p(out), out.stride(-2), out.stride(0), S, _stream())
    return out


def gemm_f32x3(A, B, alpha=1.0, beta=0.0, out=None, lower_only=False):
    """C = alpha A B^T + beta C for float32 A (M,K), B (N,K) on the bf16 matrix pipe with three-term splitting (f32-equivalent)."""
    A, B = _c(A), _c(B)
    if A.dtype != torch.float32 or B.dtype != torch.float32 or A.dim() != 2 or B.dim() != 2:
        raise ValueError('gemm_f32x3: 2-D float32 operands')
    M, K = A.shape
    N = B.shape[0]
    if out is None:
        out = torch.zeros((M, N), dtype=A.dtype, device=A.device) if lower_only else torch.empty((M, N), dtype=A.dtype, device=A.device)
    _lib.call('mxf_gemm_f32x3', _h(A), M, N, K, float(alpha), _p(A), A.stride(0), _p(B), B.stride(0), float(beta), _p(out), out.stride(0),
              int(bool(lower_only)), _stream())
    return out


def gemm_f16x2(A, B, alpha=1.0, beta=0.0, out=None, lower_only=False):
    """C = alpha A B^T + beta C for float32 A (M,K), B (N,K) on the f16 matrix pipe: two scaled f16 terms per operand, three products
    (f32-equivalent normwise; half the matrix-pipe work of gemm_f32x3)."""
    A, B = _c(A), _c(B)
    if A.dtype != torch.float32 or B.dtype != torch.float32 or A.dim() != 2 or B.dim() != 2:
        raise ValueError('gemm_f16x2: 2-D float32 operands')
    M, K = A.shape
    N = B.shape[0]
    if out is None:
        out = torch.zeros((M, N), dtype=A.dtype, device=A.device) if lower_only else torch.empty((M, N), dtype=A.dtype, device=A.device)
    _lib.call('mxf_gemm_f16x2', _h(A), M, N, K, float(alpha), _p(A), A.stride(0), _p(B), B.stride(0), float(beta), _p(out), out.stride(0),
              int(bool(lower_only)), _stream())
    return out


def f16x2_split(X):
    """The two scaled f16 planes of a 2-D float32 operand and its max-abs word (see gemm_f16x2_planes)."""
    X = _c(X)
    R, K = X.shape
    if X.dtype != torch.float32 or X.dim() != 2:
        raise ValueError('f16x2_split: 2-D float32 operand')
    n = _lib.load().mxf_f32x3_plane_elems(R, K)
    planes = torch.empty(2 * n, dtype=torch.int16, device=X.device)
    word = torch.zeros(1, dtype=torch.int32, device=X.device)
    _lib.call('mxf_f16x2_split', _h(X), R, K, _p(X), X.stride(0), _p(planes), _p(word), _stream())
    return planes, word


def gemm_f16x2_planes(A_split, B_split, M, N, K, alpha=1.0, beta=0.0, out=None, lower_only=False, blocked=False):
    """C = alpha A B^T + beta C from operands already split by f16x2_split (reuse across products).  blocked: the full product with C in
    16-column blocks, element (m, n) at ((n // 16) * M + m) * 16 + n % 16 of `out` (the layout the SVGP training step keeps T in)."""
    (pa, wa), (pb, wb) = A_split, B_split
    if out is None:
        out = torch.zeros((M, N), dtype=torch.float32, device=pa.device) if lower_only else torch.empty((M, N), dtype=torch.float32, device=pa.device)
    _lib.call('mxf_gemm_f16x2_planes', _h(pa), M, N, K, float(alpha), _p(pa), _p(wa), _p(pb), _p(wb), float(beta), _p(out), out.stride(0),
              2 if blocked else int(bool(lower_only)), _stream())
    return out


def gemm_f16x2_planes_kmajor(A_split, Bt_split, M, N, K, alpha=1.0, out=None, blocked=False, w=None):
    """C (M x N) = alpha A (M x K) Bt (K x N) from split operands, Bt_split = f16x2_split of the (K x N) matrix itself -- the product that lets
    the SVGP step form T = H0 Kuf from the planes of Kuf that Psi2 reads (mxf_gemm_f16x2_planes_kmajor).  w (K,) float32: also returns
    U[n] = sum_k w[k] Bt[k][n] from the same launch."""
    (pa, wa), (pb, wb) = A_split, Bt_split
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=pa.device)
    U = torch.empty(N, dtype=torch.float32, device=pa.device) if w is not None else None
    wc = _c(w) if w is not None else None
    _lib.call('mxf_gemm_f16x2_planes_kmajor', _h(pa), M, N, K, float(alpha), _p(pa), _p(wa), _p(pb), _p(wb), _p(out), int(bool(blocked)),
              _p(wc) if wc is not None else None, _p(U) if U is not None else None, _stream())
    return (out, U) if w is not None else out


def gemm_f16x2_planes_out(A_split, B_split, M, N, K, alpha=1.0, a_lower=False, transposed=False, a=None):
    """alpha A B^T written directly as the two f16 planes (unscaled hi + lo) of the (M x N) operand whose contraction index is its column
    (mxf_gemm_f16x2_planes_out: chained split products; M % 128 == 0, N % 256 == 0).  Returns the int16 planes tensor; transposed=True: also
    the planes of the (N x M) transpose from the same launch; with a (M,) float32 also U[n] = sum_m a[m] (hi + lo)(m, n)."""
    (pa, wa), (pb, wb) = A_split, B_split
    n = _lib.load().mxf_f32x3_plane_elems(M, N)
    out = torch.empty(2 * n, dtype=torch.int16, device=pa.device)
    transposed = transposed or a is not None
    outT = torch.empty(2 * _lib.load().mxf_f32x3_plane_elems(N, M), dtype=torch.int16, device=pa.device) if transposed else None
    U = torch.empty(N, dtype=torch.float32, device=pa.device) if a is not None else None
    _lib.call('mxf_gemm_f16x2_planes_out', _h(pa), M, N, K, float(alpha), _p(pa), _p(wa), _p(pb), _p(wb), _p(out), _p(outT),
              _p(_c(a)) if a is not None else None, _p(U), int(bool(a_lower)), _stream())
    if not transposed:
        return out
    return (out, outT) if U is None else (out, outT, U)


def f16x2_planes_transpose(planes, R, K, a=None, scale=None):
    """Planes of an (R x K) operand -> planes of its transpose (K x R) (mxf_f16x2_planes_transpose); with a (R,) and scale (1,) float32 also
    U[k] = scale * sum_r a[r] x(r, k).  Returns planes_T or (planes_T, U)."""
    n = _lib.load().mxf_f32x3_plane_elems(K, R)
    out = torch.empty(2 * n, dtype=torch.int16, device=planes.device)
    U = torch.empty(K, dtype=torch.float32, device=planes.device) if a is not None else None
    _lib.call('mxf_f16x2_planes_transpose', _h(planes), R, K, _p(planes), _p(out), _p(_c(a)) if a is not None else None,
              _p(_c(scale)) if scale is not None else None, _p(U), _stream())
    return out if U is None else (out, U)


def planes_to_dense(planes, R, K):
    """Decode two f16 planes (k16-blocked, element (r, k) at ((k // 16) * R + r) * 16 + k % 16) to the float64 matrix hi + lo (test helper)."""
    K16 = (K + 15) // 16
    n = K16 * R * 16
    v = planes.view(torch.float16)
    dec = lambda q: v[q * n:(q + 1) * n].view(K16, R, 16).permute(1, 0, 2).reshape(R, K16 * 16)[:, :K].double()
    return dec(0) + dec(1)


def gram_planes(kind, Xmin, Xmaj, ls, var, ard, w=None, majs=None, mins=None, period=1):
    """The Gram matrix cov(Xmin[r], Xmaj[k]) of float32 inputs written directly as two f16 planes (mxf_gram_planes, the first stage of the
    float32 SVGP step): Xmin (R, Q), Xmaj (Kn, Q), ls (Q,) if ard else (1,), var (1,).  Returns the int16 planes tensor --
    planes_to_dense(planes, R, Kn) * var / 2**14 is the Gram matrix -- and, with w (Kn, Pw <= 8), also U (Pw, R) = w^T K^T from the same
    pass.  majs / mins (period,): every covariance times majs[k % period] and / or mins[r % period]."""
    f = lambda t: None if t is None else _c(t).reshape(-1)
    Xmin, Xmaj, ls, var, w, majs, mins = _c(Xmin), _c(Xmaj), f(ls), f(var), _c(w), f(majs), f(mins)
    _same_kind('gram_planes', Xmin, Xmaj, ls, var, w, majs, mins)
    if Xmin.dtype != torch.float32 or Xmin.dim() != 2 or Xmaj.dim() != 2 or Xmaj.shape[1] != Xmin.shape[1]:
        raise ValueError('gram_planes: float32 Xmin (R, Q) and Xmaj (Kn, Q)')
    (R, Q), Kn = Xmin.shape, Xmaj.shape[0]
    if ls.numel() != (Q if ard else 1) or var.numel() != 1:
        raise ValueError('gram_planes: lengthscale of %d entries and one variance' % (Q if ard else 1))
    if w is not None and (w.dim() != 2 or w.shape[0] != Kn):
        raise ValueError('gram_planes: w (Kn, Pw)')
    period = int(period)
    for s in (majs, mins):
        if s is not None and s.numel() < period:
            raise ValueError('gram_planes: majs / mins hold `period` entries')
    planes = torch.empty(2 * _lib.load().mxf_f32x3_plane_elems(R, Kn), dtype=torch.int16, device=Xmin.device)
    Pw = 0 if w is None else w.shape[1]
    U = None if w is None else torch.empty((Pw, R), dtype=torch.float32, device=Xmin.device)
    if R > 0 and Kn > 0:
        _lib.call('mxf_gram_planes', _h(Xmin), KIND[kind] if isinstance(kind, str) else kind, R, Kn, Q, _p(Xmin), _p(Xmaj), _p(ls),
                  int(bool(ard)), _p(var), _p(planes), _p(w), Pw, _p(U), R, _p(majs), _p(mins), period, _stream())
    return planes if w is None else (planes, U)


def f32x3_split(X):
    """Three-term bf16 split planes of a 2-D float32 matrix (operand format of gemm_f32x3_planes); returns an int16 tensor."""
    X = _c(X)
    if X.dtype != torch.float32 or X.dim() != 2:
        raise ValueError('f32x3_split: 2-D float32 operand')
    R, K = X.shape
    n = _lib.load().mxf_f32x3_plane_elems(R, K)
    planes = torch.empty(3 * n, dtype=torch.int16, device=X.device)
    _lib.call('mxf_f32x3_split', _h(X), R, K, _p(X), X.stride(0), _p(planes), _stream())
    return planes


def gemm_f32x3_planes(A_planes, B_planes, M, N, K, alpha=1.0, beta=0.0, out=None, lower_only=False):
    """C (M,N) = alpha A B^T + beta C from operands split with f32x3_split (A: (M,K), B: (N,K))."""
    if out is None:
        out = torch.zeros((M, N), dtype=torch.float32, device=A_planes.device) if lower_only else torch.empty((M, N), dtype=torch.float32, device=A_planes.device)
    _lib.call('mxf_gemm_f32x3_planes', _h(A_planes), M, N, K, float(alpha), _p(A_planes), _p(B_planes), float(beta), _p(out), out.stride(0),
              int(bool(lower_only)), _stream())
    return out


def gram_bwd(kind, X, X2, lengthscale, variance, ard, dK, need=('X', 'X2', 'ls', 'var')):
    """Reverse mode of gram(); returns (dX, dX2, dls, dvar) shaped like their primals (summed over S for
    broadcast operands)."""
    X, X2, lengthscale, variance, dK = _c(X), _c(X2), _c(lengthscale), _c(variance), _c(dK)
    S = dK.shape[0]
    N, Q = X.shape[-2], X.shape[-1]
    N2 = N if X2 is None else X2.shape[-2]
    dX = torch.zeros_like(X) if 'X' in need else None
    dX2 = torch.zeros_like(X2) if (X2 is not None and 'X2' in need) else None
    dls = torch.zeros_like(lengthscale) if 'ls' in need else None
    dvar = torch.zeros_like(variance) if 'var' in need else None
    _lib.call('mxf_gram_bwd', _h(X), KIND[kind] if isinstance(kind, str) else kind, _dt(X), S, N, N2, Q,
              _p(X), _ss(X), _p(X2), _ss(X2), _p(lengthscale), int(bool(ard)), _ss(lengthscale), _p(variance), _ss(variance),
              _p(dK), dK.stride(-2), dK.stride(0), _p(dX), _p(dX2), _p(dls), _p(dvar), _stream())
    return dX, dX2, dls, dvar


KIND_DIFF = {'periodic': _lib.KD_PERIODIC, 'rq': _lib.KD_RQ, 'sm': _lib.KD_SM}


def _diff_operands(what, kind, ard, X, X2, p0, p1, p2, *others):
    """(kind code, contiguous operands, A) of the difference-form families: X (S|1, N, Q), X2 (S|1, N2, Q) or None, and per kind
    periodic: variance (S|1, 1), lengthscale (S|1, Q|1), period (S|1, Q|1);  rq: variance, lengthscale, alpha (S|1, 1);
    sm: weights (S|1, A), means (S|1, A, Q), scales (S|1, A, Q)."""
    _same_kind(what, X, X2, p0, p1, p2, *others)
    kd = KIND_DIFF[kind] if isinstance(kind, str) else kind
    if kd == _lib.KD_SM and not (p1.dim() == 3 and p1.shape[-2:] == (p0.shape[-1], X.shape[-1]) and p2.shape[-2:] == p1.shape[-2:]):
        raise ValueError('%s: a spectral mixture takes weights (S|1, A), means and scales (S|1, A, Q); got %s, %s, %s'
                         % (what, tuple(p0.shape), tuple(p1.shape), tuple(p2.shape)))
    if kd != _lib.KD_SM:
        n = X.shape[-1] if ard else 1
        want = (1, n, n if kd == _lib.KD_PERIODIC else 1)
        if tuple(t.shape[-1] for t in (p0, p1, p2)) != want:
            raise ValueError('%s: %s takes parameter operands of extents %s (ard = %s, Q = %d); got %s, %s, %s'
                             % (what, kind, want, bool(ard), X.shape[-1], tuple(p0.shape), tuple(p1.shape), tuple(p2.shape)))
    return kd, [_c(t) for t in (X, X2, p0, p1, p2)], (p0.shape[-1] if kd == _lib.KD_SM else 1)


def gram_diff(kind, X, X2, p0, p1, p2, ard, diag_add=None, jitter=0.0, out=None):
    """K(X, X2) (S, N, N2) of a covariance that works on the per-dimension differences (mxf_gram_diff): kind 'periodic', 'rq' or 'sm' with
    the three parameter operands _diff_operands lists; diag_add (S|1, 1) and jitter go on the diagonal of a square Gram (X2 None)."""
    kd, (X, X2, p0, p1, p2), A = _diff_operands('gram_diff', kind, ard, X, X2, p0, p1, p2, diag_add, out)
    diag_add = _c(diag_add)
    S = num_samples(X, X2, p0, p1, p2, diag_add)
    N, Q = X.shape[-2], X.shape[-1]
    N2 = N if X2 is None else X2.shape[-2]
    if out is None:
        out = torch.empty((S, N, N2), dtype=X.dtype, device=X.device)
    if N == 0 or N2 == 0:
        return out
    _lib.call('mxf_gram_diff', _h(X), kd, _dt(X), S, N, N2, Q, A, _p(X), _ss(X), _p(X2), _ss(X2), _p(p0), _ss(p0), _p(p1), _ss(p1),
              _p(p2), _ss(p2), int(bool(ard)), _p(diag_add), _ss(diag_add), float(jitter),
              _p(out), out.stride(-2), out.stride(0) if out.dim() == 3 else 0, _stream())
    return out


def gram_diff_bwd(kind, X, X2, p0, p1, p2, ard, dK, need=('X', 'X2', 'p0', 'p1', 'p2')):
    """Reverse mode of gram_diff(); returns (dX, dX2, dp0, dp1, dp2) shaped like their primals (summed over S for broadcast operands),
    None for what `need` leaves out."""
    kd, (X, X2, p0, p1, p2), A = _diff_operands('gram_diff_bwd', kind, ard, X, X2, p0, p1, p2, dK)
    dK = _c(dK)
    S = dK.shape[0]
    N, Q = X.shape[-2], X.shape[-1]
    N2 = N if X2 is None else X2.shape[-2]
    dX = torch.zeros_like(X) if 'X' in need else None
    dX2 = torch.zeros_like(X2) if (X2 is not None and 'X2' in need) else None
    dp0, dp1, dp2 = [torch.zeros_like(t) if n in need else None for n, t in (('p0', p0), ('p1', p1), ('p2', p2))]
    if N == 0 or N2 == 0:
        return dX, dX2, dp0, dp1, dp2
    _lib.call('mxf_gram_diff_bwd', _h(X), kd, _dt(X), S, N, N2, Q, A, _p(X), _ss(X), _p(X2), _ss(X2), _p(p0), _ss(p0), _p(p1), _ss(p1),
              _p(p2), _ss(p2), int(bool(ard)), _p(dK), dK.stride(-2), dK.stride(0), _p(dX), _p(dX2), _p(dp0), _p(dp1), _p(dp2), _stream())
    return dX, dX2, dp0, dp1, dp2


def _icm_operands(what, kind, ard, X, X2, idx, idx2, ls, var, B, *others):
    """(kind code, operands, T) of the fused coregionalisation pass: X (S|1, N, Q), X2 (S|1, N2, Q) or None, idx (N,) and idx2 (N2,) int32
    (idx2 None on the square Gram), lengthscale (S|1, Q|1), variance (S|1, 1), B (S|1, T, T).  The limits (Q <= 16, T <= ICM_MAX_T) are
    the entry point's to refuse."""
    _same_kind(what, X, X2, ls, var, B, *others)
    kd = KIND[kind] if isinstance(kind, str) else kind
    N2 = X.shape[-2] if X2 is None else X2.shape[-2]
    if B.dim() != 3 or B.shape[-1] != B.shape[-2]:
        raise ValueError('%s: B must be (S|1, T, T); got %s' % (what, tuple(B.shape)))
    want = (X.shape[-1] if ard else 1, 1)
    if (ls.shape[-1], var.shape[-1]) != want:
        raise ValueError('%s: lengthscale and variance of extents %s (ard = %s, Q = %d); got %s, %s'
                         % (what, want, bool(ard), X.shape[-1], tuple(ls.shape), tuple(var.shape)))
    for name, t, n in (('idx', idx, X.shape[-2]), ('idx2', idx2, N2)):
        if t is None and (name == 'idx' or X2 is not None):
            raise ValueError('%s: %s is missing' % (what, name))
        if t is not None and (t.dtype != torch.int32 or t.device != X.device or tuple(t.shape) != (n,)):
            raise TypeError('%s: %s must be an int32 tensor of shape (%d,) on %s; got %s %s on %s' % (what, name, n, X.device, t.dtype, tuple(t.shape), t.device))
    return kd, [_c(t) for t in (X, X2, idx, None if X2 is None else idx2, ls, var, B)], B.shape[-1]


def _rows_fit(t):
    """a matrix operand the kernels read with a row stride: unit column stride, rows that do not overlap"""
    return t.dim() == 3 and t.stride(-1) == 1 and t.stride(-2) >= t.shape[-1]


def gram_icm(kind, X, X2, idx, idx2, ls, var, ard, B, diag_add=None, jitter=0.0, out=None):
    """K[s, i, j] = k(x_i, x2_j) B[s|0, idx[i], idx2[j]] (S, N, N2) in one pass (mxf_gram_icm): a stationary `kind` times a
    coregionalisation matrix, operands as _icm_operands lists them; diag_add (S|1, 1) and jitter go on the diagonal of a square Gram (X2
    None).  `out` may be a view with a row stride above N2."""
    kd, (X, X2, idx, idx2, ls, var, B), T = _icm_operands('gram_icm', kind, ard, X, X2, idx, idx2, ls, var, B, diag_add, out)
    diag_add = _c(diag_add)
    S = num_samples(X, X2, ls, var, B, diag_add)
    N, Q = X.shape[-2], X.shape[-1]
    N2 = N if X2 is None else X2.shape[-2]
    if out is None:
        out = torch.empty((S, N, N2), dtype=X.dtype, device=X.device)
    elif tuple(out.shape) != (S, N, N2) or not _rows_fit(out):
        raise ValueError('gram_icm: out must be (%d, %d, %d) with a unit column stride; got %s, strides %s' % (S, N, N2, tuple(out.shape), out.stride()))
    if N == 0 or N2 == 0:
        return out
    _lib.call('mxf_gram_icm', _h(X), kd, _dt(X), S, N, N2, Q, T, _p(X), _ss(X), _p(X2), _ss(X2), _p(idx), _p(idx2),
              _p(ls), int(bool(ard)), _ss(ls), _p(var), _ss(var), _p(B), _ss(B), _p(diag_add), _ss(diag_add), float(jitter),
              _p(out), out.stride(-2), out.stride(0), _stream())
    return out


def gram_icm_bwd(kind, X, X2, idx, idx2, ls, var, ard, B, dK, need=('X', 'X2', 'ls', 'var', 'B')):
    """Reverse mode of gram_icm(); returns (dX, dX2, dls, dvar, dB) shaped like their primals (summed over S for broadcast operands), None
    for what `need` leaves out.  dK (S, N, N2) may have a row stride above N2."""
    kd, (X, X2, idx, idx2, ls, var, B), T = _icm_operands('gram_icm_bwd', kind, ard, X, X2, idx, idx2, ls, var, B, dK)
    if not _rows_fit(dK):
        dK = dK.contiguous()
    S = dK.shape[0]
    N, Q = X.shape[-2], X.shape[-1]
    N2 = N if X2 is None else X2.shape[-2]
    if tuple(dK.shape) != (S, N, N2) or S < num_samples(X, X2, ls, var, B):
        raise ValueError('gram_icm_bwd: dK must be (S, %d, %d) with S the operands\' sample count; got %s' % (N, N2, tuple(dK.shape)))
    dX = torch.zeros_like(X) if 'X' in need else None
    dX2 = torch.zeros_like(X2) if (X2 is not None and 'X2' in need) else None
    dls, dvar, dB = [torch.zeros_like(t) if n in need else None for n, t in (('ls', ls), ('var', var), ('B', B))]
    if N == 0 or N2 == 0:
        return dX, dX2, dls, dvar, dB
    _lib.call('mxf_gram_icm_bwd', _h(X), kd, _dt(X), S, N, N2, Q, T, _p(X), _ss(X), _p(X2), _ss(X2), _p(idx), _p(idx2),
              _p(ls), int(bool(ard)), _ss(ls), _p(var), _ss(var), _p(B), _ss(B), _p(dK), dK.stride(-2), dK.stride(0),
              _p(dX), _p(dX2), _p(dls), _p(dvar), _p(dB), _stream())
    return dX, dX2, dls, dvar, dB


def potrf_(A, info=None):
    """in-place batched lower Cholesky of A (S,n,n); returns (A, info) with info an int32 device tensor."""
    S, n = A.shape[0], A.shape[-1]
    if info is None:
        info = torch.zeros(S, dtype=torch.int32, device=A.device)
    _lib.call('mxf_potrf', _h(A), _dt(A), S, n, _p(A), A.stride(-2), A.stride(0), _p(info), _stream())
    return A, info


def merge_info(*infos):
    """Combine LAPACK-style info words of several factorisations WITHOUT masking: a negative word (an internal failure of the library, e.g.
    a lost workgroup hand-off of the tile Cholesky) wins over everything, otherwise the largest positive one (first non-positive-definite
    leading minor); 0 only if all are 0.  (A plain sum turns -1 + 1 into "fine".)"""
    st = torch.stack(torch.broadcast_tensors(*[i.reshape(-1) for i in infos]))      # (one word per sample, or one for all of them)
    lo, hi = st.min(0).values, st.max(0).values
    return torch.where(lo < 0, lo, hi)


def check_info(info, what='potrf'):
    """Host sync + raise on a non-positive-definite matrix (MXNet raises lazily at the next blocking read); a NEGATIVE word is an internal
    failure of the factorisation kernels and always an error."""
    bad = info.nonzero()
    if bad.numel():
        s = int(bad[0, 0])
        v = int(info.reshape(-1)[s])
        if v < 0:
            raise _lib.MXFError('%s: internal failure of the factorisation of sample %d (info %d: a workgroup hand-off was lost)' % (what, s, v))
        raise _lib.MXFError('%s: matrix of sample %d is not positive definite (leading minor %d)' % (what, s, v))


def trsm_(L, B, transpose=False):
    """B <- op(L)^-1 B in place; L (S|1,n,n) lower, B (S,n,nrhs)."""
    L = _c(L)
    S, n, nrhs = B.shape[0], B.shape[-2], B.shape[-1]
    _lib.call('mxf_trsm', _h(B), _dt(B), int(bool(transpose)), S, n, nrhs, _p(L), L.stride(-2), _ss(L), _p(B), B.stride(-2),
              B.stride(0), _stream())
    return B


def trtri(L):
    L = _c(L)
    S, n = L.shape[0], L.shape[-1]
    out = torch.empty_like(L)
    _lib.call('mxf_trtri', _h(L), _dt(L), S, n, _p(L), L.stride(-2), L.stride(0), _p(out), out.stride(-2), out.stride(0), _stream())
    return out


def sumlogdiag(L):
    L = _c(L)
    S, n = L.shape[0], L.shape[-1]
    out = torch.empty(S, dtype=L.dtype, device=L.device)
    _lib.call('mxf_sumlogdiag', _h(L), _dt(L), S, n, _p(L), L.stride(-2), L.stride(0), _p(out), _stream())
    return out


def make_diagonal(a):
    """(..., n) -> (..., n, n) diagonal embed (mxf_make_diagonal)."""
    a = _c(a)
    n = a.shape[-1]
    batch = a.numel() // n if n else 0
    out = torch.empty(tuple(a.shape) + (n,), dtype=a.dtype, device=a.device)
    _lib.call('mxf_make_diagonal', _h(a), _dt(a), batch, n, _p(a), _p(out), _stream())
    return out


def diag_of(g):
    """(..., n, n) -> (..., n) diagonal (mxf_diag_of)."""
    g = _c(g)
    n = g.shape[-1]
    batch = g.numel() // (n * n) if n else 0
    out = torch.empty(tuple(g.shape[:-1]), dtype=g.dtype, device=g.device)
    _lib.call('mxf_diag_of', _h(g), _dt(g), batch, n, _p(g), _p(out), _stream())
    return out


def softplus(x):
    x = _c(x)
    y = torch.empty_like(x)
    _lib.call('mxf_softplus_fwd', _h(x), _dt(x), x.numel(), _p(x), _p(y), _stream())
    return y


def softplus_bwd_(x, dy, dx_acc):
    _lib.call('mxf_softplus_bwd', _h(x), _dt(x), x.numel(), _p(_c(x)), _p(_c(dy)), _p(dx_acc), _stream())
    return dx_acc


def normal_reparam(mean, var, eps):
    """x[s] = mean + eps[s]*sqrt(var); mean/var (n...), eps (S, n...)."""
    mean, var, eps = _c(mean), _c(var), _c(eps)
    x = torch.empty_like(eps)
    _lib.call('mxf_normal_reparam', _h(eps), _dt(eps), eps.shape[0], mean.numel(), _p(mean), _p(var), _p(eps), _p(x), _stream())
    return x


def normal_reparam_bwd_(var, eps, dx, dmean_acc, dvar_acc):
    _lib.call('mxf_normal_reparam_bwd', _h(eps), _dt(eps), eps.shape[0], var.numel(), _p(_c(var)), _p(_c(eps)), _p(_c(dx)),
              _p(dmean_acc), _p(dvar_acc), _stream())


def normal_reparam_prec(mean, precision, eps):
    """x[s] = mean + eps[s] / sqrt(precision); mean/precision (n...), eps (S, n...)  (mxf_normal_reparam_prec)."""
    _same_kind('normal_reparam_prec', eps, mean, precision)
    mean, precision, eps = _c(mean), _c(precision), _c(eps)
    n = eps.numel() // eps.shape[0] if eps.shape[0] else 0
    if mean.numel() != n or precision.numel() != n:
        raise ValueError('normal_reparam_prec: mean and precision have the %d elements of one sample of eps; got %d and %d'
                         % (n, mean.numel(), precision.numel()))
    x = torch.empty_like(eps)
    _lib.call('mxf_normal_reparam_prec', _h(eps), _dt(eps), eps.shape[0], n, _p(mean), _p(precision), _p(eps), _p(x), _stream())
    return x


def normal_reparam_prec_bwd_(precision, eps, dx, dmean_acc, dprecision_acc):
    """Reverse mode of normal_reparam_prec, added into the (n,) buffers; either may be None (mxf_normal_reparam_prec_bwd)."""
    _same_kind('normal_reparam_prec', eps, precision, dx, dmean_acc, dprecision_acc)
    n = precision.numel()
    if eps.numel() != eps.shape[0] * n or dx.numel() != eps.numel():
        raise ValueError('normal_reparam_prec: eps and dx are (S, n) for a precision of n = %d elements' % n)
    _check_buffers('normal_reparam_prec', (dmean_acc, (n,)), (dprecision_acc, (n,)))
    _lib.call('mxf_normal_reparam_prec_bwd', _h(eps), _dt(eps), eps.shape[0], n, _p(_c(precision)), _p(_c(eps)), _p(_c(dx)),
              _p(dmean_acc), _p(dprecision_acc), _stream())


TR_KIND = {'softplus': _lib.TR_SOFTPLUS, 'logistic': _lib.TR_LOGISTIC}


def _transform_table(what, segments, x, *others):
    """the host arrays of a segment table; segments: (kind, size, p0, p1) per segment of the flat x, one after the other"""
    _same_kind(what, x, *others, contiguous=True)
    n = len(segments)
    kinds = (_lib._c.c_int * n)(*[TR_KIND[k] if isinstance(k, str) else int(k) for k, _, _, _ in segments])
    sizes = (_lib._c.c_int64 * n)(*[int(s) for _, s, _, _ in segments])
    if min(sizes, default=0) < 0 or sum(sizes) != x.numel() or any(t.numel() != x.numel() for t in others):
        raise ValueError('%s: the segment sizes must add up to the %d elements of every buffer' % (what, x.numel()))
    return n, kinds, sizes, (_lib._c.c_double * n)(*[float(p) for _, _, p, _ in segments]), \
        (_lib._c.c_double * n)(*[float(p) for _, _, _, p in segments])


def transform(segments, x):
    """y, shaped like the contiguous x: segment k of the flat x mapped by its kind -- 'softplus' (p0 the offset) or 'logistic' (p0 the lower
    bound, p1 = upper - lower); segments: (kind, size, p0, p1) each.  One launch per _lib.TR_MAX_SEG segments (mxf_transform_fwd)."""
    y = torch.empty_like(x)
    _lib.call('mxf_transform_fwd', _h(x), _dt(x), *_transform_table('transform', segments, x, y), _p(x), _p(y), _stream())
    return y


def transform_bwd_(segments, x, dy, dx_acc):
    """dx_acc += dy * (d transform / d x), segment by segment (mxf_transform_bwd)."""
    _lib.call('mxf_transform_bwd', _h(x), _dt(x), *_transform_table('transform', segments, x, dy, dx_acc), _p(x), _p(dy), _p(dx_acc),
              _stream())
    return dx_acc


def normal_logpdf_(x, mean, var, scale, out_acc, dx_acc=None, dmean_acc=None, dvar_acc=None):
    """out_acc += scale * sum_{s,i} log N(x[s,i]|mean[i],var[i]) (+ reverse mode into the *_acc buffers)."""
    x, mean, var = _c(x), _c(mean), _c(var)
    S = x.shape[0]
    n = x.numel() // S
    _lib.call('mxf_normal_logpdf', _h(x), _dt(x), S, n, _p(x), _p(mean), mean.numel(), _p(var), var.numel(), float(scale),
              _p(out_acc), _p(dx_acc), _p(dmean_acc), _p(dvar_acc), _stream())
    return out_acc


D_KIND = {'gamma': _lib.D_GAMMA, 'gamma_mv': _lib.D_GAMMA_MV, 'beta': _lib.D_BETA, 'laplace': _lib.D_LAPLACE, 'uniform': _lib.D_UNIFORM,
          'bernoulli': _lib.D_BERNOULLI, 'normal_prec': _lib.D_NORMAL_PREC}


def _uni_param(p, S, n):
    """(number of elements per sample, sample stride) of a parameter: 1 or n elements without a sample axis, or (S, n) with one"""
    if p.numel() in (1, n):
        return p.numel(), 0
    if p.numel() == S * n:
        return n, n
    raise ValueError('univariate log-pdf: a parameter has 1, n or S*n elements (n = %d, S = %d), got %d' % (n, S, p.numel()))


def univariate_logpdf_(kind, x, a, b, scale, out_acc, dx_acc=None, da_acc=None, db_acc=None):
    """out_acc += scale * sum_{s,i} log p(x[s,i] | a[i], b[i]) for kind in D_KIND (+ reverse mode into the *_acc buffers); x (S, n...),
    a and b of 1 or n elements (mxf_univariate_logpdf)."""
    _same_kind('univariate log-pdf', x, a, b, out_acc, dx_acc, da_acc, db_acc, contiguous=True)
    S = x.shape[0]
    n = x.numel() // S
    _lib.call('mxf_univariate_logpdf', _h(x), D_KIND[kind] if isinstance(kind, str) else kind, _dt(x), S, n, _p(x), _p(a), a.numel(),
              _p(b), b.numel(), float(scale), _p(out_acc), _p(dx_acc), _p(da_acc), _p(db_acc), _stream())
    return out_acc


def univariate_logpdf_elem(kind, x, a, b, scale=1.0):
    """scale * log p(x[s,i] | a, b), shaped like x (S, n...); a and b of 1 or n elements, or S*n (a sample axis of their own)
    (mxf_univariate_logpdf_elem)."""
    _same_kind('univariate log-pdf', x, a, b, contiguous=True)
    S = x.shape[0]
    n = x.numel() // S
    (n_a, ss_a), (n_b, ss_b) = _uni_param(a, S, n), _uni_param(b, S, n)
    out = torch.empty_like(x)
    _lib.call('mxf_univariate_logpdf_elem', _h(x), D_KIND[kind] if isinstance(kind, str) else kind, _dt(x), S, n, _p(x), _p(a), n_a, ss_a,
              _p(b), n_b, ss_b, float(scale), _p(out), _stream())
    return out


def univariate_logpdf_bwd_(kind, x, a, b, cot, scale, dx_acc=None, da_acc=None, db_acc=None):
    """Reverse mode of univariate_logpdf_elem: dx_acc (S, n...), da_acc, db_acc (shaped like a, b) += scale * cot * d log p / d(.)
    (mxf_univariate_logpdf_bwd)."""
    _same_kind('univariate log-pdf', x, a, b, cot, dx_acc, da_acc, db_acc, contiguous=True)
    S = x.shape[0]
    n = x.numel() // S
    (n_a, ss_a), (n_b, ss_b) = _uni_param(a, S, n), _uni_param(b, S, n)
    _lib.call('mxf_univariate_logpdf_bwd', _h(x), D_KIND[kind] if isinstance(kind, str) else kind, _dt(x), S, n, _p(x), _p(a), n_a, ss_a,
              _p(b), n_b, ss_b, _p(cot), float(scale), _p(dx_acc), _p(da_acc), _p(db_acc), _stream())


def _ps_operands(what, kind, x, a, b, *buffers):
    """(entry-point prefix, leading arguments, S, n, parameter layouts) of the per-sample log-pdfs: kind 'normal' or a key of D_KIND"""
    _same_kind(what, x, a, b, *buffers, contiguous=True)
    S = x.shape[0]
    n = x.numel() // S
    lead = (_h(x),) if kind == 'normal' else (_h(x), D_KIND[kind] if isinstance(kind, str) else kind)
    return ('mxf_normal_logpdf_ps' if kind == 'normal' else 'mxf_univariate_logpdf_ps'), lead + (_dt(x), S, n), S, _uni_param(a, S, n), \
        _uni_param(b, S, n)


def logpdf_per_sample_(kind, x, a, b, scale, out_acc):
    """out_acc[s] += scale * sum_i log p(x[s,i] | a, b): kind 'normal' (a the mean, b the variance: mxf_normal_logpdf_ps) or a key of D_KIND
    (mxf_univariate_logpdf_ps); x (S, n...), a and b of 1 or n elements, or S*n (a sample axis of their own); out_acc (S,)."""
    name, lead, S, (n_a, ss_a), (n_b, ss_b) = _ps_operands('per-sample log-pdf', kind, x, a, b, out_acc)
    _check_buffers('per-sample log-pdf', (out_acc, (S,)))
    _lib.call(name, *lead, _p(x), _p(a), n_a, ss_a, _p(b), n_b, ss_b, float(scale), _p(out_acc), _stream())
    return out_acc


def logpdf_per_sample_bwd_(kind, x, a, b, w, scale, dx_acc=None, da_acc=None, db_acc=None):
    """Reverse mode of logpdf_per_sample_ with the per-sample weights w (S,): dx_acc (S, n...), da_acc, db_acc (shaped like a, b) +=
    scale * w[s] * d log p / d(.)  (mxf_normal_logpdf_ps_bwd / mxf_univariate_logpdf_ps_bwd)."""
    name, lead, S, (n_a, ss_a), (n_b, ss_b) = _ps_operands('per-sample log-pdf', kind, x, a, b, w, dx_acc, da_acc, db_acc)
    _check_buffers('per-sample log-pdf', (w, (S,)), (dx_acc, x.shape), (da_acc, a.shape), (db_acc, b.shape))
    _lib.call(name + '_bwd', *lead, _p(x), _p(a), n_a, ss_a, _p(b), n_b, ss_b, _p(w), float(scale), _p(dx_acc), _p(da_acc), _p(db_acc),
              _stream())


LIK_KIND = {'bernoulli_logit': _lib.LIK_BERNOULLI_LOGIT, 'bernoulli_probit': _lib.LIK_BERNOULLI_PROBIT, 'poisson_exp': _lib.LIK_POISSON_EXP}
_lik_rules = {}


def lik_nodes(num_nodes):
    """(nq, nodes, weights): the Gauss-Hermite rule of numpy.polynomial.hermite.hermgauss as host arrays of doubles, kept per order"""
    nq = int(num_nodes)
    if not 1 <= nq <= _lib.LIK_MAX_NODES:
        raise ValueError('likelihood expectation: 1 <= num_nodes <= %d, got %d' % (_lib.LIK_MAX_NODES, nq))
    if nq not in _lik_rules:
        import numpy as np
        x, w = np.polynomial.hermite.hermgauss(nq)
        _lik_rules[nq] = (nq, (_lib._c.c_double * nq)(*x), (_lib._c.c_double * nq)(*w))
    return _lik_rules[nq]


def _lik_operands(what, y, m, v, *buffers):
    """(S, n, P, [(pointer, sample stride) of y, m, v]) of the likelihood expectations: m (S|1, n, P), v (S|1, n), y like m or None"""
    _same_kind(what, m, v, y, *buffers, contiguous=True)
    if m.dim() != 3 or v.dim() != 2 or v.shape[1] != m.shape[1] or (y is not None and (y.dim() != 3 or y.shape[1:] != m.shape[1:])):
        raise ValueError('%s: y and m are (S|1, n, P) and v is (S|1, n); got %s, %s, %s'
                         % (what, None if y is None else tuple(y.shape), tuple(m.shape), tuple(v.shape)))
    S = num_samples(y, m, v)
    if any(t is not None and t.shape[0] not in (1, S) for t in (y, m, v)):
        raise ValueError('%s: the sample axes must be 1 or %d' % (what, S))
    n, P = int(m.shape[1]), int(m.shape[2])
    return S, n, P, [a for t in (y, m, v) if t is not None for a in (_p(t), 0 if t.shape[0] == 1 else t.stride(0))]


def _lik_kind(kind):
    return LIK_KIND[kind] if isinstance(kind, str) else int(kind)


def lik_expect_(kind, y, m, v, scale, out_acc, dm_acc=None, dv_acc=None, cot=None, num_nodes=20):
    """out_acc[s] += scale * sum_{i,p} E_{N(f; m[s,i,p], v[s,i])}[log p(y[s,i,p] | f)] for kind in LIK_KIND by Gauss-Hermite quadrature, and the
    reverse mode in the same pass: dm_acc (S, n, P) += w sum_k w_k g'(f_k), dv_acc (S, n) += w / 2 sum_p sum_k w_k g''(f_k) with w = scale, or
    scale * cot[s] given per-sample weights cot (S,).  y, m (S|1, n, P), v (S|1, n); the gradient buffers always carry the sample axis
    (mxf_lik_expect)."""
    S, n, P, strided = _lik_operands('likelihood expectation', y, m, v, out_acc, dm_acc, dv_acc, cot)
    _check_buffers('likelihood expectation', (out_acc, (S,)), (cot, (S,)), (dm_acc, (S, n, P)), (dv_acc, (S, n)))
    _lib.call('mxf_lik_expect', _h(m), _lik_kind(kind), _dt(m), S, n, P, *strided, *lik_nodes(num_nodes), _p(cot), float(scale), _p(out_acc),
              _p(dm_acc), _p(dv_acc), _stream())
    return out_acc


def lik_expect_elem(kind, y, m, v, scale=1.0, num_nodes=20):
    """scale * E_{N(f; m, v)}[log p(y | f)] per element, (S, n, P) (mxf_lik_expect_elem)."""
    S, n, P, strided = _lik_operands('likelihood expectation', y, m, v)
    out = torch.empty((S, n, P), dtype=m.dtype, device=m.device)
    _lib.call('mxf_lik_expect_elem', _h(m), _lik_kind(kind), _dt(m), S, n, P, *strided, *lik_nodes(num_nodes), float(scale), _p(out), _stream())
    return out


def lik_moments(kind, m, v, num_nodes=20):
    """(E[mu(f)], E[mu(f)^2]) under N(f; m, v) per element, each (S, n, P), mu(f) = E[y | f] the inverse link (mxf_lik_moments)."""
    S, n, P, strided = _lik_operands('likelihood moments', None, m, v)
    e1 = torch.empty((S, n, P), dtype=m.dtype, device=m.device)
    e2 = torch.empty_like(e1)
    _lib.call('mxf_lik_moments', _h(m), _lik_kind(kind), _dt(m), S, n, P, *strided, *lik_nodes(num_nodes), _p(e1), _p(e2), _stream())
    return e1, e2


def _robustmax_operands(what, y, m, v, *buffers):
    """(S, n, C, [(pointer, sample stride) of y, m, v]) of the robust-max likelihood: m (S|1, n, C), v (S|1, n), y (S|1, n, 1) or None"""
    _same_kind(what, m, v, y, *buffers, contiguous=True)
    if m.dim() != 3 or v.dim() != 2 or v.shape[1] != m.shape[1] or (y is not None and (y.dim() != 3 or tuple(y.shape[1:]) != (m.shape[1], 1))):
        raise ValueError('%s: y is (S|1, n, 1), m is (S|1, n, C) and v is (S|1, n); got %s, %s, %s'
                         % (what, None if y is None else tuple(y.shape), tuple(m.shape), tuple(v.shape)))
    S = num_samples(y, m, v)
    if any(t is not None and t.shape[0] not in (1, S) for t in (y, m, v)):
        raise ValueError('%s: the sample axes must be 1 or %d' % (what, S))
    n, C = int(m.shape[1]), int(m.shape[2])
    if not 2 <= C <= _lib.ROBUSTMAX_MAX_C:
        raise ValueError('%s: 2 <= C <= %d classes, got %d' % (what, _lib.ROBUSTMAX_MAX_C, C))
    return S, n, C, [a for t in (y, m, v) if t is not None for a in (_p(t), 0 if t.shape[0] == 1 else t.stride(0))]


def robustmax_expect_(y, m, v, eps, scale, out_acc, dm_acc=None, dv_acc=None, cot=None, num_nodes=20):
    """out_acc[s] += scale * sum_i E[log p(y[s,i] | f)] of the robust-max likelihood -- 1 - eps where the label's latent value is the largest of
    the row's C, eps / (C - 1) otherwise -- under f_c ~ N(m[s,i,c], v[s,i]), by Gauss-Hermite quadrature over the label's value, and the
    reverse mode in the same pass: dm_acc (S, n, C) and dv_acc (S, n) += w times the exact derivatives of the quadrature sum, w = scale, or
    scale * cot[s] given per-sample weights cot (S,).  y (S|1, n, 1) holds integer-valued labels (read clamped to [0, C - 1]), m (S|1, n, C),
    v (S|1, n); the gradient buffers always carry the sample axis (mxf_robustmax_expect)."""
    S, n, C, strided = _robustmax_operands('robust-max expectation', y, m, v, out_acc, dm_acc, dv_acc, cot)
    if not 0.0 < float(eps) < 1.0:
        raise ValueError('robust-max expectation: eps must lie in (0, 1), got %r' % (eps,))
    if out_acc is None:
        raise ValueError('robust-max expectation: out_acc is required')
    _check_buffers('robust-max expectation', (out_acc, (S,)), (cot, (S,)), (dm_acc, (S, n, C)), (dv_acc, (S, n)))
    _lib.call('mxf_robustmax_expect', _h(m), _dt(m), S, n, C, *strided, *lik_nodes(num_nodes), float(eps), _p(cot), float(scale), _p(out_acc),
              _p(dm_acc), _p(dv_acc), _stream())
    return out_acc


def robustmax_probs(m, v, num_nodes=20):
    """probs[s,i,c] = P(f_c is the largest of the row) under f_c ~ N(m[s,i,c], v[s,i]), (S, n, C); not renormalised: the sum over c differs
    from 1 by the error of the quadrature rule (mxf_robustmax_probs)."""
    S, n, C, strided = _robustmax_operands('robust-max probabilities', None, m, v)
    probs = torch.empty((S, n, C), dtype=m.dtype, device=m.device)
    _lib.call('mxf_robustmax_probs', _h(m), _dt(m), S, n, C, *strided, *lik_nodes(num_nodes), _p(probs), _stream())
    return probs


def _psi_operands(what, mu, s, Z, lengthscale, variance, ard, *buffers):
    """(S, N, M, Q, [pointer, sample stride of mu, s, Z], [lengthscale, ard, stride], [variance, stride]) of the RBF psi statistics:
    mu, s (S|1, N, Q), Z (S|1, M, Q), lengthscale (S|1, Q with ard else 1), variance (S|1, 1)"""
    _same_kind(what, mu, s, Z, lengthscale, variance, *buffers, contiguous=True)
    if mu.dim() != 3 or s.shape[1:] != mu.shape[1:] or s.dim() != 3 or Z.dim() != 3 or Z.shape[2] != mu.shape[2]:
        raise ValueError('%s: mu and s are (S|1, N, Q) and Z is (S|1, M, Q); got %s, %s, %s' % (what, tuple(mu.shape), tuple(s.shape), tuple(Z.shape)))
    N, M, Q = int(mu.shape[1]), int(Z.shape[1]), int(mu.shape[2])
    if lengthscale.dim() != 2 or lengthscale.shape[1] != (Q if ard else 1) or variance.dim() != 2 or variance.shape[1] != 1:
        raise ValueError('%s: lengthscale is (S|1, %d) and variance (S|1, 1); got %s, %s'
                         % (what, Q if ard else 1, tuple(lengthscale.shape), tuple(variance.shape)))
    ops_ = (mu, s, Z, lengthscale, variance)
    S = num_samples(*ops_)
    if any(t.shape[0] not in (1, S) for t in ops_):
        raise ValueError('%s: the sample axes must be 1 or %d' % (what, S))
    st = lambda t: [_p(t), 0 if t.shape[0] == 1 else t.stride(0)]
    return S, N, M, Q, st(mu) + st(s) + st(Z), [_p(lengthscale), int(bool(ard)), st(lengthscale)[1]], st(variance)


def psi_rbf(mu, s, Z, lengthscale, variance, ard, want_psi1=True, want_psi2=True):
    """(Psi1 (S, M, N), Psi2 (S, M, M)) of the RBF kernel under x_n ~ N(mu_n, diag(s_n)), s >= 0; None for the one not wanted
    (mxf_psi_rbf_fwd).  Psi2 is bitwise symmetric."""
    S, N, M, Q, big, ls, var = _psi_operands('psi statistics', mu, s, Z, lengthscale, variance, ard)
    Psi1 = torch.empty((S, M, N), dtype=mu.dtype, device=mu.device) if want_psi1 else None
    Psi2 = torch.empty((S, M, M), dtype=mu.dtype, device=mu.device) if want_psi2 else None
    _lib.call('mxf_psi_rbf_fwd', _h(mu), _dt(mu), S, N, M, Q, *big, *ls, *var, _p(Psi1), _p(Psi2), _stream())
    return Psi1, Psi2


def psi_rbf_bwd_(mu, s, Z, lengthscale, variance, ard, G1, G2, dmu_acc=None, ds_acc=None, dZ_acc=None, dls_acc=None, dvar_acc=None):
    """The reverse mode of psi_rbf: the cotangents G1 (S, M, N) and G2 (S, M, M, need not be symmetric), either None, ACCUMULATED into
    buffers shaped like the operands, a shared sample axis at extent 1 and summed over (mxf_psi_rbf_bwd)."""
    S, N, M, Q, big, ls, var = _psi_operands('psi statistics', mu, s, Z, lengthscale, variance, ard, G1, G2, dmu_acc, ds_acc, dZ_acc, dls_acc,
                                             dvar_acc)
    _check_buffers('psi statistics', (G1, (S, M, N)), (G2, (S, M, M)), (dmu_acc, mu.shape), (ds_acc, s.shape), (dZ_acc, Z.shape),
                   (dls_acc, lengthscale.shape), (dvar_acc, variance.shape))
    _lib.call('mxf_psi_rbf_bwd', _h(mu), _dt(mu), S, N, M, Q, *big, *ls, *var, _p(G1), _p(G2), _p(dmu_acc), _p(ds_acc), _p(dZ_acc), _p(dls_acc),
              _p(dvar_acc), _stream())


def psi_rbf_quad(mu, s, Z, lengthscale, variance, ard, A):
    """R (S, N, J), R[s, n, j] = sum_{m,m'} A[s, j, m, m'] psi2n[s, n, m, m']: the terms Psi2 sums over n, contracted per row with J weight
    matrices A (S|1, J, M, M) that need not be symmetric (mxf_psi_rbf_quad).  No reverse mode."""
    S, N, M, Q, big, ls, var = _psi_operands('psi statistics', mu, s, Z, lengthscale, variance, ard, A)
    if A.dim() != 4 or A.shape[1] < 1 or tuple(A.shape[2:]) != (M, M):
        raise ValueError('psi statistics: A is (S|1, J, %d, %d) with J >= 1; got %s' % (M, M, tuple(A.shape)))
    if S > 1 and A.shape[0] not in (1, S):
        raise ValueError('psi statistics: the sample axes must be 1 or %d' % S)
    S, J = max(S, int(A.shape[0])), int(A.shape[1])
    R = torch.empty((S, N, J), dtype=mu.dtype, device=mu.device)
    _lib.call('mxf_psi_rbf_quad', _h(mu), _dt(mu), S, N, M, Q, *big, *ls, *var, J, _p(A), 0 if A.shape[0] == 1 else A.stride(0), _p(R), _stream())
    return R


def _rff_operands(what, X, Omega, phase, W, *buffers):
    """(S, N, D, Q, J, [pointer, sample stride of X, Omega, phase, W]) of the random Fourier features: X (S|1, N, Q), Omega (S|1, D, Q),
    phase (S|1, D), W (S|1, D, J)"""
    _same_kind(what, X, Omega, phase, W, *buffers, contiguous=True)
    if X.dim() != 3 or Omega.dim() != 3 or phase.dim() != 2 or W.dim() != 3 or Omega.shape[2] != X.shape[2] or phase.shape[1] != Omega.shape[1] \
            or W.shape[1] != Omega.shape[1]:
        raise ValueError('%s: X is (S|1, N, Q), Omega (S|1, D, Q), phase (S|1, D) and W (S|1, D, J); got %s, %s, %s, %s'
                         % (what, tuple(X.shape), tuple(Omega.shape), tuple(phase.shape), tuple(W.shape)))
    N, D, Q, J = int(X.shape[1]), int(Omega.shape[1]), int(X.shape[2]), int(W.shape[2])
    if min(N, D, Q, J) < 1:
        raise ValueError('%s: N, D, Q and J must be at least 1; got %d, %d, %d, %d' % (what, N, D, Q, J))
    ops_ = (X, Omega, phase, W)
    S = num_samples(*ops_)
    if any(t.shape[0] not in (1, S) for t in ops_):
        raise ValueError('%s: the sample axes must be 1 or %d' % (what, S))
    args = []
    for t in ops_:
        args += [_p(t), 0 if t.shape[0] == 1 else t.stride(0)]
    return S, N, D, Q, J, args


def rff_eval(X, Omega, phase, W):
    """out (S, N, J), out[s, n, j] = sum_d cos(X[s, n] . Omega[s, d] + phase[s, d]) W[s, d, j]: D random Fourier features of a stationary
    prior draw, each cosine evaluated once for the J columns and none of them stored (mxf_rff_eval)."""
    S, N, D, Q, J, args = _rff_operands('random features', X, Omega, phase, W)
    out = torch.empty((S, N, J), dtype=X.dtype, device=X.device)
    _lib.call('mxf_rff_eval', _h(X), _dt(X), S, N, D, Q, J, *args, _p(out), _stream())
    return out


def rff_eval_bwd_(X, Omega, phase, W, G, dX_acc):
    """The reverse mode of rff_eval in X: the cotangent G (S, N, J), the gradient ACCUMULATED into dX_acc, shaped like X, a shared sample axis
    at extent 1 and summed over (mxf_rff_eval_bwd).  Omega, phase and W have no reverse mode."""
    S, N, D, Q, J, args = _rff_operands('random features', X, Omega, phase, W, G, dX_acc)
    _check_buffers('random features', (G, (S, N, J)), (dX_acc, X.shape))
    _lib.call('mxf_rff_eval_bwd', _h(X), _dt(X), S, N, D, Q, J, *args, _p(G), _p(dX_acc), _stream())


class RFFEval(torch.autograd.Function):
    """rff_eval with its reverse mode in X; the basis and the weights are constants of a drawn sample path."""

    @staticmethod
    def forward(ctx, X, Omega, phase, W):
        ops_ = [t.contiguous() for t in (X, Omega, phase, W)]
        ctx.save_for_backward(*ops_)
        return rff_eval(*ops_)

    @staticmethod
    def backward(ctx, G):
        X = ctx.saved_tensors[0]
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        dX = torch.zeros_like(X)
        rff_eval_bwd_(*ctx.saved_tensors, G.contiguous(), dX)
        return dX, None, None, None


def _kmv_operands(what, kind, X, X2, lengthscale, variance, ard, V, *buffers):
    """(S, N, N2, Q, J, [kind, dtype, S, N, N2, Q, J, X, X2, lengthscale, ard, variance with their sample strides]) of the matrix-free kernel
    product: X (S|1, N, Q), X2 (S|1, N2, Q) or None (square), lengthscale (S|1, Q with ard else 1), variance (S|1, 1), V (S|1, N2, J)"""
    _same_kind(what, X, X2, lengthscale, variance, V, *buffers, contiguous=True)
    kind = KIND[kind] if isinstance(kind, str) else kind
    if kind not in (_lib.K_RBF, _lib.K_MATERN12, _lib.K_MATERN32, _lib.K_MATERN52):
        raise ValueError('%s: stationary kernels only (rbf, matern12, matern32, matern52)' % what)
    if X.dim() != 3 or (X2 is not None and (X2.dim() != 3 or X2.shape[2] != X.shape[2])) or V.dim() != 3:
        raise ValueError('%s: X is (S|1, N, Q), X2 (S|1, N2, Q) or None and V (S|1, N2, J); got %s, %s, %s'
                         % (what, tuple(X.shape), None if X2 is None else tuple(X2.shape), tuple(V.shape)))
    N, Q, J = int(X.shape[1]), int(X.shape[2]), int(V.shape[2])
    N2 = N if X2 is None else int(X2.shape[1])
    if min(N, N2, Q, J) < 1 or V.shape[1] != N2:
        raise ValueError('%s: N, N2, Q and J must be at least 1 and V must have N2 = %d rows; got V %s' % (what, N2, tuple(V.shape)))
    if lengthscale.dim() != 2 or lengthscale.shape[1] != (Q if ard else 1) or variance.dim() != 2 or variance.shape[1] != 1:
        raise ValueError('%s: lengthscale is (S|1, %d) and variance (S|1, 1); got %s, %s'
                         % (what, Q if ard else 1, tuple(lengthscale.shape), tuple(variance.shape)))
    ops_ = [t for t in (X, X2, lengthscale, variance, V) if t is not None]
    S = num_samples(*ops_)
    if any(t.shape[0] not in (1, S) for t in ops_):
        raise ValueError('%s: the sample axes must be 1 or %d' % (what, S))
    st = lambda t: [_p(t), 0 if t is None or t.shape[0] == 1 else t.stride(0)]
    return S, N, N2, Q, J, [kind, _dt(X), S, N, N2, Q, J] + st(X) + st(X2) + st(lengthscale) + [int(bool(ard))] + st(variance)


def kernel_matvec(kind, X, X2, lengthscale, variance, ard, V, diag_add=None):
    """out (S, N, J) = K(X, X2) V (+ diag_add V for the square product, X2 None) without the N x N2 matrix: each covariance evaluated once for
    the J columns and none of them stored (mxf_kmv).  The covariance of a pair is the one gram() writes.  diag_add (S|1, 1)."""
    S, N, N2, Q, J, args = _kmv_operands('kernel product', kind, X, X2, lengthscale, variance, ard, V, diag_add)
    if diag_add is not None:
        if X2 is not None:
            raise ValueError('kernel product: diag_add goes with the square product (X2 None)')
        if diag_add.dim() != 2 or diag_add.shape[1] != 1 or diag_add.shape[0] not in (1, S):
            raise ValueError('kernel product: diag_add is (S|1, 1); got %s' % (tuple(diag_add.shape),))
    out = torch.empty((S, N, J), dtype=X.dtype, device=X.device)
    _lib.call('mxf_kmv', _h(X), *args, _p(diag_add), 0 if diag_add is None or diag_add.shape[0] == 1 else diag_add.stride(0),
              _p(V), 0 if V.shape[0] == 1 else V.stride(0), _p(out), _stream())
    return out


def kernel_matvec_bwd_(kind, X, X2, lengthscale, variance, ard, A, V, w=None, dls_acc=None, dvar_acc=None):
    """The gradient of sum_s sum_j w[j] A[s, :, j]^T K(X[s], X2[s]) V[s, :, j] in lengthscale and variance, ACCUMULATED into buffers shaped like
    them, a shared sample axis at extent 1 and summed over (mxf_kmv_bwd).  A (S|1, N, J), V (S|1, N2, J), w: J numbers (None: ones).  The
    N x N2 cotangent sum_j w[j] A[:, j] V[:, j]^T is never stored.  There is no reverse mode in X or X2."""
    S, N, N2, Q, J, args = _kmv_operands('kernel product', kind, X, X2, lengthscale, variance, ard, V, A, dls_acc, dvar_acc)
    if A.dim() != 3 or tuple(A.shape[1:]) != (N, J) or A.shape[0] not in (1, S):
        raise ValueError('kernel product: A is (S|1, %d, %d); got %s' % (N, J, tuple(A.shape)))
    _check_buffers('kernel product', (dls_acc, lengthscale.shape), (dvar_acc, variance.shape))
    w = [1.0] * J if w is None else [float(x) for x in w]
    if len(w) != J:
        raise ValueError('kernel product: %d weights for J = %d columns' % (len(w), J))
    _lib.call('mxf_kmv_bwd', _h(X), *args, _p(A), 0 if A.shape[0] == 1 else A.stride(0), _p(V), 0 if V.shape[0] == 1 else V.stride(0),
              (_lib._c.c_double * J)(*w), _p(dls_acc), _p(dvar_acc), _stream())


class KernelMatvec(torch.autograd.Function):
    """kernel_matvec, differentiable in V (the product with X and X2 exchanged), lengthscale and variance (kernel_matvec_bwd_); X, X2 and
    diag_add have no reverse mode."""

    @staticmethod
    def forward(ctx, kind, ard, X, X2, ls, var, V, diag_add):
        ops_ = [None if t is None else t.contiguous() for t in (X, X2, ls, var, V, diag_add)]
        ctx.kind, ctx.ard = kind, ard
        ctx.save_for_backward(*ops_)
        X, X2, ls, var, V, diag_add = ops_
        return kernel_matvec(kind, X, X2, ls, var, ard, V, diag_add)

    @staticmethod
    def backward(ctx, G):
        X, X2, ls, var, V, diag_add = ctx.saved_tensors
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3] or ctx.needs_input_grad[7]:
            raise NotImplementedError('the matrix-free kernel product has no reverse mode in X, X2 or diag_add: detach them')
        G = G.contiguous()
        dls = torch.zeros_like(ls) if ctx.needs_input_grad[4] else None
        dvar = torch.zeros_like(var) if ctx.needs_input_grad[5] else None
        if dls is not None or dvar is not None:
            kernel_matvec_bwd_(ctx.kind, X, X2, ls, var, ctx.ard, G, V, None, dls, dvar)
        dV = None
        if ctx.needs_input_grad[6]:         # K(X, X2)^T G = K(X2, X) G (+ diag_add G)
            dV = kernel_matvec(ctx.kind, X if X2 is None else X2, None if X2 is None else X, ls, var, ctx.ard, G, diag_add)
            if V.shape[0] == 1 and dV.shape[0] > 1:
                dV = dV.sum(0, keepdim=True)
        return None, None, None, None, dls, dvar, dV, None


def _nearest_operands(what, X, C):
    """(N, M, Q) of the nearest-centre assignment: X (N, Q) and the centres C (M, Q), no sample axis"""
    _same_kind(what, X, C, contiguous=True)
    if X.dim() != 2 or C.dim() != 2 or C.shape[1] != X.shape[1]:
        raise ValueError('%s: X is (N, Q) and C (M, Q); got %s, %s' % (what, tuple(X.shape), tuple(C.shape)))
    N, M, Q = int(X.shape[0]), int(C.shape[0]), int(X.shape[1])
    if min(N, M, Q) < 1:
        raise ValueError('%s: N, M and Q must be at least 1; got %d, %d, %d' % (what, N, M, Q))
    return N, M, Q


def nearest(X, C, want_d2=True):
    """(idx, d2): idx (N,) int32, idx[n] = argmin_m |X[n] - C[m]|^2 with the smallest index among exact ties, and d2 (N,) that minimum
    (None without want_d2); the N x M distances are never stored (mxf_nearest).  X (N, Q), C (M, Q).  No reverse mode."""
    N, M, Q = _nearest_operands('nearest centre', X, C)
    idx = torch.empty((N,), dtype=torch.int32, device=X.device)
    d2 = torch.empty((N,), dtype=X.dtype, device=X.device) if want_d2 else None
    _lib.call('mxf_nearest', _h(X), _dt(X), N, M, Q, _p(X), _p(C), _p(idx), _p(d2), _stream())
    return idx, d2


def kmeans_step(X, C):
    """(C_new, idx, counts, inertia) of one Lloyd iteration in one call (mxf_kmeans_step): C_new (M, Q) the means of the rows assigned to each
    centre (C[m] itself where none is), idx (N,) int32 the assignment, counts (M,) int64 and inertia, a 0-d float64 device tensor, the sum
    of the squared distances to the assigned centres.  X (N, Q), C (M, Q).  No reverse mode."""
    N, M, Q = _nearest_operands('k-means step', X, C)
    C_new = torch.empty_like(C)
    idx = torch.empty((N,), dtype=torch.int32, device=X.device)
    counts = torch.empty((M,), dtype=torch.int64, device=X.device)
    inertia = torch.empty((), dtype=torch.float64, device=X.device)
    _lib.call('mxf_kmeans_step', _h(X), _dt(X), N, M, Q, _p(X), _p(C), _p(C_new), _p(idx), _p(counts), _p(inertia), _stream())
    return C_new, idx, counts, inertia


def knn(X, C=None, k=1, causal=False, want_d2=True):
    """(idx, d2): idx (N, k) int32, the k nearest rows of C (Nc, Q) for every row of X (N, Q), sorted ascending by (distance, index), and d2
    (N, k) their squared distances (None without want_d2); slots beyond the number of candidates hold -1 and +inf.  causal: the candidates of
    row n are the rows j < n of X itself (C None or X).  The N x Nc distances are never stored (mxf_knn).  No reverse mode."""
    if causal and C is not None and C is not X:
        raise ValueError('k nearest neighbours: a causal search runs within X (C None)')
    C = X if C is None else C
    N, Nc, Q = _nearest_operands('k nearest neighbours', X, C)
    k = int(k)
    if k < 1:
        raise ValueError('k nearest neighbours: k must be at least 1; got %d' % k)
    idx = torch.empty((N, k), dtype=torch.int32, device=X.device)
    d2 = torch.empty((N, k), dtype=X.dtype, device=X.device) if want_d2 else None
    _lib.call('mxf_knn', _h(X), _dt(X), N, Nc, Q, k, int(bool(causal)), _p(X), _p(C), _p(idx), _p(d2), _stream())
    return idx, d2


def _vecchia_operands(what, kind, X, Y, nbr, lengthscale, variance, noise, ard, rows, *others):
    """(N, Q, P, k, [kind, dtype], [X, Y, nbr, lengthscale, variance, noise pointers]) of the Vecchia kernels: X (N, Q), Y (N, P), nbr (rows, k)
    int32, lengthscale (Q with ard else 1), variance (1), noise (1); no sample axis"""
    _same_kind(what, X, Y, lengthscale, variance, noise, *others, contiguous=True)
    kind = KIND[kind] if isinstance(kind, str) else kind
    if kind not in (_lib.K_RBF, _lib.K_MATERN12, _lib.K_MATERN32, _lib.K_MATERN52):
        raise ValueError('%s: stationary kernels only (rbf, matern12, matern32, matern52)' % what)
    if X.dim() != 2 or Y.dim() != 2 or Y.shape[0] != X.shape[0] or nbr.dim() != 2:
        raise ValueError('%s: X is (N, Q), Y (N, P) and nbr (rows, k); got %s, %s, %s' % (what, tuple(X.shape), tuple(Y.shape), tuple(nbr.shape)))
    N, Q, P, k = int(X.shape[0]), int(X.shape[1]), int(Y.shape[1]), int(nbr.shape[1])
    if min(N, Q, P, k) < 1 or nbr.shape[0] != rows:
        raise ValueError('%s: N, Q, P and k must be at least 1 and nbr must have %d rows; got nbr %s' % (what, rows, tuple(nbr.shape)))
    if nbr.dtype != torch.int32 or nbr.device != X.device or not nbr.is_contiguous():
        raise TypeError('%s: nbr is a contiguous int32 tensor on the device of X' % what)
    if lengthscale.numel() != (Q if ard else 1) or variance.numel() != 1 or noise.numel() != 1:
        raise ValueError('%s: lengthscale has %d elements, variance and noise one; got %s, %s, %s'
                         % (what, Q if ard else 1, tuple(lengthscale.shape), tuple(variance.shape), tuple(noise.shape)))
    return N, Q, P, k, [kind, _dt(X)], [_p(X), _p(Y), _p(nbr), _p(lengthscale), _p(variance), _p(noise)]


def vecchia_cond(kind, Xt, X, Y, nbr, lengthscale, variance, noise, ard):
    """(mean (Nt, P), var (Nt,)) of the latent function at the rows of Xt (Nt, Q), each conditioned on its neighbours nbr (Nt, k) int32 among
    the rows of X (N, Q) with Y (N, P): kappa^T (K_cc + noise I)^-1 Y_c and variance - kappa^T (K_cc + noise I)^-1 kappa (mxf_vecchia_cond).
    -1 in nbr is an empty slot."""
    if Xt.dim() != 2 or Xt.shape[1] != X.shape[-1] or Xt.shape[0] < 1:
        raise ValueError('Vecchia predictor: Xt is (Nt, Q) with Nt >= 1; got %s' % (tuple(Xt.shape),))
    Nt = int(Xt.shape[0])
    N, Q, P, k, head, ptrs = _vecchia_operands('Vecchia predictor', kind, X, Y, nbr, lengthscale, variance, noise, ard, Nt, Xt)
    mean = torch.empty((Nt, P), dtype=X.dtype, device=X.device)
    var = torch.empty((Nt,), dtype=X.dtype, device=X.device)
    _lib.call('mxf_vecchia_cond', _h(X), *head, Nt, N, Q, P, k, int(bool(ard)), _p(Xt), *ptrs, _p(mean), _p(var), _stream())
    return mean, var


def vecchia_logpdf(kind, X, Y, nbr, lengthscale, variance, noise, ard, want_terms=True):
    """(value, terms): the Vecchia log-likelihood sum_i log N(y_i | y_c(i)) of Y (N, P) at X (N, Q) with the neighbour sets nbr (N, k) int32
    (entries of row i are -1 or < i), a 0-d float64 device tensor, and its N terms (None without want_terms) (mxf_vecchia_logpdf)."""
    N, Q, P, k, head, ptrs = _vecchia_operands('Vecchia log-pdf', kind, X, Y, nbr, lengthscale, variance, noise, ard, X.shape[0])
    terms = torch.empty((N,), dtype=X.dtype, device=X.device) if want_terms else None
    value = torch.empty((), dtype=torch.float64, device=X.device)
    _lib.call('mxf_vecchia_logpdf', _h(X), *head, N, Q, P, k, int(bool(ard)), *ptrs, _p(terms), _p(value), _stream())
    return value, terms


def vecchia_logpdf_bwd(kind, X, Y, nbr, lengthscale, variance, noise, ard, g, want=(True, True, True, True)):
    """(dls, dvar, dnoise, dY) of g * vecchia_logpdf's value, g one element of X's dtype on the device; want: which of the four are formed,
    the others are None (mxf_vecchia_logpdf_bwd).  There is no reverse mode in X."""
    N, Q, P, k, head, ptrs = _vecchia_operands('Vecchia log-pdf', kind, X, Y, nbr, lengthscale, variance, noise, ard, X.shape[0], g)
    if g.numel() != 1:
        raise ValueError('Vecchia log-pdf: g has one element; got %s' % (tuple(g.shape),))
    outs = [torch.empty_like(t) if w else None for t, w in zip((lengthscale, variance, noise, Y), want)]
    _lib.call('mxf_vecchia_logpdf_bwd', _h(X), *head, N, Q, P, k, int(bool(ard)), *ptrs, _p(g), *[_p(t) for t in outs], _stream())
    return tuple(outs)


class VecchiaLogPdf(torch.autograd.Function):
    """vecchia_logpdf's value in X's dtype, shape (1,), differentiable in Y, noise, lengthscale and variance (vecchia_logpdf_bwd, which
    recomputes the factors); the neighbour sets are constants, and X has no reverse mode."""

    @staticmethod
    def forward(ctx, kind, ard, X, Y, nbr, noise, ls, var):
        X, Y, noise, ls, var = [t.detach().contiguous() for t in (X, Y, noise, ls, var)]
        ctx.kind, ctx.ard = kind, ard
        ctx.save_for_backward(X, Y, nbr, noise, ls, var)
        value, _ = vecchia_logpdf(kind, X, Y, nbr, ls, var, noise, ard, want_terms=False)
        return value.to(X.dtype).reshape(1)

    @staticmethod
    def backward(ctx, g):
        X, Y, nbr, noise, ls, var = ctx.saved_tensors
        if ctx.needs_input_grad[2]:
            raise NotImplementedError('the Vecchia log-pdf has no reverse mode in X: detach it')
        need = ctx.needs_input_grad
        dls, dvar, dnoise, dY = vecchia_logpdf_bwd(ctx.kind, X, Y, nbr, ls, var, noise, ctx.ard, g.reshape(1).contiguous(),
                                                   want=(need[6], need[7], need[5], need[3]))
        return None, None, None, dY, None, dnoise, dls, dvar


MVN_MAX_ORDER = 32    # the order up to which the mxf_mvn_* entry points run (MVN_MAX of mvn.hip)


def _mvn_rows(x, mean):
    """x (S|1, B, n) and mean (S|1, B|1, n) as the entry points take them -- rows of n contiguous elements, x at batch stride n -- and their
    strides.  An operand that already has that layout, expanded axes included, is passed as it is."""
    n = x.shape[-1]
    x, ((_, ss_x),) = _shared_axes(x, (0,), lambda t: t.stride(2) == 1 and (t.shape[1] == 1 or t.stride(1) == n))
    mean, ((_, ss_m), (_, sb_m)) = _shared_axes(mean, (0, 1), lambda t: t.stride(2) == 1)
    return x, ss_x, mean, ss_m, sb_m


def mvn_factor(A, form=0):
    """(F, logdet, info) of A (S|1, B|1, n, n), n <= 32 (mxf_mvn_factor): per distinct matrix -- an expanded axis counts as 1 -- the lower
    factor F (S_A, B_A, n, n) of the covariance inverted (form 0) or of the precision itself (form 1), logdet (S_A, B_A) = sum log L_ii and
    the int32 info word (0, or the 1-based index of the first pivot that is not positive)."""
    _same_kind('multivariate normal', A)
    n = A.shape[-1]
    A, ((S_A, ss), (B_A, sb)) = _shared_axes(A, (0, 1), lambda t: t.stride(-1) == 1)
    F = torch.empty((S_A, B_A, n, n), dtype=A.dtype, device=A.device)
    logdet = torch.empty((S_A, B_A), dtype=A.dtype, device=A.device)
    info = torch.zeros((S_A, B_A), dtype=torch.int32, device=A.device)
    _lib.call('mxf_mvn_factor', _h(A), _dt(A), int(form), S_A, B_A, n, _p(A), A.stride(-2), ss, sb, _p(F), _p(logdet), _p(info), _stream())
    return F, logdet, info


def mvn_logpdf(x, mean, F, logdet, form=0, scale=1.0):
    """scale * log N(x[s,b] | mean, A) (S, B) from mvn_factor's F and logdet; x (S|1, B, n), mean (S|1, B|1, n) (mxf_mvn_logpdf)."""
    _same_kind('multivariate normal', x, mean, F, logdet)
    S, B, n = max(x.shape[0], mean.shape[0], F.shape[0]), x.shape[1], x.shape[2]
    x, ss_x, mean, ss_m, sb_m = _mvn_rows(x, mean)
    out = torch.empty((S, B), dtype=x.dtype, device=x.device)
    _lib.call('mxf_mvn_logpdf', _h(x), _dt(x), int(form), S, B, n, _p(x), ss_x, _p(mean), ss_m, sb_m, _p(F), _p(logdet), F.shape[0],
              F.shape[1], float(scale), _p(out), _stream())
    return out


def mvn_logpdf_bwd_(x, mean, F, cot, form=0, scale=1.0, dx_acc=None, dmean_acc=None, dA_acc=None):
    """Reverse mode of mvn_logpdf: dx_acc (S|1, B, n), dmean_acc (S|1, B|1, n), dA_acc (S_A, B_A, n, n) -- dense, shaped like their operands
    with the shared axes at extent 1 -- += the gradients under the cotangent cot (S, B) (mxf_mvn_logpdf_bwd)."""
    _same_kind('multivariate normal', x, mean, F, cot, dx_acc, dmean_acc, dA_acc)
    S, B, n = cot.shape[0], x.shape[1], x.shape[2]
    x, ss_x, mean, ss_m, sb_m = _mvn_rows(x, mean)
    _check_buffers('multivariate normal', (cot, (S, B)), (dx_acc, x.shape), (dmean_acc, mean.shape), (dA_acc, F.shape))
    _lib.call('mxf_mvn_logpdf_bwd', _h(x), _dt(x), int(form), S, B, n, _p(x), ss_x, _p(mean), ss_m, sb_m, _p(F), F.shape[0], F.shape[1],
              _p(cot), float(scale), _p(dx_acc), _p(dmean_acc), _p(dA_acc), _stream())


def _wishart_operands(X, dof, V):
    """X (S|1, B, n, n), dof (S|1, B|1) and V (S|1, B|1, n, n) as the mxf_wishart_* entry points take them, and the arguments that describe
    them: rows of n contiguous elements, X's matrices n rows apart.  An operand that already has that layout, expanded axes included, is
    passed as it is."""
    n = X.shape[-1]
    if X.dim() != 4 or V.dim() != 4 or dof.dim() != 2 or X.shape[-2] != n or tuple(V.shape[-2:]) != (n, n):
        raise ValueError('Wishart: X (S|1, B, n, n), dof (S|1, B|1), V (S|1, B|1, n, n); got %s, %s, %s'
                         % (tuple(X.shape), tuple(dof.shape), tuple(V.shape)))
    rows = lambda t: t.stride(3) == 1 and t.stride(2) >= n
    X, ((S_X, ss_X),) = _shared_axes(X, (0,), lambda t: rows(t) and (t.shape[1] == 1 or t.stride(1) == n * t.stride(2)))
    V, ((S_V, ss_V), (B_V, sb_V)) = _shared_axes(V, (0, 1), rows)
    dof, ((S_d, ss_d), (B_d, sb_d)) = _shared_axes(dof, (0, 1), None)
    S, B = max(S_X, S_d, S_V), X.shape[1]
    if any(e not in (1, S) for e in (S_X, S_d, S_V)) or any(e not in (1, B) for e in (B_d, B_V)):
        raise ValueError('Wishart: operands of %s, %s, %s do not broadcast to (%d, %d) rows' % (tuple(X.shape), tuple(dof.shape), tuple(V.shape), S, B))
    args = (_p(X), X.stride(2), ss_X, _p(dof), ss_d, sb_d, _p(V), V.stride(2), ss_V, sb_V, S_V, B_V)
    return (X, dof, V), S, B, n, args, ((S_X, B, n, n), (S_d, B_d), (S_V, B_V, n, n))


def wishart_logpdf(X, dof, V, scale=1.0):
    """(scale * log W(X[s,b] | V, dof) (S, B), info (S, B) int32) for n <= 32; X (S|1, B, n, n), dof (S|1, B|1), V (S|1, B|1, n, n), an
    expanded axis counting as shared (mxf_wishart_logpdf).  info: 0, j for V's j-th pivot, n + j for X's, 2 n + 1 for dof <= n - 1."""
    _same_kind('Wishart', X, dof, V)
    (X, dof, V), S, B, n, args, _ = _wishart_operands(X, dof, V)          # bound here: `args` holds their addresses, a copy lives until the call
    out = torch.empty((S, B), dtype=X.dtype, device=X.device)
    info = torch.zeros((S, B), dtype=torch.int32, device=X.device)
    _lib.call('mxf_wishart_logpdf', _h(X), _dt(X), S, B, n, *args, float(scale), _p(out), _p(info), _stream())
    return out, info


def wishart_logpdf_bwd_(X, dof, V, cot, scale=1.0, dX_acc=None, ddof_acc=None, dV_acc=None):
    """Reverse mode of wishart_logpdf: dX_acc (S|1, B, n, n), ddof_acc (S|1, B|1), dV_acc (S_V, B_V, n, n) -- dense, shaped like their
    operands with the shared axes at extent 1 -- += the gradients under the cotangent cot (S, B) (mxf_wishart_logpdf_bwd)."""
    _same_kind('Wishart', X, dof, V, cot, dX_acc, ddof_acc, dV_acc)
    (X, dof, V), S, B, n, args, shapes = _wishart_operands(X, dof, V)     # bound here: `args` holds their addresses
    _check_buffers('Wishart', *zip((cot, dX_acc, ddof_acc, dV_acc), ((S, B),) + shapes))
    _lib.call('mxf_wishart_logpdf_bwd', _h(X), _dt(X), S, B, n, *args, _p(cot), float(scale), _p(dX_acc), _p(ddof_acc), _p(dV_acc), _stream())


def _simplex_operand(t, shared_axes):
    """(t, strideS, strideB) of an operand (S|1, B|1, ...) as those entry points take it: dense, the axes it is shared over -- of extent 1,
    or expanded, among shared_axes -- at stride 0 (_shared_axes: passed as it is where it has that layout, never materialised)"""
    t, _ = _shared_axes(t, shared_axes)
    return t, (0 if t.shape[0] == 1 else int(t.stride(0))), (0 if t.shape[1] == 1 else int(t.stride(1)))


def _simplex_operands(what, x, p, labels, cot=None):
    """x (S|1, B, K) (labels: (S|1, B)) and the parameter p (S|1, B|1, K) of a row-wise log-pdf as those entry points take them -- dense,
    the axes they are shared over at stride 0 -- with S, B, K and the strides.  S is the largest sample extent among the operands as they
    are given (an expanded axis counts with its extent) and the cotangent."""
    if p.dim() != 3 or x.dim() != (2 if labels else 3) or (not labels and x.shape[2] != p.shape[2]):
        raise ValueError('%s: x %s and a parameter (S|1, B|1, K); got %s, %s'
                         % (what, '(S|1, B)' if labels else '(S|1, B, K)', tuple(x.shape), tuple(p.shape)))
    B, K = int(x.shape[1]), int(p.shape[2])
    S = max(int(x.shape[0]), int(p.shape[0]), 1 if cot is None else int(cot.shape[0]))
    x, ss_x, _ = _simplex_operand(x, (0,))
    p, ss_p, sb_p = _simplex_operand(p, (0, 1))
    if x.shape[0] not in (1, S) or p.shape[0] not in (1, S) or p.shape[1] not in (1, B):
        raise ValueError('%s: operands of %s, %s do not broadcast to (%d, %d) rows' % (what, tuple(x.shape), tuple(p.shape), S, B))
    return x, ss_x, p, ss_p, sb_p, S, B, K


def categorical_logpdf(logp, x, one_hot=False, normalize=True, scale=1.0):
    """scale * log p(x[s,b] | logp) (S, B): logp (S|1, B|1, K), softmax-normalised along K if `normalize`; x (S|1, B) class indices held in
    logp's dtype (clipped to [0, K - 1]), or with one_hot (S|1, B, K) rows.  An axis of extent 1 or an expanded one is shared
    (mxf_categorical_logpdf)."""
    _same_kind('Categorical', logp, x)
    x, ss_x, logp, ss_p, sb_p, S, B, K = _simplex_operands('Categorical', x, logp, not one_hot)
    out = torch.empty((S, B), dtype=logp.dtype, device=logp.device)
    _lib.call('mxf_categorical_logpdf', _h(logp), _dt(logp), S, B, K, _p(logp), ss_p, sb_p, _p(x), ss_x, int(bool(one_hot)),
              int(bool(normalize)), float(scale), _p(out), _stream())
    return out


def categorical_logpdf_bwd_(logp, x, cot, one_hot=False, normalize=True, scale=1.0, dlogp_acc=None, dx_acc=None):
    """Reverse mode of categorical_logpdf: dlogp_acc (S|1, B|1, K) and, with one_hot only, dx_acc (S|1, B, K) -- dense, shaped like their
    operands with the shared axes at extent 1 -- += the gradients under the cotangent cot (S, B) (mxf_categorical_logpdf_bwd)."""
    _same_kind('Categorical', logp, x, cot, dlogp_acc, dx_acc)
    x, ss_x, logp, ss_p, sb_p, S, B, K = _simplex_operands('Categorical', x, logp, not one_hot, cot)
    _check_buffers('Categorical', (cot, (S, B)), (dlogp_acc, logp.shape), (dx_acc, x.shape))
    _lib.call('mxf_categorical_logpdf_bwd', _h(logp), _dt(logp), S, B, K, _p(logp), ss_p, sb_p, _p(x), ss_x, int(bool(one_hot)),
              int(bool(normalize)), _p(cot), float(scale), _p(dlogp_acc), _p(dx_acc), _stream())


def dirichlet_logpdf(x, alpha, normalize=True, scale=1.0):
    """scale * log Dir(x[s,b] | alpha) (S, B): x (S|1, B, K), divided by its 1-norm along K if `normalize`; alpha (S|1, B|1, K).  An axis of
    extent 1 or an expanded one is shared.  A row with an x_k <= 0 or an alpha_k <= 0 is NaN (mxf_dirichlet_logpdf)."""
    _same_kind('Dirichlet', x, alpha)
    x, ss_x, alpha, ss_a, sb_a, S, B, K = _simplex_operands('Dirichlet', x, alpha, False)
    out = torch.empty((S, B), dtype=x.dtype, device=x.device)
    _lib.call('mxf_dirichlet_logpdf', _h(x), _dt(x), S, B, K, _p(x), ss_x, _p(alpha), ss_a, sb_a, int(bool(normalize)), float(scale),
              _p(out), _stream())
    return out


def dirichlet_logpdf_bwd_(x, alpha, cot, normalize=True, scale=1.0, dx_acc=None, dalpha_acc=None):
    """Reverse mode of dirichlet_logpdf: dx_acc (S|1, B, K), dalpha_acc (S|1, B|1, K) -- dense, shaped like their operands with the shared
    axes at extent 1 -- += the gradients under the cotangent cot (S, B) (mxf_dirichlet_logpdf_bwd)."""
    _same_kind('Dirichlet', x, alpha, cot, dx_acc, dalpha_acc)
    x, ss_x, alpha, ss_a, sb_a, S, B, K = _simplex_operands('Dirichlet', x, alpha, False, cot)
    _check_buffers('Dirichlet', (cot, (S, B)), (dx_acc, x.shape), (dalpha_acc, alpha.shape))
    _lib.call('mxf_dirichlet_logpdf_bwd', _h(x), _dt(x), S, B, K, _p(x), ss_x, _p(alpha), ss_a, sb_a, int(bool(normalize)), _p(cot),
              float(scale), _p(dx_acc), _p(dalpha_acc), _stream())


ACT = {None: _lib.ACT_IDENTITY, 'identity': _lib.ACT_IDENTITY, 'tanh': _lib.ACT_TANH, 'relu': _lib.ACT_RELU, 'sigmoid': _lib.ACT_SIGMOID}


def _dense_act(act):
    return ACT[act] if act is None or isinstance(act, str) else int(act)


def _dense_operands(X, W, b):
    """X (S|1, N, I), W (S|1, O, I), b (S|1, O) or None as the mxf_dense_* entry points take them: rows of X contiguous and ldx apart, W and
    b dense; an expanded sample axis counts as shared and is never materialised."""
    if X.dim() != 3 or W.dim() != 3 or W.shape[2] != X.shape[2] or (b is not None and (b.dim() != 2 or b.shape[1] != W.shape[1])):
        raise ValueError('dense: X (S|1, N, I), W (S|1, O, I), b (S|1, O); got %s, %s, %s'
                         % (tuple(X.shape), tuple(W.shape), None if b is None else tuple(b.shape)))
    N, I = int(X.shape[1]), int(X.shape[2])
    X = _shared_axes(X, (0,), lambda t: t.stride(2) == 1 and (N == 1 or t.stride(1) >= I)
                     and (t.shape[0] == 1 or t.stride(0) >= (N - 1) * t.stride(1) + I))[0]
    W, b = _shared_axes(W, (0,))[0], None if b is None else _shared_axes(b, (0,))[0]
    S = num_samples(X, W, b)
    if any(t is not None and t.shape[0] not in (1, S) for t in (X, W, b)):
        raise ValueError('dense: sample extents %s do not broadcast' % [t.shape[0] for t in (X, W, b) if t is not None])
    return X, W, b, S, N, I, int(W.shape[1]), (X.stride(1) if N > 1 else I)


def _dense_fits(I, O):
    return 1 <= I <= _lib.DENSE_MAX_WIDTH and 1 <= O <= _lib.DENSE_MAX_WIDTH


def _dense_dact(act, Y):
    return {_lib.ACT_IDENTITY: lambda: None, _lib.ACT_TANH: lambda: 1 - Y * Y, _lib.ACT_RELU: lambda: (Y > 0).to(Y.dtype),
            _lib.ACT_SIGMOID: lambda: Y * (1 - Y)}[act]()


def dense(X, W, b=None, act=None):
    """Y[s] = act(X[s] W[s]^T + b[s]) (S, N, O) for all samples in one launch (mxf_dense_fwd): X (S|1, N, I), W (S|1, O, I) in the layout of
    torch.nn.Linear.weight, b (S|1, O) or None, act None / 'identity', 'tanh', 'relu', 'sigmoid'.  Widths beyond the kernel's (128) go
    through gemm and elementwise torch."""
    _same_kind('dense', X, W, b)
    act = _dense_act(act)
    X, W, b, S, N, I, O, ldx = _dense_operands(X, W, b)
    if not _dense_fits(I, O):
        Z = gemm(X, W, transB=True)
        if b is not None:
            Z = Z + b.unsqueeze(1)
        return {_lib.ACT_IDENTITY: lambda z: z, _lib.ACT_TANH: torch.tanh, _lib.ACT_RELU: torch.relu, _lib.ACT_SIGMOID: torch.sigmoid}[act](Z)
    Y = torch.empty((S, N, O), dtype=X.dtype, device=X.device)
    _lib.call('mxf_dense_fwd', _h(X), _dt(X), S, N, I, O, act, _p(X), ldx, _ss(X), _p(W), _ss(W), _p(b), _ss(b), _p(Y), _stream())
    return Y


def dense_bwd_(X, W, Y, dY, act=None, dX_acc=None, dW_acc=None, db_acc=None):
    """Reverse mode of dense from its result Y and the cotangent dY (S, N, O): dX_acc (S|1, N, I), dW_acc (S|1, O, I), db_acc (S|1, O) --
    dense, shaped like their operands with a shared sample axis at extent 1 -- += the gradients (mxf_dense_bwd)."""
    _same_kind('dense', X, W, Y, dY, dX_acc, dW_acc, db_acc)
    act = _dense_act(act)
    X, W, _, S, N, I, O, ldx = _dense_operands(X, W, None)
    S = max(S, int(Y.shape[0]))
    ss_b = 0 if db_acc is None or db_acc.shape[0] == 1 else O          # b itself is not passed: db_acc says whether it is shared
    _check_buffers('dense', (Y, (S, N, O)), (dY, (S, N, O)), (dX_acc, (X.shape[0], N, I)), (dW_acc, W.shape), (db_acc, (S if ss_b else 1, O)))
    if not _dense_fits(I, O):
        d = _dense_dact(act, Y)
        G = dY if d is None else dY * d
        fold = lambda t, acc: acc.add_(t.sum(0, keepdim=True) if acc.shape[0] == 1 and t.shape[0] > 1 else t)
        if dX_acc is not None:
            fold(gemm(G, W), dX_acc)
        if dW_acc is not None:
            fold(gemm(G, X, transA=True), dW_acc)
        if db_acc is not None:
            fold(G.sum(1), db_acc)
        return
    _lib.call('mxf_dense_bwd', _h(X), _dt(X), S, N, I, O, act, _p(X), ldx, _ss(X), _p(W), _ss(W), ss_b, _p(Y), _p(dY),
              _p(dX_acc), _p(dW_acc), _p(db_acc), _stream())


EW_OP = {'add': _lib.EW_ADD, 'subtract': _lib.EW_SUBTRACT, 'multiply': _lib.EW_MULTIPLY, 'divide': _lib.EW_DIVIDE, 'power': _lib.EW_POWER,
         'square': _lib.EW_SQUARE, 'exp': _lib.EW_EXP, 'log': _lib.EW_LOG}
RED_KIND = {'sum': _lib.RED_SUM, 'mean': _lib.RED_MEAN, 'prod': _lib.RED_PROD}

_EW_TORCH = {_lib.EW_ADD: torch.add, _lib.EW_SUBTRACT: torch.sub, _lib.EW_MULTIPLY: torch.mul, _lib.EW_DIVIDE: torch.div, _lib.EW_POWER: torch.pow,
             _lib.EW_SQUARE: torch.square, _lib.EW_EXP: torch.exp, _lib.EW_LOG: torch.log}


def _ew_op(op):
    return EW_OP[op] if isinstance(op, str) else int(op)


def ewise_operands(x, y=None):
    """x (S|1, ...) and y (S|1, ...) or None as the broadcast map takes them, through views alone: of one rank -- the shorter one gets axes of
    extent 1 behind its sample axis, the numpy rule as BroadcastToOperator applies it -- and with every expanded (stride-0) axis back at
    extent 1, so that what came out of broadcast_to is never materialised and its gradient has the shape of what went in."""
    ts = [t for t in (x, y) if t is not None]
    if any(t.dim() < 1 for t in ts):
        raise ValueError('ewise: an operand without a sample axis')
    rank = max(t.dim() for t in ts)
    out = []
    for t in ts:
        if t.dim() < rank:
            t = t.reshape((t.shape[0],) + (1,) * (rank - t.dim()) + tuple(t.shape[1:]))
        out.append(_shared_axes(t, range(rank), None)[0])
    return out[0], (out[1] if y is not None else None)


def _ewise_plan(x, y):
    """(output shape, extents, strides of x, strides of y) of the map over ewise_operands' x and y, the axes of extent 1 dropped and adjacent
    axes merged where both operands traverse them the same way: each dense over the run, or shared over all of it"""
    ts = [x] if y is None else [x, y]
    shape = tuple(max(int(t.shape[d]) for t in ts) for d in range(x.dim()))
    for t in ts:
        if any(t.shape[d] not in (1, shape[d]) for d in range(x.dim())):
            raise ValueError('ewise: operands of %s do not broadcast' % ', '.join(str(tuple(u.shape)) for u in ts))
    axes = []          # [extent, stride of each operand]
    for d, e in enumerate(shape):
        if e == 1:
            continue
        cur = [e] + [0 if t.shape[d] == 1 else int(t.stride(d)) for t in ts]
        if axes and all((p == 0 and c == 0) or (c != 0 and p == c * e) for p, c in zip(axes[-1][1:], cur[1:])):
            axes[-1] = [axes[-1][0] * e] + cur[1:]
        else:
            axes.append(cur)
    if not axes:
        axes = [[1] + [0] * len(ts)]
    return shape, [a[0] for a in axes], [a[1] for a in axes], ([a[2] for a in axes] if y is not None else None)


def _ewise_fits(extent, sx, sy):
    span = lambda s: sum((e - 1) * k for e, k in zip(extent, s))
    n = 1
    for e in extent:
        n *= e
    return len(extent) <= _lib.EW_MAX_RANK and n <= _lib.EW_MAX_ELEMS and span(sx) <= _lib.EW_MAX_ELEMS and (sy is None or span(sy) <= _lib.EW_MAX_ELEMS)


def _i64s(values):
    return (_lib._c.c_int64 * len(values))(*values)


def _ewise_prepare(what, op, x, y):
    op = _ew_op(op)
    if op > _lib.EW_POWER:
        y = None
    elif y is None:
        raise ValueError('%s: op %d takes two operands' % (what, op))
    _same_kind(what, x, y)
    x, y = ewise_operands(x, y)
    return (op, x, y) + _ewise_plan(x, y)


def ewise_fits(x, y=None):
    """whether the kernel takes the map over these operands (mxf_ewise_* would not answer -3); ewise and ewise_bwd_ go through the torch
    expression on the device where it does not"""
    x, y = ewise_operands(x, y)
    return _ewise_fits(*_ewise_plan(x, y)[1:])


def ewise(op, x, y=None):
    """z = op(x, y) (S, ...) for all samples in one launch (mxf_ewise_fwd): op 'add', 'subtract', 'multiply', 'divide', 'power' on x (S|1, ...)
    and y (S|1, ...), broadcast by the numpy rule behind the sample axis, or 'square', 'exp', 'log' on x alone.  An axis of extent 1 or an
    expanded one is shared; a non-contiguous operand is passed as it is, never copied.  More than five axes after merging go through the
    torch expression on the device."""
    op, x, y, shape, extent, sx, sy = _ewise_prepare('ewise', op, x, y)
    if not _ewise_fits(extent, sx, sy):
        return _EW_TORCH[op](x, y).contiguous() if y is not None else _EW_TORCH[op](x)
    z = torch.empty(shape, dtype=x.dtype, device=x.device)
    if z.numel():
        _lib.call('mxf_ewise_fwd', _h(x), op, _dt(x), len(extent), _i64s(extent), _p(x), _i64s(sx), _p(y), None if sy is None else _i64s(sy),
                  _p(z), _stream())
    return z


def _ewise_grads_torch(op, x, y, dz):
    if op == _lib.EW_ADD:
        return dz, dz
    if op == _lib.EW_SUBTRACT:
        return dz, -dz
    if op == _lib.EW_MULTIPLY:
        return dz * y, dz * x
    if op == _lib.EW_DIVIDE:
        return dz / y, -dz * x / (y * y)
    if op == _lib.EW_POWER:
        return dz * y * torch.pow(x, y - 1), dz * torch.pow(x, y) * torch.log(x)
    return {_lib.EW_SQUARE: lambda: 2 * x * dz, _lib.EW_EXP: lambda: dz * torch.exp(x), _lib.EW_LOG: lambda: dz / x}[op](), None


def ewise_bwd_(op, x, y, dz, dx_acc=None, dy_acc=None):
    """Reverse mode of ewise under the cotangent dz (S, ...): dx_acc and dy_acc -- dense, shaped like ewise_operands' x and y, every shared
    axis at extent 1 -- += the gradients, summed over the shared axes in double (mxf_ewise_bwd).  Either may be None."""
    _same_kind('ewise', x, dz, dx_acc, dy_acc)
    op, x, y, shape, extent, sx, sy = _ewise_prepare('ewise', op, x, y)
    if y is None:
        dy_acc = None
    _check_buffers('ewise', (dz, shape), (dx_acc, x.shape), (dy_acc, None if y is None else y.shape))
    if dx_acc is None and dy_acc is None:
        return
    if not _ewise_fits(extent, sx, sy):
        for g, acc in zip(_ewise_grads_torch(op, x, y, dz), (dx_acc, dy_acc)):
            if acc is not None:
                acc.add_(g.sum_to_size(acc.shape))
        return
    if dz.numel():
        _lib.call('mxf_ewise_bwd', _h(x), op, _dt(x), len(extent), _i64s(extent), _p(x), _i64s(sx), _p(y), None if sy is None else _i64s(sy),
                  _p(dz), _p(dx_acc), _p(dy_acc), _stream())


def _reduce_plan(x, axes):
    """x (S, ...) and the per-sample axes to reduce (None: all) -> (x as the kernel takes it: contiguous, the reduced axes one run, the
    permutation that made it so or None, outer, R, inner, the result's shape)"""
    nd = x.dim() - 1
    if axes is None:
        axes = tuple(range(nd))
        out_shape = (x.shape[0], 1)
    else:
        axes = (axes,) if isinstance(axes, int) else tuple(axes)
        axes = tuple(sorted(a + nd if a < 0 else a for a in axes))
        if not axes or len(set(axes)) != len(axes) or axes[0] < 0 or axes[-1] >= nd:
            raise ValueError('reduce: axes %s of a per-sample array of %d dimension(s)' % (axes, nd))
        out_shape = tuple(x.shape[d] for d in range(x.dim()) if d == 0 or d - 1 not in axes)
    full = [a + 1 for a in axes]
    perm = None
    if full and full != list(range(full[0], full[0] + len(full))):
        perm = [d for d in range(x.dim()) if d not in full] + full
        x = x.permute(perm)
        full = list(range(x.dim() - len(full), x.dim()))
    x = x.contiguous()
    lo, hi = (full[0], full[-1] + 1) if full else (x.dim(), x.dim())
    return x, perm, _numel(x.shape[:lo]), _numel(x.shape[lo:hi]), _numel(x.shape[hi:]), out_shape


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def reduce(kind, x, axes=None):
    """'sum', 'mean' or 'prod' of x (S, ...) over the per-sample axes `axes` -- an int, a tuple, or None for all of them -- for all samples in
    one launch (mxf_reduce_fwd).  With axes the result drops them; with None it is (S, 1).  Axes that are not adjacent are brought together
    by a permuted copy first."""
    _same_kind('reduce', x)
    kind = RED_KIND[kind] if isinstance(kind, str) else int(kind)
    xc, _, outer, R, inner, out_shape = _reduce_plan(x, axes)
    out = torch.empty(out_shape, dtype=x.dtype, device=x.device)
    if out.numel():
        _lib.call('mxf_reduce_fwd', _h(xc), kind, _dt(xc), outer, R, inner, _p(xc), _p(out), _stream())
    return out


def reduce_bwd_(kind, x, axes, dy, dx_acc):
    """Reverse mode of reduce under the cotangent dy (shaped like the result): dx_acc, contiguous and shaped like x, += the gradient
    (mxf_reduce_bwd); prod never divides."""
    _same_kind('reduce', x, dy, dx_acc)
    kind = RED_KIND[kind] if isinstance(kind, str) else int(kind)
    xc, perm, outer, R, inner, out_shape = _reduce_plan(x, axes)
    _check_buffers('reduce', (dy, out_shape), (dx_acc, x.shape))
    if not dx_acc.numel():
        return
    acc = dx_acc if perm is None else torch.zeros(xc.shape, dtype=x.dtype, device=x.device)
    _lib.call('mxf_reduce_bwd', _h(xc), kind, _dt(xc), outer, R, inner, _p(xc), _p(dy), _p(acc), _stream())
    if perm is not None:
        inverse = [perm.index(d) for d in range(len(perm))]
        dx_acc.add_(acc.permute(inverse))


def adam_step_(w, g, m, v, lr, t, beta1=0.9, beta2=0.999, epsilon=1e-8, rescale_grad=1.0):
    _lib.call('mxf_adam_step', _h(w), _dt(w), w.numel(), _p(w), _p(g), _p(m), _p(v), float(lr), float(beta1), float(beta2),
              float(epsilon), float(rescale_grad), int(t), _stream())


def uniform_sum(g):
    """sum(g) if all entries of the (small) vector g agree to 1e-6 relative, NaN otherwise -- one launch, no host sync (mxf_uniform_sum)."""
    g = _c(g)
    out = torch.empty((), dtype=g.dtype, device=g.device)
    _lib.call('mxf_uniform_sum', _h(g), _dt(g), g.numel(), _p(g), _p(out), _stream())
    return out


def sgd_step_(w, g, mom, lr, momentum=0.0, wd=0.0, rescale_grad=1.0):
    """MXNet SGD on a flat buffer (mxf_sgd_step); mom = None for plain SGD."""
    _lib.call('mxf_sgd_step', _h(w), _dt(w), w.numel(), _p(w), _p(g), None if mom is None else _p(mom), float(lr), float(momentum), float(wd),
              float(rescale_grad), _stream())


OPT_KIND = {'rmsprop': 1, 'adagrad': 2, 'adadelta': 3, 'nag': 4}


def opt_step_(kind, w, g, s1, s2, lr, p1, epsilon, wd=0.0, rescale_grad=1.0):
    """MXNet 'rmsprop' / 'adagrad' / 'adadelta' / 'nag' on a flat buffer (mxf_opt_step); s1, s2: the rule's state buffers (s2: adadelta only)."""
    _lib.call('mxf_opt_step', _h(w), OPT_KIND[kind], _dt(w), w.numel(), _p(w), _p(g), _p(s1), None if s2 is None else _p(s2), float(lr), float(p1),
              float(epsilon), float(wd), float(rescale_grad), _stream())


def gp_logpdf(kind, X, Y, noise_var, lengthscale, variance, ard, jitter=0.0, want_grad=False):
    """GPRegressionLogPdf.compute (gp_regression.py:42-76).  X (S|1,N,Q), Y (S|1,N,P) [minus mean], noise_var (S|1,1),
    lengthscale (S|1,Q|1), variance (S|1,1).  Returns dict(logL (S,), L (S,N,N), LinvY (S,N,P), info, grads...)."""
    X, Y, noise_var, lengthscale, variance = _c(X), _c(Y), _c(noise_var), _c(lengthscale), _c(variance)
    S = num_samples(X, Y, noise_var, lengthscale, variance)
    N, Q, P = X.shape[-2], X.shape[-1], Y.shape[-1]
    dev, dt = X.device, X.dtype
    out = {'logL': torch.empty(S, dtype=dt, device=dev), 'L': torch.empty((S, N, N), dtype=dt, device=dev),
           'LinvY': torch.empty((S, N, P), dtype=dt, device=dev), 'info': torch.zeros(S, dtype=torch.int32, device=dev)}
    g = {}
    if want_grad:
        g = {'dX': torch.empty((S, N, Q), dtype=dt, device=dev), 'dY': torch.empty((S, N, P), dtype=dt, device=dev),
             'dnoise': torch.empty((S, 1), dtype=dt, device=dev),
             'dls': torch.empty((S, lengthscale.shape[-1]), dtype=dt, device=dev), 'dvar': torch.empty((S, 1), dtype=dt, device=dev)}
    _lib.call('mxf_gp_logpdf', _h(X), KIND[kind], _dt(X), S, N, Q, P, _p(X), _ss(X), _p(Y), _ss(Y), _p(noise_var), _ss(noise_var),
              _p(lengthscale), int(bool(ard)), _ss(lengthscale), _p(variance), _ss(variance), float(jitter),
              _p(out['logL']), _p(out['L']), _p(out['LinvY']), _p(out['info']), int(want_grad),
              _p(g.get('dX')), _p(g.get('dY')), _p(g.get('dnoise')), _p(g.get('dls')), _p(g.get('dvar')), _stream())
    out.update(g)
    return out


def svgp_logpdf(kind, X, Y, Z, noise_var, qU_mean, qU_cov_W, qU_cov_diag, lengthscale, variance, ard, jitter=0.0,
                scaling=1.0, gscale=1.0, want_grad=False):
    """SVGPRegressionLogPdf.compute (svgp_regression.py:43-109).  X (S|1,B,Q), Y (S|1,B,P) [minus mean],
    Z (M,Q), noise_var (1,) | (P,) | (B,1) | (B,P), qU_mean (M,P), qU_cov_W (M,M), qU_cov_diag (M,) [positive], lengthscale (Q|1,), variance (1,).
    Returns dict(logL (S,), info, and -- if want_grad -- the gradients of gscale*sum_s logL[s])."""
    X, Y, Z = _c(X), _c(Y), _c(Z)
    noise_var, qU_mean, qU_cov_W, qU_cov_diag, lengthscale, variance = [_c(t) for t in (noise_var, qU_mean, qU_cov_W, qU_cov_diag, lengthscale, variance)]
    S = num_samples(X, Y)
    B, Q, P, M = X.shape[-2], X.shape[-1], Y.shape[-1], Z.shape[-2]
    dev, dt = X.device, X.dtype
    out = {'logL': torch.empty(S, dtype=dt, device=dev), 'info': torch.zeros(1, dtype=torch.int32, device=dev)}
    # noise_var: (1,) homoscedastic -> streaming fused path; (P,), (B,1) or (B,P) -> mxf_svgp_logpdf_het (svgp_regression.py:61-67)
    if noise_var.dim() == 1:
        noise_var = noise_var.reshape(1, -1)
    nrows, ncols = noise_var.shape
    if nrows not in (1, B) or ncols not in (1, P):
        raise ValueError('svgp_logpdf: noise_var must be (1|B, 1|P), got %s' % (tuple(noise_var.shape),))
    het = nrows * ncols > 1
    g = {}
    if want_grad:
        E = lambda *sh: torch.empty(sh, dtype=dt, device=dev)
        g = {'dX': E(*X.shape), 'dY': E(*Y.shape), 'dZ': E(M, Q), 'dnoise': E(nrows, ncols), 'dmu': E(M, P), 'dW': E(M, M), 'dSdiag': E(M),
             'dls': E(lengthscale.numel()), 'dvar': E(1)}
    tail = (_p(qU_mean), _p(qU_cov_W), _p(qU_cov_diag), _p(lengthscale), int(bool(ard)), _p(variance), float(jitter),
            float(scaling), float(gscale), _p(out['logL']), _p(out['info']), int(want_grad),
            _p(g.get('dX')), _p(g.get('dY')), _p(g.get('dZ')), _p(g.get('dnoise')), _p(g.get('dmu')), _p(g.get('dW')),
            _p(g.get('dSdiag')), _p(g.get('dls')), _p(g.get('dvar')), _stream())
    head = (_h(X), KIND[kind], _dt(X), S, B, M, Q, P, _p(X), _ss(X), _p(Y), _ss(Y), _p(Z), _p(noise_var))
    if het:
        _lib.call('mxf_svgp_logpdf_het', *head, nrows, ncols, *tail)
    else:
        _lib.call('mxf_svgp_logpdf', *head, *tail)
    out.update(g)
    return out


def svgp_logpdf_sampled(kind, X, Y, Z, noise_var, qU_mean, qU_cov_W, qU_cov_diag, lengthscale, variance, ard, jitter=0.0, scaling=1.0,
                        gscale=1.0, want_grad=False):
    """mxf_svgp_logpdf_sampled: the homoscedastic bound with any operand sampled.  Every operand carries a leading sample axis of size S or 1:
    X (S|1,B,Q) Y (S|1,B,P) Z (S|1,M,Q) noise_var (S|1,1) qU_mean (S|1,M,P) qU_cov_W (S|1,M,M) qU_cov_diag (S|1,M) lengthscale (S|1,Q|1)
    variance (S|1,1).  Returns logL (S,), info (S,) and -- if want_grad -- per-sample gradients (S, ...) of gscale * logL[s]."""
    ops_in = [_c(t) for t in (X, Y, Z, noise_var, qU_mean, qU_cov_W, qU_cov_diag, lengthscale, variance)]
    X, Y, Z, noise_var, qU_mean, qU_cov_W, qU_cov_diag, lengthscale, variance = ops_in
    S = max(t.shape[0] for t in ops_in)
    if any(t.shape[0] not in (1, S) for t in ops_in):
        raise ValueError('svgp_logpdf_sampled: sample axes must be 1 or %d' % S)
    B, Q, P, M = X.shape[-2], X.shape[-1], Y.shape[-1], Z.shape[-2]
    if noise_var.numel() != noise_var.shape[0]:
        raise ValueError('svgp_logpdf_sampled: homoscedastic noise (S|1, 1) only')
    dev, dt = X.device, X.dtype
    st = lambda t: 0 if t.shape[0] == 1 else t[0].numel()
    lsn = lengthscale[0].numel()
    out = {'logL': torch.empty(S, dtype=dt, device=dev), 'info': torch.zeros(S, dtype=torch.int32, device=dev)}
    g = {}
    if want_grad:
        E = lambda *sh: torch.empty(sh, dtype=dt, device=dev)
        g = {'dX': E(S, B, Q), 'dY': E(S, B, P), 'dZ': E(S, M, Q), 'dnoise': E(S, 1), 'dmu': E(S, M, P), 'dW': E(S, M, M), 'dSdiag': E(S, M),
             'dls': E(S, lsn), 'dvar': E(S, 1)}
    _lib.call('mxf_svgp_logpdf_sampled', _h(X), KIND[kind], _dt(X), S, B, M, Q, P, _p(X), st(X), _p(Y), st(Y), _p(Z), st(Z), _p(noise_var), st(noise_var),
              _p(qU_mean), st(qU_mean), _p(qU_cov_W), st(qU_cov_W), _p(qU_cov_diag), st(qU_cov_diag), _p(lengthscale), int(bool(ard)), st(lengthscale),
              _p(variance), st(variance), float(jitter), float(scaling), float(gscale), _p(out['logL']), _p(out['info']), int(want_grad),
              _p(g.get('dX')), _p(g.get('dY')), _p(g.get('dZ')), _p(g.get('dnoise')), _p(g.get('dmu')), _p(g.get('dW')), _p(g.get('dSdiag')),
              _p(g.get('dls')), _p(g.get('dvar')), _stream())
    out.update(g)
    return out


def _device_index(device):
    """CUDA device index of `device` (None / torch.device('cuda') without an index -> the current device; int / torch.device / str)."""
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, str):
        device = torch.device(device)
    if isinstance(device, torch.device):
        if device.type != 'cuda':
            raise ValueError('mxfusion_amd: %r is not a GPU device' % (device,))
        return device.index if device.index is not None else torch.cuda.current_device()
    return int(device)


def svgp_cond_nowait(device=None, reset=False):
    """Running maximum of the condition numbers published by the finished svgp_logpdf training calls of this thread on `device`; does not
    synchronise (mxf_svgp_cond_nowait)."""
    return _lib.svgp_cond_nowait(_device_index(device), reset)


def svgp_last_cond(device=None):
    """1-norm condition number of Kuu + jitter I seen by the last svgp_logpdf training call of this thread on `device` (mxf_svgp_last_cond;
    synchronises).  The float32 streaming form is valid up to ~3e3 (include/mxf_gp.h)."""
    idx = _device_index(device)
    return _lib.svgp_last_cond(idx)


# ---- gradient exchange through the C ABI (RCCL); mxfusion_amd's own loops use torch.distributed, these mirror what a reference-side
# binder without PyTorch calls (include/mxf_gp.h) -------------------------------------------------------------
def comm_unique_id(device=None):
    """128-byte rendezvous id (rank 0 creates it and hands it to the other ranks)."""
    import ctypes
    idx = _device_index(device)
    buf = ctypes.create_string_buffer(128)
    _lib.call('mxf_comm_unique_id', _lib.handle(idx), ctypes.cast(buf, ctypes.c_void_p))
    return buf.raw


def comm_init(nranks, rank, unique_id, device=None):
    import ctypes
    idx = _device_index(device)
    assert len(unique_id) == 128
    buf = ctypes.create_string_buffer(bytes(unique_id), 128)
    _lib.call('mxf_comm_init', _lib.handle(idx), int(nranks), int(rank), ctypes.cast(buf, ctypes.c_void_p))


def comm_destroy(device=None):
    idx = _device_index(device)
    _lib.call('mxf_comm_destroy', _lib.handle(idx))


def allreduce_sum_(t):
    """In-place sum over the ranks of the handle's communicator (mxf_allreduce_sum), ordered on the current stream."""
    assert t.is_contiguous()
    _lib.call('mxf_allreduce_sum', _h(t), _dt(t), _p(t), t.numel(), _stream())
    return t


def bcast_(t, root=0):
    assert t.is_contiguous()
    _lib.call('mxf_bcast', _h(t), _dt(t), _p(t), t.numel(), int(root), _stream())
    return t


def svgp_logpdf_mat(Kuu, Kuf, Kdiag, Y, noise_var, qU_mean, qU_cov_W, qU_cov_diag, jitter=0.0, scaling=1.0, gscale=1.0, want_grad=False):
    """SVGP bound from materialised Grams: Kuu (M,M) without jitter, Kuf (M,B), Kdiag (B,), Y (B,P) or (S,B,P) [S samples of the outputs over
    the same inputs], noise_var (1,) | (P,) | (B,1) | (B,P).  Returns dict(logL (S,), info, and -- if want_grad -- dKuu, dKuf, dKdiag, dY,
    dnoise, dmu, dW, dSdiag of gscale * sum_s logL[s])."""
    Kuu, Kuf, Kdiag, Y, noise_var, qU_mean, qU_cov_W, qU_cov_diag = [_c(t) for t in (Kuu, Kuf, Kdiag, Y, noise_var, qU_mean, qU_cov_W, qU_cov_diag)]
    M, B, P = Kuf.shape[-2], Kuf.shape[-1], Y.shape[-1]
    S = Y.shape[0] if Y.dim() == 3 else 1
    dev, dt = Kuf.device, Kuf.dtype
    if noise_var.dim() == 1:
        noise_var = noise_var.reshape(1, -1)
    nrows, ncols = noise_var.shape
    if nrows not in (1, B) or ncols not in (1, P):
        raise ValueError('svgp_logpdf_mat: noise_var must be (1|B, 1|P), got %s' % (tuple(noise_var.shape),))
    out = {'logL': torch.empty(S, dtype=dt, device=dev), 'info': torch.zeros(1, dtype=torch.int32, device=dev)}
    g = {}
    if want_grad:
        E = lambda *sh: torch.empty(sh, dtype=dt, device=dev)
        g = {'dKuu': E(M, M), 'dKuf': E(M, B), 'dKdiag': E(B), 'dY': E(*Y.shape), 'dnoise': E(nrows, ncols), 'dmu': E(M, P), 'dW': E(M, M),
             'dSdiag': E(M)}
    _lib.call('mxf_svgp_logpdf_mat', _h(Kuf), _dt(Kuf), S, B, M, P, _p(Kuu), _p(Kuf), _p(Kdiag), _p(Y), B * P if S > 1 else 0, _p(noise_var),
              nrows, ncols, _p(qU_mean), _p(qU_cov_W), _p(qU_cov_diag), float(jitter), float(scaling), float(gscale), _p(out['logL']),
              _p(out['info']), int(want_grad), _p(g.get('dKuu')), _p(g.get('dKuf')), _p(g.get('dKdiag')), _p(g.get('dY')), _p(g.get('dnoise')),
              _p(g.get('dmu')), _p(g.get('dW')), _p(g.get('dSdiag')), _stream())
    out.update(g)
    return out


def coldot(A, B):
    """out[s, n] = sum_m A[s, m, n] * B[s, m, n]  (F.sum(A*B, axis=-2))."""
    A, B = _c(A), _c(B)
    S, M, N = max(A.shape[0], B.shape[0]), A.shape[-2], A.shape[-1]
    out = torch.empty((S, N), dtype=A.dtype, device=A.device)
    _lib.call('mxf_coldot', _h(A), _dt(A), S, M, N, _p(A), A.stride(-2), _ss(A), _p(B), B.stride(-2), _ss(B), _p(out), _stream())
    return out


def kdiag(kind, X, lengthscale, variance, ard):
    """Kernel.Kdiag through the C ABI (mxf_kdiag): X (S,N,Q) -> (S,N).  For 'linear', `lengthscale` carries the variances."""
    X = _c(X)
    S, N, Q = X.shape
    ls = None if lengthscale is None else _c(lengthscale).reshape(-1, _c(lengthscale).shape[-1])
    var = None if variance is None else _c(variance).reshape(-1)
    out = torch.empty((S, N), dtype=X.dtype, device=X.device)
    sls = 0 if ls is None or ls.shape[0] == 1 else ls.shape[-1]
    svar = 0 if var is None or var.numel() == 1 else 1
    _lib.call('mxf_kdiag', _h(X), KIND[kind], _dt(X), S, N, Q, _p(X), N * Q, _p(ls), int(bool(ard)), sls, _p(var), svar, _p(out), _stream())
    return out


def gp_predict(kind, X_cond, X_test, lengthscale, variance, ard, L, LinvY, noise_var, noise_free=False, full_cov=False):
    """GPRegressionMeanVariancePrediction.compute (gp_regression.py:146-196) as one C-ABI call (mxf_gp_predict): one posterior
    (L (N,N), LinvY (N,P)), X_test (S,Nt,Q) -> mean (S,Nt,P), var (S,Nt) or (S,Nt,Nt)."""
    X_cond, X_test, lengthscale, variance, L, LinvY = [_c(t) for t in (X_cond, X_test, lengthscale, variance, L, LinvY)]
    S, Nt, Q = X_test.shape
    N, P = X_cond.shape[-2], LinvY.shape[-1]
    mean = torch.empty((S, Nt, P), dtype=X_test.dtype, device=X_test.device)
    var = torch.empty((S, Nt, Nt) if full_cov else (S, Nt), dtype=X_test.dtype, device=X_test.device)
    _lib.call('mxf_gp_predict', _h(X_test), KIND[kind], _dt(X_test), S, N, Nt, Q, P, _p(X_cond), _p(X_test), _p(lengthscale), int(bool(ard)),
              _p(variance), _p(L), L.stride(-2), _p(LinvY), None if noise_var is None else _p(_c(noise_var)), int(bool(noise_free)),
              int(bool(full_cov)), _p(mean), _p(var), _stream())
    return mean, var


def svgp_predict(kind, Z, X_test, lengthscale, variance, ard, qU_mean, qU_cov_W, qU_cov_diag, noise_var, jitter=0.0, noise_free=False,
                 full_cov=False):
    """SVGPRegressionMeanVariancePrediction.compute (svgp_regression.py:121-189) as one C-ABI call (mxf_svgp_predict).
    Returns mean (S,Nt,P), var (S,Nt) or (S,Nt,Nt), info (2,) int32."""
    Z, X_test, lengthscale, variance, qU_mean, qU_cov_W, qU_cov_diag = [_c(t) for t in (Z, X_test, lengthscale, variance, qU_mean, qU_cov_W,
                                                                                        qU_cov_diag)]
    S, Nt, Q = X_test.shape
    M, P = Z.shape[-2], qU_mean.shape[-1]
    mean = torch.empty((S, Nt, P), dtype=X_test.dtype, device=X_test.device)
    var = torch.empty((S, Nt, Nt) if full_cov else (S, Nt), dtype=X_test.dtype, device=X_test.device)
    info = torch.zeros(2, dtype=torch.int32, device=X_test.device)
    _lib.call('mxf_svgp_predict', _h(X_test), KIND[kind], _dt(X_test), S, M, Nt, Q, P, _p(Z), _p(X_test), _p(lengthscale), int(bool(ard)),
              _p(variance), _p(qU_mean), _p(qU_cov_W), _p(qU_cov_diag), None if noise_var is None else _p(_c(noise_var)), float(jitter),
              int(bool(noise_free)), int(bool(full_cov)), _p(mean), _p(var), _p(info), _stream())
    return mean, var, info


def sgp_logpdf(kind, X, Y, Z, noise_var, lengthscale, variance, ard, jitter=0.0, gscale=1.0, want_grad=False):
    """SparseGPRegressionLogPdf.compute (sparsegp_regression.py:42-108) for ONE sample: X (B,Q), Y (B,P), Z (M,Q), noise_var (1,),
    lengthscale (Q|1,), variance (1,).  Returns dict(logL (1,), wv (M,P), L (M,M), LA (M,M), info, gradients...)."""
    X, Y, Z, noise_var, lengthscale, variance = [_c(t) for t in (X, Y, Z, noise_var, lengthscale, variance)]
    B, Q, P, M = X.shape[-2], X.shape[-1], Y.shape[-1], Z.shape[-2]
    dev, dt = X.device, X.dtype
    E = lambda *sh: torch.empty(sh, dtype=dt, device=dev)
    out = {'logL': E(1), 'wv': E(M, P), 'L': E(M, M), 'LA': E(M, M), 'info': torch.zeros(1, dtype=torch.int32, device=dev)}
    g = {}
    if want_grad:
        g = {'dX': E(B, Q), 'dY': E(B, P), 'dZ': E(M, Q), 'dnoise': E(1), 'dls': E(lengthscale.numel()), 'dvar': E(1)}
    _lib.call('mxf_sgp_logpdf', _h(X), KIND[kind], _dt(X), B, M, Q, P, _p(X), _p(Y), _p(Z), _p(noise_var), _p(lengthscale),
              int(bool(ard)), _p(variance), float(jitter), float(gscale), _p(out['logL']), _p(out['wv']), _p(out['L']), _p(out['LA']),
              _p(out['info']), int(want_grad), _p(g.get('dX')), _p(g.get('dY')), _p(g.get('dZ')), _p(g.get('dnoise')), _p(g.get('dls')),
              _p(g.get('dvar')), _stream())
    out.update(g)
    return out
