"""Operands of the dense C ABI (include/mxf_gp.h) laid out as VIEWS inside a larger allocation: padded rows (ld > width), a base that is not
16-byte aligned, a gap between samples -- and a checker that every byte outside the view survived the call.  Plain module, no fixtures.

    v = carve(a, ld_pad=3, lead=1, gap=5)      # torch view (S, R, C) with strides (R * ld + gap, ld, 1) at element offset `lead`
    snap = snapshot(v)
    gemm(A, B, C=v, ...)                        # the thin callers below pass data_ptr / ld / sample stride of the views as they are
    assert_padding_untouched(v, snap)

Input padding is NaN (an over-read that reaches the arithmetic poisons the result); output padding is SENTINEL, a finite value with a bit
pattern no kernel produces.  The allocation ends with TAIL more padding elements, so a correct kernel never leaves it and a store one
vector past the last row still lands inside it (and is seen).  ops.* is bypassed on purpose: it makes every operand contiguous."""
import numpy as np
import torch

NAN = float('nan')
SENTINEL = -123456.7890625      # exact in float32 and float64
TAIL = 64                       # padding elements behind the last sample


def carve(array, ld_pad=0, lead=0, gap=0, fill=NAN, device=None, dtype=None):
    """A view holding `array` ((R, C) or (S, R, C); numpy or torch) inside a fresh 1-D allocation filled with `fill`:
    row stride ld = C + ld_pad, sample stride R * ld + gap, first element at offset `lead`.  The view's ._base is the allocation."""
    a = torch.as_tensor(np.asarray(array) if not torch.is_tensor(array) else array)
    if dtype is not None:
        a = a.to(dtype)
    if a.dim() not in (2, 3):
        raise ValueError('carve: (R, C) or (S, R, C) arrays')
    if min(ld_pad, lead, gap) < 0:
        raise ValueError('carve: negative padding')
    shape = tuple(a.shape)
    S, (R, C) = (shape[0] if a.dim() == 3 else 1), shape[-2:]
    ld = C + ld_pad
    sstride = R * ld + gap
    base = torch.full((lead + S * sstride + TAIL,), fill, dtype=a.dtype, device=device if device is not None else a.device)
    strides = (sstride, ld, 1) if a.dim() == 3 else (ld, 1)
    view = base.as_strided(shape, strides, lead)
    view.copy_(a)
    assert view._base is base
    return view


def ld(v):
    """leading dimension (row stride in elements) of a carved view"""
    return v.stride(-2)


def sstride(v):
    """sample stride in elements; a single-sample 3-D view broadcasts (stride 0, include/mxf_gp.h)"""
    if v is None or v.dim() < 3 or v.shape[0] == 1:
        return 0
    return v.stride(0)


def _bits(t):
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])


def _outside(v):
    """bool mask over the allocation: True where an element does NOT belong to the view"""
    base = v._base
    m = torch.ones(base.numel(), dtype=torch.bool, device=base.device)
    m.as_strided(tuple(v.shape), v.stride(), v.storage_offset()).fill_(False)
    return m


def snapshot(v):
    """bit copy of the whole allocation behind a carved view (take it right before the call under test)"""
    return _bits(v._base).clone()


def padding_diff(v, snap):
    """indices (into the allocation) of the elements outside the view whose bits differ from the snapshot"""
    changed = (_bits(v._base) != snap) & _outside(v)
    return changed.nonzero().reshape(-1)


def assert_padding_untouched(v, snap, what=''):
    bad = padding_diff(v, snap)
    if bad.numel():
        i = int(bad[0])
        off = i - v.storage_offset()
        raise AssertionError('%s: %d element(s) outside the view changed; first at allocation index %d (view offset %d, ld %d, sample stride %d): '
                             '%r' % (what or 'padding', bad.numel(), i, off, ld(v), v.stride(0) if v.dim() == 3 else 0,
                                     v._base[i].item()))


def assert_unchanged(v, snap, what=''):
    """an input operand: nothing of its allocation, view included, may change"""
    if not torch.equal(_bits(v._base), snap):
        raise AssertionError('%s: a read-only operand was written' % (what or 'input'))


# ---- layout variants of the issue: (name, ld_pad, lead, gap) -------------------------------------------------------------------------
PLAIN = ('plain', 0, 0, 0)
LD8 = ('ld+8', 8, 0, 0)            # (a) padded, rows stay 16-byte aligned for aligned widths
LD3 = ('ld+3', 3, 0, 0)            # (b) padded, rows lose their alignment
LEAD1 = ('lead1', 0, 1, 0)         # (c) base off by one element, ld as it was
LEAD1_LD8 = ('lead1+ld8', 8, 1, 0)
GAP5 = ('gap5', 0, 0, 5)           # (d) gap between samples, not a multiple of 4 elements
GAP5_LD8 = ('gap5+ld8', 8, 0, 5)
VARIANTS = {v[0]: v for v in (PLAIN, LD8, LD3, LEAD1, LEAD1_LD8, GAP5, GAP5_LD8)}


def carve_as(array, variant, fill=NAN, device='cuda', dtype=None):
    _, ld_pad, lead, gap = VARIANTS[variant] if isinstance(variant, str) else variant
    return carve(array, ld_pad=ld_pad, lead=lead, gap=gap, fill=fill, device=device, dtype=dtype)


# ---- thin callers: explicit pointers, leading dimensions and strides through _lib.call ---------------------------------------------------
def _ctx(t):
    from mxfusion_amd import _lib
    dt = {torch.float32: _lib.F32, torch.float64: _lib.F64}[t.dtype]
    return _lib, _lib.handle(t.device.index if t.device.index is not None else torch.cuda.current_device()), dt, torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def gemm(A, B, C, transA=False, transB=False, alpha=1.0, beta=0.0):
    """mxf_gemm on 3-D views A (S|1, ., .), B (S|1, ., .), C (S, M, N)"""
    lib, h, dt, st = _ctx(C)
    S, M, N = C.shape
    K = A.shape[-2] if transA else A.shape[-1]
    lib.call('mxf_gemm', h, dt, int(transA), int(transB), M, N, K, float(alpha), _p(A), ld(A), sstride(A), _p(B), ld(B), sstride(B),
             float(beta), _p(C), ld(C), sstride(C) if S > 1 else C.stride(0), S, st)


def gemm_split(name, A, B, C, alpha=1.0, beta=0.0, lower_only=False):
    """mxf_gemm_f32x3 / mxf_gemm_f16x2 on 2-D float32 views A (M, K), B (N, K), C (M, N)"""
    lib, h, _, st = _ctx(C)
    (M, K), N = A.shape, B.shape[0]
    lib.call(name, h, M, N, K, float(alpha), _p(A), ld(A), _p(B), ld(B), float(beta), _p(C), ld(C), int(bool(lower_only)), st)


def split_planes(mode, X):
    """mxf_f16x2_split (mode 'f16x2': returns (planes, maxword)) / mxf_f32x3_split (mode 'f32x3': returns planes) of a 2-D float32 view"""
    lib, h, _, st = _ctx(X)
    R, K = X.shape
    n = lib.load().mxf_f32x3_plane_elems(R, K)
    if mode == 'f16x2':
        planes = torch.empty(2 * n, dtype=torch.int16, device=X.device)
        word = torch.zeros(1, dtype=torch.int32, device=X.device)
        lib.call('mxf_f16x2_split', h, R, K, _p(X), ld(X), _p(planes), _p(word), st)
        return planes, word
    planes = torch.empty(3 * n, dtype=torch.int16, device=X.device)
    lib.call('mxf_f32x3_split', h, R, K, _p(X), ld(X), _p(planes), st)
    return planes


def gemm_planes(mode, pa, pb, C, K, alpha=1.0, beta=0.0, lower_only=False):
    """mxf_gemm_f16x2_planes / mxf_gemm_f32x3_planes into a 2-D view C (M, N)"""
    lib, h, _, st = _ctx(C)
    M, N = C.shape
    if mode == 'f16x2':
        lib.call('mxf_gemm_f16x2_planes', h, M, N, K, float(alpha), _p(pa[0]), _p(pa[1]), _p(pb[0]), _p(pb[1]), float(beta), _p(C), ld(C),
                 int(bool(lower_only)), st)
    else:
        lib.call('mxf_gemm_f32x3_planes', h, M, N, K, float(alpha), _p(pa), _p(pb), float(beta), _p(C), ld(C), int(bool(lower_only)), st)


def potrf(A):
    """mxf_potrf in place on a view A (S, n, n); returns the info words"""
    lib, h, dt, st = _ctx(A)
    S, n = A.shape[0], A.shape[-1]
    info = torch.zeros(S, dtype=torch.int32, device=A.device)
    lib.call('mxf_potrf', h, dt, S, n, _p(A), ld(A), A.stride(0), _p(info), st)
    return info


def trsm(L, B, transpose=False):
    """mxf_trsm in place on B (S, n, nrhs); L (S|1, n, n)"""
    lib, h, dt, st = _ctx(B)
    S, n, nrhs = B.shape
    lib.call('mxf_trsm', h, dt, int(bool(transpose)), S, n, nrhs, _p(L), ld(L), sstride(L), _p(B), ld(B), B.stride(0), st)


def trtri(L, Linv):
    lib, h, dt, st = _ctx(L)
    S, n = L.shape[0], L.shape[-1]
    lib.call('mxf_trtri', h, dt, S, n, _p(L), ld(L), L.stride(0), _p(Linv), ld(Linv), Linv.stride(0), st)


def sumlogdiag(L):
    lib, h, dt, st = _ctx(L)
    S, n = L.shape[0], L.shape[-1]
    out = torch.empty(S, dtype=L.dtype, device=L.device)
    lib.call('mxf_sumlogdiag', h, dt, S, n, _p(L), ld(L), L.stride(0), _p(out), st)
    return out


def _xs(v):
    """sample stride of a coordinate / parameter operand whose per-sample block is contiguous (the contract of X, X2, lengthscale ...)"""
    return 0 if v is None or v.shape[0] == 1 else v.stride(0)


def gram(kind, X, X2, ls, var, ard, K, diag_add=None, jitter=0.0, mode=0):
    """mxf_gram into a view K (S, N, N2); X (S|1, N, Q) and X2 may sit at a sample stride larger than N Q"""
    lib, h, dt, st = _ctx(K)
    S, N, N2 = K.shape
    lib.call('mxf_gram', h, kind, dt, S, N, N2, X.shape[-1], _p(X), _xs(X), _p(X2), _xs(X2), _p(ls), int(bool(ard)), _xs(ls), _p(var), _xs(var),
             _p(diag_add), _xs(diag_add), float(jitter), int(mode), _p(K), ld(K), K.stride(0), st)


def gram2(kind1, kind2, op, X, X2, ls1, var1, ard1, ls2, var2, ard2, K, diag_add=None, jitter=0.0):
    lib, h, dt, st = _ctx(K)
    S, N, N2 = K.shape
    lib.call('mxf_gram2', h, kind1, kind2, int(op), dt, S, N, N2, X.shape[-1], _p(X), _xs(X), _p(X2), _xs(X2), _p(ls1), int(bool(ard1)), _xs(ls1),
             _p(var1), _xs(var1), _p(ls2), int(bool(ard2)), _xs(ls2), _p(var2), _xs(var2), _p(diag_add), _xs(diag_add), float(jitter),
             _p(K), ld(K), K.stride(0), st)


def gram_bwd(kind, X, X2, ls, var, ard, dK, out=None):
    """mxf_gram_bwd from a view dK (S, N, N2); returns freshly zeroed (dX, dX2, dls, dvar), contiguous.
    out: the caller's own output buffers (dX, dX2, dls, dvar), contiguous and shaped like the primals, passed as they are -- the call
    ACCUMULATES into them, and None is a null pointer (that gradient is not computed)"""
    lib, h, dt, st = _ctx(dK)
    S, N, N2 = dK.shape
    z = lambda t: None if t is None else torch.zeros(tuple(t.shape), dtype=t.dtype, device=t.device)
    if out is None:
        dX, dX2, dls, dvar = z(X), z(X2), z(ls), z(var)
    else:
        dX, dX2, dls, dvar = out
        for o, p in zip(out, (X, X2, ls, var)):
            assert o is None or (p is not None and o.is_contiguous() and o.shape == p.shape and o.dtype == p.dtype), 'gram_bwd: output buffer'
    # contiguous outputs: their sample strides are implied by the shapes, as for the inputs
    assert X.is_contiguous() and (X2 is None or X2.is_contiguous()), 'gram_bwd writes dX / dX2 with the strides of X / X2'
    lib.call('mxf_gram_bwd', h, kind, dt, S, N, N2, X.shape[-1], _p(X), _xs(X), _p(X2), _xs(X2), _p(ls), int(bool(ard)), _xs(ls), _p(var), _xs(var),
             _p(dK), ld(dK), dK.stride(0), _p(dX), _p(dX2), _p(dls), _p(dvar), st)
    return dX, dX2, dls, dvar


def coldot(A, B):
    """mxf_coldot of views A, B (S|1, M, N) -> (S, N)"""
    lib, h, dt, st = _ctx(A)
    S, (M, N) = max(A.shape[0], B.shape[0]), A.shape[-2:]
    out = torch.empty((S, N), dtype=A.dtype, device=A.device)
    lib.call('mxf_coldot', h, dt, S, M, N, _p(A), ld(A), sstride(A), _p(B), ld(B), sstride(B), _p(out), st)
    return out
