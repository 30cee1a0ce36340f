"""GPU: the dense entry points of include/mxf_gp.h on operands that are VIEWS -- padded rows (ld > width), a base that is not 16-byte
aligned, a gap between samples, sample stride 0, outputs that are windows of a larger buffer -- against numpy / torch float64 on the CPU.

ops.* makes every operand contiguous and torch allocations are 256-byte aligned, so the rest of the suite only ever runs ld == width,
stride == rows * width and an aligned base: the branches that choose a vector loader / store or the LDS-DMA kernel from the alignment of
(pointer, ld, stride) are taken here (tests/_strided.py builds the views and calls the C ABI with explicit pointers, lds and strides).
Input padding is NaN (an over-read poisons the result), output padding a finite sentinel compared bit for bit after the call.
Tolerances and their scaling are those of the contiguous tests of the same operation (named at each test).

Observed once on an MI355X with a scratch build whose generic gemm_kernel stores at C + row * N + col (N for ldc): tests/test_gpu_gemm.py
passes (124 passed), this file fails in 152 of 1045 cases -- every test_gemm_layouts row with ldc > N that reaches that kernel (C:ld+8,
C:ld+3, the all:* rows, A:stride0,B:lead1), and every potrf case of test_chol_family_layouts and of the two plan tests, whose updates are
gemm calls on sub-blocks.  C:gap5 alone does not see that mutation (ldc == N there; it guards the sample stride)."""
import functools

import numpy as np
import pytest
import torch

import _strided as st

pytestmark = pytest.mark.gpu

from oracle import gp_oracle as O  # noqa: E402

F32, F64 = torch.float32, torch.float64
NAN, SENT = st.NAN, st.SENTINEL


def _np(v):
    return v.double().cpu().numpy()


# ======================================================================================================================== mxf_gemm
# Kernel reached by each shape (gemm_plan.h: gemm_plan; t128 = ceil(M/128) ceil(N/128) batch, batch = 2):
#   float64, t128 <= 64                      -> gemm_small_f64_kernel (64 x 64 tiles, guarded scalar loaders); K >= 128 -> split-K + scale_kernel
#   float64, t128 > 64, M % 128 == N % 128 == 0, K % 16 == 0, BOTH operands vectorisable (pointer % 16, ld % 2, stride % 2)
#                                            -> gemm_f64_dma_kernel (LDS-DMA); one misaligned operand -> gemm_kernel<double>
#   everything else                          -> gemm_kernel<T> (128 x 128): interior tiles with (kend - kbeg) % 32 == 0 take load_tile_vec
#                                               per operand when that operand is vectorisable, else the guarded load_tile
#   tiles < CU slots and K >= 256            -> split-K: atomic epilogue, scale_kernel (indexes with ldc / sC) when beta != 1
GEMM_SHAPES = {
    F64: [(130, 257, 33),        # small-tile kernel, 3 x 5 tiles, ragged
          (130, 70, 1000),       # small-tile kernel, split-K 15 + scale_kernel
          (1100, 1200, 96),      # 128 x 128 generic kernel, 9 x 10 tiles with an interior (vector loaders) and ragged edges, one launch
          (1152, 1280, 208),     # LDS-DMA eligible (9 x 10 tiles, short K); a misaligned operand steps down to the generic kernel
          (1152, 1152, 1040),    # LDS-DMA + split-K 3 + scale_kernel
          (1100, 1200, 1040)],   # generic kernel + split-K 2 + scale_kernel
    F32: [(130, 257, 33),        # 128 x 128 kernel, 2 x 3 ragged tiles, k tail
          (300, 400, 96),        # 128 x 128 kernel, 3 x 4 tiles: interior tiles with vector loaders (K = 3 BK), ragged last row / column
          (300, 400, 1040)],     # ... + split-K (on 256 CUs: 7 chunks of 160 + scale_kernel; the last is 80 wide, not a multiple of BK,
                                 #     so its interior tiles take the guarded loader, the other chunks the vector loader)
}
# (name, variant of A, of B, of C, the operand shared by the batch with stride 0 -- variant (e) -- or None)
GEMM_LAYOUTS = [('A:ld+8', 'ld+8', 'plain', 'plain', None), ('A:ld+3', 'ld+3', 'plain', 'plain', None),
                ('A:lead1,B:plain', 'lead1', 'plain', 'plain', None), ('A:gap5', 'gap5', 'plain', 'plain', 'B'),
                ('B:ld+8', 'plain', 'ld+8', 'plain', None), ('B:ld+3', 'plain', 'ld+3', 'plain', 'B'),
                ('A:plain,B:lead1', 'plain', 'lead1', 'plain', None), ('B:gap5', 'plain', 'gap5', 'plain', None),
                ('C:ld+8', 'plain', 'plain', 'ld+8', None), ('C:ld+3', 'plain', 'plain', 'ld+3', None),
                ('C:lead1', 'plain', 'plain', 'lead1', 'B'), ('C:gap5', 'plain', 'plain', 'gap5', None),
                ('all:lead1+ld8', 'lead1+ld8', 'lead1+ld8', 'lead1+ld8', None), ('all:gap5+ld8', 'gap5+ld8', 'gap5+ld8', 'gap5+ld8', None),
                ('A:stride0', 'ld+8', 'plain', 'plain', 'A'), ('A:stride0,B:lead1', 'plain', 'lead1', 'ld+3', 'A')]


@functools.lru_cache(maxsize=4)
def _gemm_data(M, N, K, ta, tb):
    rng = np.random.RandomState(M * 7 + N * 3 + K + 2 * ta + tb)
    S = 2
    A = rng.randn(S, K, M) if ta else rng.randn(S, M, K)
    B = rng.randn(S, N, K) if tb else rng.randn(S, K, N)
    C0 = rng.randn(S, M, N)
    opA = np.swapaxes(A, 1, 2) if ta else A
    opB = np.swapaxes(B, 1, 2) if tb else B
    return A, B, C0, opA @ opB, opA @ opB[:1], opA[:1] @ opB


@pytest.mark.parametrize('layout', GEMM_LAYOUTS, ids=[l[0] for l in GEMM_LAYOUTS])
@pytest.mark.parametrize('ta,tb', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('dtype,shape', [(dt, s) for dt in (F64, F32) for s in GEMM_SHAPES[dt]],
                         ids=['%s-%dx%dx%d' % ((('f64', 'f32')[dt == F32],) + s) for dt in (F64, F32) for s in GEMM_SHAPES[dt]])
def test_gemm_layouts(dtype, shape, ta, tb, layout):
    """Tolerance of test_gemm_vs_cpu: rtol = tol, atol = tol sqrt(K), tol = 1e-12 / 2e-5, alpha = 0.7, beta = -0.3."""
    _, vA, vB, vC, shared = layout
    M, N, K = shape
    tol = 1e-12 if dtype == F64 else 2e-5
    A, B, C0, P, PB, PA = _gemm_data(M, N, K, ta, tb)
    if shared == 'B':                             # (e) stride 0: one B for both batch entries
        B, P = B[:1], PB
    if shared == 'A':                             # ... one A (sA == 0 is an input of the vecA guard)
        A, P = A[:1], PA
    if dtype == F32:                              # the reference multiplies the operands the kernel sees
        r32 = lambda a: a.astype(np.float32).astype(np.float64)
        A, B, C0 = r32(A), r32(B), r32(C0)
        opA, opB = (np.swapaxes(A, 1, 2) if ta else A), (np.swapaxes(B, 1, 2) if tb else B)
        P = opA @ opB
    dA, dB = st.carve_as(A, vA, NAN, dtype=dtype), st.carve_as(B, vB, NAN, dtype=dtype)
    dC = st.carve_as(C0, vC, SENT, dtype=dtype)
    sA, sB, sC = st.snapshot(dA), st.snapshot(dB), st.snapshot(dC)
    st.gemm(dA, dB, dC, ta, tb, 0.7, -0.3)
    got = _np(dC)
    st.assert_padding_untouched(dC, sC, 'C ' + layout[0])
    st.assert_unchanged(dA, sA, 'A')
    st.assert_unchanged(dB, sB, 'B')
    ref = 0.7 * P - 0.3 * C0
    assert np.allclose(got, ref, rtol=tol, atol=tol * np.sqrt(K))
    # beta == 0 never reads C: a window holding NaN gets the finite product (the epilogues and both scale_kernels special-case it)
    dN = st.carve_as(np.full_like(C0, np.nan), vC, SENT, dtype=dtype)
    sN = st.snapshot(dN)
    st.gemm(dA, dB, dN, ta, tb, 1.0, 0.0)
    got = _np(dN)
    st.assert_padding_untouched(dN, sN, 'C (beta = 0) ' + layout[0])
    assert np.isfinite(got).all()
    assert np.allclose(got, P, rtol=tol, atol=tol * np.sqrt(K))


# ============================================================================================== split GEMMs (gemm_split.hip), float32
# C = alpha A B^T + beta C, A (M x K), B (N x K).  Kernels (split_plan):
#   split pass: split_planes_kernel reads float4 only when ld % 4 == 0 and X is 16-byte aligned, else element-wise; mxf_gemm_f16x2 /
#     mxf_f16x2_split first run maxabs_kernel (indexes with ld);
#   (130, 70, 50)       -> gemm_split_kernel<false, NP> (128 x 128 tiles, guarded register loaders; ragged M, N, K)
#   (256, 384, 1024)    -> gemm_split_kernel<true, NP>  (LDS-DMA from the planes), split-K 8: atomic epilogue + split_scale_kernel (ldc)
#   (300, 300, 333) lower_only -> gemm_split_kernel<false, NP>, the tiles on and below the diagonal
#   (1024, 1024, 4096) lower_only, f16x2 -> gemm_f16x2_wide_kernel_256lo (16-byte stores into C) ONLY when ldc % 4 == 0 and C is 16-byte
#     aligned (ldc = N + 8 stays wide); ldc = N + 1 or C one float off -> gemm_split_kernel<true, 2>.  f32x3 always takes the tile kernel.
SPLIT_SHAPES = [(130, 70, 50, False), (256, 384, 1024, False), (300, 300, 333, True)]
SPLIT_LAYOUTS = [('A:ld+8', 'ld+8', 'plain', 'plain'), ('A:ld+3', 'ld+3', 'plain', 'plain'), ('A:lead1,B:plain', 'lead1', 'plain', 'plain'),
                 ('B:ld+8', 'plain', 'ld+8', 'plain'), ('B:ld+3', 'plain', 'ld+3', 'plain'), ('A:plain,B:lead1', 'plain', 'lead1', 'plain'),
                 ('C:ld+8', 'plain', 'plain', 'ld+8'), ('C:ld+3', 'plain', 'plain', 'ld+3'), ('C:lead1', 'plain', 'plain', 'lead1'),
                 ('all:lead1+ld8', 'lead1+ld8', 'lead1+ld8', 'lead1+ld8')]
LD1 = ('ld+1', 1, 0, 0)
SPLIT_CASES = [(s, l) for s in SPLIT_SHAPES for l in SPLIT_LAYOUTS] + \
              [((1024, 1024, 4096, True), l) for l in (('C:ld+8(wide)', 'plain', 'plain', 'ld+8'), ('C:ld+1', 'plain', 'plain', LD1),
                                                        ('C:lead1', 'plain', 'plain', 'lead1'), ('A:lead1,B:ld+3', 'lead1', 'ld+3', 'plain'))]


@functools.lru_cache(maxsize=2)
def _split_data(M, N, K):
    """operands of test_gemm_f32x3_is_f32_accurate (both signs, wide dynamic range), as float32 values"""
    rng = np.random.RandomState(M * 7 + N * 3 + K)
    A = ((rng.rand(M, K) * 2 - 0.7) * np.exp(rng.randn(M, 1))).astype(np.float32)
    B = (np.exp(-rng.rand(N, K) * 8) * (rng.rand(N, K) - 0.3)).astype(np.float32)
    C0 = rng.uniform(-2, 2, (M, N)).astype(np.float32)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    return A, B, C0, A64 @ B64.T, np.abs(A64) @ np.abs(B64).T


@pytest.mark.parametrize('shape,layout', SPLIT_CASES, ids=['%dx%dx%d%s-%s' % (s[0], s[1], s[2], '-lower' if s[3] else '', l[0]) for s, l in SPLIT_CASES])
@pytest.mark.parametrize('mode', ['f32x3', 'f16x2'])
def test_split_gemm_layouts(mode, shape, layout):
    """Bound of test_gemm_f32x3_is_f32_accurate / test_gemm_f16x2_is_f32_accurate: 4e-7 of sum |a||b|; beta = 1 into a window as those tests
    bound their accumulating call (4e-7 resp. 2e-6 of the magnitude of the terms, here sum |a||b| + |C0| / 2 <= theirs)."""
    _, vA, vB, vC = layout
    M, N, K, lower = shape
    A, B, C0, ref, scale = _split_data(M, N, K)
    msk = np.tril(np.ones((M, N))) if lower else np.ones((M, N))
    dA, dB = st.carve_as(A, vA, NAN), st.carve_as(B, vB, NAN)
    sA, sB = st.snapshot(dA), st.snapshot(dB)
    # the one-call entry point, beta = 0, into a window that holds C0
    dC = st.carve_as(C0, vC, SENT)
    sC = st.snapshot(dC)
    st.gemm_split('mxf_gemm_' + mode, dA, dB, dC, lower_only=lower)
    got = _np(dC)
    st.assert_padding_untouched(dC, sC, 'C ' + layout[0])
    st.assert_unchanged(dA, sA, 'A')
    st.assert_unchanged(dB, sB, 'B')
    e = float(((np.abs(got - ref) / scale) * msk).max())
    assert e < 4e-7, e
    if lower:      # the strict upper triangle of the window keeps its bits
        up = np.triu(np.ones((M, N), dtype=bool), 1)
        assert np.array_equal(dC.cpu().numpy()[up].view(np.int32), C0[up].view(np.int32))
    # the two halves: split pass on the padded / misaligned operands, then the planes product with beta = 1 into a window
    pa, pb = st.split_planes(mode, dA), st.split_planes(mode, dB)
    st.assert_unchanged(dA, sA, 'A (split)')
    dD = st.carve_as(C0, vC, SENT)
    sD = st.snapshot(dD)
    st.gemm_planes(mode, pa, pb, dD, K, alpha=0.5, beta=1.0, lower_only=lower)
    got = _np(dD)
    st.assert_padding_untouched(dD, sD, 'C (planes, beta = 1) ' + layout[0])
    want = 0.5 * ref + C0
    e2 = float(((np.abs(got - want) / (scale + 0.5 * np.abs(C0))) * msk).max())
    assert e2 < (4e-7 if mode == 'f32x3' else 2e-6), e2
    if lower:
        assert np.array_equal(dD.cpu().numpy()[up].view(np.int32), C0[up].view(np.int32))


# ================================================================================= mxf_potrf / mxf_trsm / mxf_trtri / mxf_sumlogdiag
# Plan form per n (chol_plan.h potrf_plan): ragged n -> potrf_panel_kernel per 64 columns + gemm updates on sub-blocks A + r0 lda + k0
# (65: two panels, 200: four); float64 192 -> potrf_tiles_kernel, one launch; float64 1536 -> potrf_tiles_kernel per 512-column outer panel
# + trailing gemm (LDS-DMA when the sub-block pointers, lda and stride allow it: not with lead1 / ld+3 / gap5); float64 1024: two outer
# panels; float32 (192, 1024, 1536): the column form.  All chol.hip kernels index element-wise, so an offset base is safe in them; the
# gemm calls choose their loaders from the sub-block's alignment.  trsm: solve_cols_kernel + gemm updates; trtri: trtri_diag_kernel + the
# merge products (temporaries in the upper mirror blocks INSIDE the output window) + zero_upper_kernel.
CHOL_SHAPES = [(3, 65), (1, 200), (2, 192), (2, 1024), (1, 1536)]
CHOL_VARIANTS = ['ld+8', 'ld+3', 'lead1', 'gap5', 'lead1+ld8']


def _spd(rng, S, n):
    A = rng.randn(S, n, n)
    return A @ np.swapaxes(A, 1, 2) / n + np.eye(n)[None]


@functools.lru_cache(maxsize=2)
def _chol_data(S, n):
    rng = np.random.RandomState(n)
    A = _spd(rng, S, n)
    L = np.linalg.cholesky(A)
    return A, L, np.linalg.inv(L), {nrhs: rng.randn(S, n, nrhs) for nrhs in (1, 3, 300)}


@pytest.mark.parametrize('variant', CHOL_VARIANTS)
@pytest.mark.parametrize('S,n', CHOL_SHAPES)
@pytest.mark.parametrize('dtype,tol', [(F64, 1e-11), (F32, 2e-4)])
def test_chol_family_layouts(dtype, tol, S, n, variant):
    """Tolerances of test_potrf_trsm_trtri_logdet.  `variant` lays out A / L; the right-hand sides and the inverse take the next one."""
    other = CHOL_VARIANTS[(CHOL_VARIANTS.index(variant) + 1) % len(CHOL_VARIANTS)]
    A, Lref, Liref, rhs = _chol_data(S, n)
    dA = st.carve_as(A, variant, SENT, dtype=dtype)
    sA = st.snapshot(dA)
    info = st.potrf(dA)
    Lh = _np(dA)
    st.assert_padding_untouched(dA, sA, 'A in place (right of column n, between samples) ' + variant)
    assert int(info.abs().sum()) == 0
    assert np.allclose(Lh, Lref, rtol=tol, atol=tol)
    assert np.all(np.triu(Lh, 1) == 0)
    dL = st.carve_as(Lref, variant, NAN, dtype=dtype)
    sL = st.snapshot(dL)
    sld = _np(st.sumlogdiag(dL))
    assert np.allclose(sld, np.log(np.diagonal(Lref, axis1=1, axis2=2)).sum(-1), rtol=tol, atol=tol * n)
    for nrhs in (1, 3, 300):
        for tr in (False, True):
            ref = np.linalg.solve(np.swapaxes(Lref, 1, 2) if tr else Lref, rhs[nrhs])
            dB = st.carve_as(rhs[nrhs], other, SENT, dtype=dtype)
            sB = st.snapshot(dB)
            st.trsm(dL, dB, tr)
            X = _np(dB)
            st.assert_padding_untouched(dB, sB, 'B nrhs=%d tr=%d %s' % (nrhs, tr, other))
            assert np.allclose(X, ref, rtol=tol * 10, atol=tol * 10 * np.abs(ref).max()), (nrhs, tr)
    # L shared by two right-hand-side samples (stride 0), B gapped: every nrhs, both transposes
    dL1 = st.carve_as(Lref[:1], variant, NAN, dtype=dtype)
    rng2 = np.random.RandomState(n + 1)
    for nrhs in (1, 3, 300):
        B2 = rng2.randn(2, n, nrhs)
        for tr in (False, True):
            ref = np.linalg.solve(np.swapaxes(Lref[:1], 1, 2) if tr else Lref[:1], B2)
            dB = st.carve_as(B2, 'gap5+ld8', SENT, dtype=dtype)
            sB = st.snapshot(dB)
            st.trsm(dL1, dB, tr)
            X = _np(dB)
            st.assert_padding_untouched(dB, sB, 'B (L stride 0) nrhs=%d tr=%d' % (nrhs, tr))
            assert np.allclose(X, ref, rtol=tol * 10, atol=tol * 10 * np.abs(ref).max()), (nrhs, tr)
    # the inverse into a window of uninitialised (NaN) memory
    dI = st.carve_as(np.full_like(Lref, np.nan), other, SENT, dtype=dtype)
    sI = st.snapshot(dI)
    st.trtri(dL, dI)
    Li = _np(dI)
    st.assert_padding_untouched(dI, sI, 'Linv ' + other)
    st.assert_unchanged(dL, sL, 'L')
    assert np.allclose(Li, Liref, rtol=tol * 10, atol=tol * 10)


# Two plan branches of potrf_plan no other test reaches, on plain contiguous inputs (tolerances of test_potrf_trsm_trtri_logdet):
@pytest.mark.parametrize('dtype,tol', [(F64, 1e-11), (F32, 2e-4)])
def test_potrf_ragged_n_with_look_ahead(dtype, tol):
    """n = 2100: ragged (column form, potrf_panel_kernel per 64 columns) AND n >= 2048, so the trailing updates of the ragged outer panels
    are split between the caller's stream and the auxiliary one (look-ahead)."""
    from mxfusion_amd import ops
    S, n = 1, 2100
    A = _spd(np.random.RandomState(n), S, n)
    Lref = np.linalg.cholesky(A)
    L, info = ops.potrf_(torch.as_tensor(A, dtype=dtype).cuda())
    Lh = _np(L)
    assert int(info.abs().sum()) == 0
    assert np.allclose(Lh, Lref, rtol=tol, atol=tol)
    assert np.all(np.triu(Lh, 1) == 0)
    sld = _np(ops.sumlogdiag(L))
    assert np.allclose(sld, np.log(np.diagonal(Lref, axis1=1, axis2=2)).sum(-1), rtol=tol, atol=tol * n)


def test_potrf_f64_more_block_rows_than_cus_falls_back_to_columns():
    """float64, n % 64 == 0, but (n / 64) S workgroups of the tile kernel would not be resident at once: S = 9, n = 2048 -> 288 block rows
    on a 256-CU device -> the column form with look-ahead."""
    from mxfusion_amd import ops
    S, n, tol = 9, 2048, 1e-11
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if (n // 64) * S <= ncu:
        pytest.skip('%d CUs hold the %d block rows of this batch: the tile kernel takes it, the fallback does not engage' % (ncu, (n // 64) * S))
    A = _spd(np.random.RandomState(7), S, n)
    Lref = np.linalg.cholesky(A)
    L, info = ops.potrf_(torch.as_tensor(A).cuda())
    Lh = _np(L)
    assert int(info.abs().sum()) == 0
    assert np.allclose(Lh, Lref, rtol=tol, atol=tol)
    assert np.all(np.triu(Lh, 1) == 0)
    sld = _np(ops.sumlogdiag(L))
    assert np.allclose(sld, np.log(np.diagonal(Lref, axis1=1, axis2=2)).sum(-1), rtol=tol, atol=tol * n)


# =================================================================================================================== mxf_gram / gram2
# gram_plan.h gram_plan: vec_ok = ldk % VEC == 0 and sK % VEC == 0 and K_out 16-byte aligned (VEC = 4 floats / 2 doubles).
#   WRITE, vec_ok, N2 % VEC == 0 -> LEAN / LEAN_XF: gram_lean_kernel (16-byte non-temporal stores; float32 RBF: TRC = 12, float64 RBF: XF form, else run-time rows)
#   otherwise                   -> COORD_SLOW: gram_kernel<T, QT, KIND, false>: 16-byte stores for the lanes with col0 + VEC <= N2 when vecst, element-wise else;
#                                  ACC_ADD / ACC_MUL read the window's old contents
#   Q > 16                      -> gram_generic_kernel (one element per thread)
# N2 = 1028 is a multiple of both vector widths, 1031 of neither.
KINDS = {'rbf': (0, O.RBF), 'matern52': (3, O.Matern52), 'matern32': (2, O.Matern32), 'matern12': (1, O.Matern12)}
GRAM_CASES = [(130, 1028, 8, 2, 1), (130, 1031, 5, 2, 2), (33, 70, 20, 2, 2), (300, None, 8, 2, None)]
GRAM_LAYOUTS = [('K:ld+8', 'ld+8', 'plain'), ('K:ld+3', 'ld+3', 'plain'), ('K:lead1', 'lead1', 'plain'), ('K:gap5', 'gap5', 'plain'),
                ('K:gap5+ld8', 'gap5+ld8', 'plain'), ('X,X2:gap5', 'plain', 'gap5')]


def _oracle_K(kind, X, X2, ls, var, ard):
    k = KINDS[kind][1](X.shape[-1], ARD=ard)
    return k.K(O.T(X), None if X2 is None else O.T(X2), **{k.name + '_lengthscale': O.T(ls), k.name + '_variance': O.T(var)}).numpy()


def _flat(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


@pytest.mark.parametrize('layout', GRAM_LAYOUTS, ids=[l[0] for l in GRAM_LAYOUTS])
@pytest.mark.parametrize('N,N2,Q,S,SX2', GRAM_CASES)
@pytest.mark.parametrize('kind', ['rbf', 'matern52'])
@pytest.mark.parametrize('dtype,tol', [(F64, 1e-11), (F32, 1e-5)])
def test_gram_layouts(dtype, tol, kind, N, N2, Q, S, SX2, layout):
    """Tolerance of test_gram_shapes_vs_oracle (rtol = tol, atol = tol max(variance)), for WRITE into a NaN window, ACC_ADD and ACC_MUL into a
    window holding K0, and -- square Gram -- diag_add + jitter on the window's diagonal."""
    _, vK, vX = layout
    rng = np.random.RandomState(N + (N2 or 0) + Q)
    r = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == F32 else (lambda a: a)
    X = r(rng.uniform(-3, 3, (S, N, Q)))
    X2 = None if N2 is None else r(rng.uniform(-3, 3, (SX2, N2, Q)))       # SX2 == 1: X2 shared by the samples (stride 0)
    ard = Q % 2 == 1 or Q == 8
    ls, var = r(rng.rand(1, Q if ard else 1) * 2 + 0.7), r(rng.rand(1, 1) + 0.5)
    noise = r(rng.rand(S, 1) + 0.1)
    ref = _oracle_K(kind, X, X2, ls, var, ard)
    jit = 1e-3 if N2 is None else 0.0
    if N2 is None:
        ref = ref + np.eye(N)[None] * (noise[:, :, None] + jit)
    K0 = r(rng.uniform(0.5, 1.5, ref.shape))
    dX = st.carve_as(X, vX, NAN, dtype=dtype)                               # the per-sample (N, Q) block stays contiguous: the contract
    dX2 = None if X2 is None else st.carve_as(X2, vX, NAN, dtype=dtype)
    dls, dvar, dnoise = _flat(ls, dtype), _flat(var, dtype), (_flat(noise, dtype) if N2 is None else None)
    for mode, init, want in ((0, np.full_like(ref, np.nan), ref), (1, K0, K0 + ref), (2, K0, K0 * ref)):
        dK = st.carve_as(init, vK, SENT, dtype=dtype)
        sK = st.snapshot(dK)
        st.gram(KINDS[kind][0], dX, dX2, dls, dvar, ard, dK, diag_add=dnoise, jitter=jit, mode=mode)
        got = _np(dK)
        st.assert_padding_untouched(dK, sK, 'K_out mode %d %s' % (mode, layout[0]))
        assert np.allclose(got, want, rtol=tol, atol=tol * float(var.max())), mode


GRAM2_CASES = [(50, 31, 4), (129, None, 8), (33, 300, 12)]      # N2 = 31: ragged for both vector widths; 300: a multiple of both; square 129


@pytest.mark.parametrize('layout', GRAM_LAYOUTS, ids=[l[0] for l in GRAM_LAYOUTS])
@pytest.mark.parametrize('N,N2,Q', GRAM2_CASES)
@pytest.mark.parametrize('k1,k2', [('rbf', 'matern52'), ('matern32', 'matern12')])
@pytest.mark.parametrize('dtype,tol', [(F64, 1e-12), (F32, 3e-6)])
def test_gram2_layouts(dtype, tol, k1, k2, N, N2, Q, layout):
    """gram2_kernel: 16-byte stores when ldk % VEC == 0 and the SAMPLE's base K_out + s sK is aligned, element-wise otherwise; never reads K_out
    (the window holds NaN).  Bounds of test_gram2_two_kernel_epilogue_vs_oracle."""
    _, vK, vX = layout
    rng = np.random.RandomState(N + Q)
    S = 2
    r = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == F32 else (lambda a: a)
    X = r(rng.uniform(-2, 2, (S, N, Q)))
    X2 = None if N2 is None else r(rng.uniform(-2, 2, (1, N2, Q)))
    ls1, var1 = r(rng.rand(S, Q) + 0.5), r(rng.rand(1, 1) + 0.5)
    ls2, var2 = r(rng.rand(1, 1) + 0.5), r(rng.rand(S, 1) + 0.5)
    dadd = r(rng.rand(S, 1)) if N2 is None else None
    r1, r2 = _oracle_K(k1, X, X2, ls1, var1, True), _oracle_K(k2, X, X2, ls2, var2, False)
    dX = st.carve_as(X, vX, NAN, dtype=dtype)
    dX2 = None if X2 is None else st.carve_as(X2, vX, NAN, dtype=dtype)
    for op, ref in ((1, r1 + r2), (2, r1 * r2)):
        if N2 is None:
            ref = ref + np.eye(N)[None] * (dadd[:, :, None] + 1e-3)
        dK = st.carve_as(np.full_like(ref, np.nan), vK, SENT, dtype=dtype)
        sK = st.snapshot(dK)
        st.gram2(KINDS[k1][0], KINDS[k2][0], op, dX, dX2, _flat(ls1, dtype), _flat(var1, dtype), True, _flat(ls2, dtype), _flat(var2, dtype), False,
                 dK, diag_add=None if dadd is None else _flat(dadd, dtype), jitter=1e-3 if N2 is None else 0.0)
        got = _np(dK)
        st.assert_padding_untouched(dK, sK, 'K_out op %d %s' % (op, layout[0]))
        err = np.abs(got - ref)
        assert np.isfinite(err).all()
        if N2 is None:      # (the Matern diagonal: clipped r^2, equal to ~1e-7 only -- see test_gram2_two_kernel_epilogue_vs_oracle)
            d = np.arange(N)
            assert err[:, d, d].max() <= 1e-6 * np.abs(ref).max(), op
            err[:, d, d] = 0
        assert err.max() <= tol * max(1.0, np.abs(ref).max()), op


# ================================================================================================================== mxf_gram_bwd
# gram_bwd.hip reads dK element-wise at dK + s strideS_dK + row lddk + col in every kernel it dispatches to.
@pytest.mark.parametrize('variant', ['ld+8', 'ld+3', 'lead1', 'gap5', 'gap5+ld8'])
@pytest.mark.parametrize('N,N2,Q,S,ard', [(70, 300, 8, 2, True), (130, None, 5, 2, False), (33, 700, 1, 1, True)])
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('dtype,tol', [(F64, 1e-9), (F32, 2e-4)])
def test_gram_bwd_layouts(dtype, tol, kind, N, N2, Q, S, ard, variant):
    """Tolerance of test_gram_bwd_vs_autograd: rtol = tol, atol = tol max(1, max |ref|)."""
    rng = np.random.RandomState(N + Q)
    r = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == F32 else (lambda a: a)
    X = r(rng.uniform(-2, 2, (S, N, Q)))
    X2 = None if N2 is None else r(rng.uniform(-2, 2, (1, N2, Q)))
    ls, var = r(rng.rand(1, Q if ard else 1) + 0.8), r(rng.rand(1, 1) + 0.5)
    dK = r(rng.randn(S, N, N if N2 is None else N2))
    k = KINDS[kind][1](Q, ARD=ard)
    tX, tls, tvar = [O.T(a).clone().requires_grad_(True) for a in (X, ls, var)]
    tX2 = None if X2 is None else O.T(X2).clone().requires_grad_(True)
    (k.K(tX, tX2, **{k.name + '_lengthscale': tls, k.name + '_variance': tvar}) * O.T(dK)).sum().backward()
    refs = (tX.grad, None if tX2 is None else tX2.grad, tls.grad, tvar.grad)
    if kind == 'matern12' and Q == 1:      # refereed by the difference-form closed form, as in test_gram_bwd_vs_autograd
        import _gram_ref
        g, _ = _gram_ref.gram_bwd_ref(kind, X, X2, ls, var, dK, dtype=_gram_ref.HI)
        refs = [None if g[n] is None else torch.as_tensor(g[n].astype(np.float64)) for n in ('dX', 'dX2', 'dls', 'dvar')]
    ddK = st.carve_as(dK, variant, NAN, dtype=dtype)
    sdK = st.snapshot(ddK)
    out = st.gram_bwd(KINDS[kind][0], _flat(X, dtype), None if X2 is None else _flat(X2, dtype), _flat(ls, dtype), _flat(var, dtype), ard, ddK)
    st.assert_unchanged(ddK, sdK, 'dK')
    for got, ref, name in zip(out, refs, ('dX', 'dX2', 'dls', 'dvar')):
        if ref is None:
            assert got is None
            continue
        rr = ref.numpy()
        assert np.allclose(_np(got), rr, rtol=tol, atol=tol * max(1., np.abs(rr).max())), name


# ==================================================================================================================== mxf_coldot
# elementwise.hip: S N < 16384 and M >= 64 -> coldot_small_kernel (16 columns per workgroup), else coldot_kernel (a thread per column).
COLDOT_LAYOUTS = [('A:ld+8', 'ld+8', 'plain', 0), ('A:ld+3', 'ld+3', 'plain', 0), ('A:lead1', 'lead1', 'plain', 0), ('A:gap5', 'gap5', 'plain', 0),
                  ('B:ld+8', 'plain', 'ld+8', 0), ('B:ld+3', 'plain', 'ld+3', 0), ('B:lead1', 'plain', 'lead1', 0), ('B:gap5', 'plain', 'gap5', 0),
                  ('A:stride0,B:gap5+ld8', 'ld+3', 'gap5+ld8', 1), ('B:stride0,A:gap5+ld8', 'gap5+ld8', 'ld+3', 2)]


@pytest.mark.parametrize('layout', COLDOT_LAYOUTS, ids=[l[0] for l in COLDOT_LAYOUTS])
@pytest.mark.parametrize('S,M,N', [(2, 1000, 64), (3, 70, 5), (2, 64, 8200)])
@pytest.mark.parametrize('dtype', [F64, F32])
def test_coldot_layouts(dtype, S, M, N, layout):
    """Tolerance of test_coldot_shapes: rtol = tol, atol = tol max |ref|, tol = 1e-12 / 2e-5."""
    _, vA, vB, shared = layout
    rng = np.random.RandomState(S + M + N)
    r = (lambda a: a.astype(np.float32).astype(np.float64)) if dtype == F32 else (lambda a: a)
    A, B = r(rng.randn(1 if shared == 1 else S, M, N)), r(rng.randn(1 if shared == 2 else S, M, N))
    dA, dB = st.carve_as(A, vA, NAN, dtype=dtype), st.carve_as(B, vB, NAN, dtype=dtype)
    sA, sB = st.snapshot(dA), st.snapshot(dB)
    got = _np(st.coldot(dA, dB))
    st.assert_unchanged(dA, sA, 'A')
    st.assert_unchanged(dB, sB, 'B')
    ref = (A * B).sum(-2)
    tol = 1e-12 if dtype == F64 else 2e-5
    assert got.shape == (S, N)
    assert np.allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())
