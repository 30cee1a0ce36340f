// Internal (non-exported) typed launchers shared between translation units of libmxf_gp.so.
#pragma once
#include "common.h"
#include "gemm_plan.h"      // MXF_TRI_*
#include "svgp_plan.h"

void mxf_comm_release(mxf_ctx* h);      // comm.hip: destroys the handle's RCCL communicator, if any

// C = alpha op(A) op(B) + beta C (gemm.hip; row-major).  A plain descriptor (an aggregate, every member defaulted): a call site names what it
// passes, in declaration order, and omits what is default.
struct MxfMat  { const void* p = nullptr; int64_t ld = 0, stride = 0; };   // stride: per batch entry, 0 = shared
struct MxfMatW { void* p = nullptr;       int64_t ld = 0, stride = 0; };
struct MxfGemm {
    int dtype = 0, ta = 0, tb = 0;
    int64_t M = 0, N = 0, K = 0;
    double alpha = 1.0; MxfMat A, B; double beta = 0.0; MxfMatW C;
    int batch = 1;
    int lower_only = 0;        // square output: skip blocks / entries strictly above the diagonal (syrk-style update)
    int reserve_cus = 0;       // CUs left to the kernels of other streams (sizes the split-K grid)
    int tri = MXF_TRI_NONE;    // the caller vouches: MXF_TRI_UPPER, op(A) = A^T of a lower-triangular A (counts only with ta); MXF_TRI_LOWER, op(A) = A itself,
                               // lower triangular (only without ta); the k loops then skip the zero part
};
int mxf_gemm_internal(mxf_ctx* h, hipStream_t st, const MxfGemm& d);

// The Cholesky family (chol.hip), the same kind of descriptor: S matrices of n x n; mxf_potrf / mxf_trsm / mxf_trtri / mxf_sumlogdiag of
// include/mxf_gp.h document the operands.
struct MxfPotrf {
    int dtype = 0, S = 1; int64_t n = 0;
    MxfMatW A;                  // factored in place
    int* info = nullptr;
    bool zero_upper = true;     // false: leave the strict upper triangle outside the 64 x 64 diagonal blocks as it was (callers that only read the lower part)
    bool zero_info = true;      // false: the caller has zeroed `info` already (the SVGP composite clears its status words in one launch off the critical path)
    // optional (float64, S = 1, large n): L^-1 is formed into this n x n buffer NEXT TO the factorisation, row block by row block on a third
    // stream; *inv_done says whether it was -- if not, the caller runs mxf_trtri_internal as before
    MxfMatW Linv; bool* inv_done = nullptr;
};
struct MxfTrsm { int dtype = 0, transpose = 0, S = 1; int64_t n = 0, nrhs = 0; MxfMat L; MxfMatW B; };      // B (n x nrhs) <- op(L)^-1 B
struct MxfTrtri { int dtype = 0, S = 1; int64_t n = 0; MxfMat L; MxfMatW Linv; };
struct MxfSumLogDiag { int dtype = 0, S = 1; int64_t n = 0; MxfMat L; void* out = nullptr; };               // out[s] = sum_i log |L_s[i][i]|
int mxf_potrf_internal(mxf_ctx* h, hipStream_t st, const MxfPotrf& d);
int mxf_trsm_internal(mxf_ctx* h, hipStream_t st, const MxfTrsm& d);
int mxf_trtri_internal(mxf_ctx* h, hipStream_t st, const MxfTrtri& d);
int mxf_sumlogdiag_internal(mxf_ctx* h, hipStream_t st, const MxfSumLogDiag& d);

// K = k(X, X2) for S samples (gram.hip), the same kind of descriptor; mxf_gram of include/mxf_gp.h documents the operands.
struct MxfGram {
    int kind = 0, dtype = 0;
    int S = 1; int64_t N = 0, N2 = 0; int Q = 0;        // S samples of an (N x N2) Gram over Q coordinates
    const void* X = nullptr; int64_t sX = 0;            // (N x Q); the s* members are per-sample strides in elements, 0 = shared by the samples
    const void* X2 = nullptr; int64_t sX2 = 0;          // (N2 x Q); nullptr: the square Gram of X with itself (N2 is ignored)
    const void* ls = nullptr; int ard = 0; int64_t sls = 0; const void* var = nullptr; int64_t svar = 0;
    const void* diag_add = nullptr; int64_t sdiag = 0; double jitter = 0.0;      // square Gram only: K[i][i] += diag_add[s] + jitter
    int mode = MXF_WRITE;
    MxfMatW K;
};
int mxf_gram_internal(mxf_ctx* h, hipStream_t st, const MxfGram& d);

// The Gram reverse passes take plain descriptors (aggregates, every member defaulted, as the split GEMMs' below): a call site names what it passes.
// Plain reverse mode of a stationary Gram (gram_bwd.hip): dK -> dX, dX2, dls, dvar, all ACCUMULATED into; outputs may be nullptr.
struct MxfGramBwd {
    int kind = 0, dtype = 0;
    int S = 1; int64_t N = 0, N2 = 0; int Q = 0;        // S samples of an (N x N2) Gram over Q coordinates
    const void* X = nullptr; int64_t sX = 0;            // (N x Q); the s* members are per-sample strides in elements, 0 = shared by the samples
    const void* X2 = nullptr; int64_t sX2 = 0;          // (N2 x Q); nullptr: the square Gram of X with itself (N2 is ignored, both roles flow into dX)
    const void* ls = nullptr; int ard = 0; int64_t sls = 0; const void* var = nullptr; int64_t svar = 0;
    const void* dK = nullptr; int64_t lddk = 0, sdK = 0;
    void* dX = nullptr; void* dX2 = nullptr; void* dls = nullptr; void* dvar = nullptr;
    bool dk_symmetric = false;      // square case only: the caller vouches that dK is symmetric -- the row-side sums are skipped and the column side counts twice
};
int mxf_gram_bwd_internal(mxf_ctx* h, hipStream_t st, const MxfGramBwd& d);

// SVGP-fused reverse pass over Text = [H0; w^T] Kuf_all (rows 0..M-1: T, rows M..M+P-1: U), which never materialises dKuf.  dXall is WRITTEN
// (not accumulated); dZ, dls, dvar, R, scal are accumulated into (the caller zeroes them); dY is written or (dY_shared) accumulated.
struct MxfSvgpBwd {
    int kind = 0, dtype = 0;
    int64_t M = 0, SB = 0, B = 0; int Q = 0, P = 0;     // M inducing points, SB = samples x B columns, P outputs
    const void* Z = nullptr; const void* Xall = nullptr; const void* ls = nullptr; int ard = 0; const void* var = nullptr; const void* Text = nullptr;
    const void* Y = nullptr; int64_t sY = 0;            // (B x P) per sample, sample stride sY (0: shared)
    const void* w = nullptr; const void* noise = nullptr; double a1 = 0.0; void* dZ = nullptr; void* dXall = nullptr; void* dls = nullptr; void* dvar = nullptr;
    void* dY = nullptr; int dY_shared = 0; void* R = nullptr; double* scal = nullptr;
    int t_blocked = 0;              // T in 16-column blocks, element (m, n) at ((n / 16) * M + m) * 16 + n % 16 (mxf_gemm_split_internal's blocked output)
    // h0max: bit pattern of max |H0| when T = H0 Kuf came from the f16x2 split GEMM -- the operand bound that lets the matrix-pipe pass
    // accumulate its weights as hi + lo f16; nullptr: float32 accumulation.  tmax: bit pattern of max |T| if the GEMM reported it (word != 0): the tight bound
    const unsigned* h0max = nullptr; const unsigned* tmax = nullptr;
};
// true if mxf_svgp_bwd_fused_internal takes the matrix-pipe pass (svgp_bwd_mfma.hip) for these arguments, not the difference-form one of gram_bwd.hip
bool mxf_svgp_bwd_is_mfma(int kind, int dtype, int64_t SB, int64_t B, int Q, int P, const void* Text);
bool mxf_svgp_bwd_reads_blocked(int kind, int dtype, int64_t SB, int64_t B, int Q, int P, const void* Text);
int mxf_svgp_bwd_fused_internal(mxf_ctx* h, hipStream_t st, const MxfSvgpBwd& d);
int mxf_svgp_bwd_mfma_internal(mxf_ctx* h, hipStream_t st, const MxfSvgpBwd& d);      // svgp_bwd_mfma.hip; the caller has asked mxf_svgp_bwd_is_mfma

// f32-accurate GEMM on the bf16 matrix pipe (three-term bf16 splitting, gemm_split.hip)
size_t mxf_split_plane_elems(int64_t R, int64_t K);    // elements (bf16) of ONE plane of an (R x K) operand
// operand formats of the split GEMM (gemm_split.hip): three bf16 terms / two scaled f16 terms
#define MXF_SPLIT_BF16X3 0
#define MXF_SPLIT_F16X2 1
int mxf_maxabs_internal(mxf_ctx* h, int64_t R, int64_t K, const float* x, int64_t ld, unsigned* out, hipStream_t st, bool zero = true);   // out[0] = bit pattern of max |x| (zero = false: the caller cleared the word)
int mxf_split_planes_internal(mxf_ctx* h, int64_t R, int64_t K, const float* X, int64_t ld, unsigned short* planes, hipStream_t st,
                              int mode = MXF_SPLIT_BF16X3, const unsigned* maxbits = nullptr);
// The split GEMMs take plain descriptors (aggregates, every member defaulted): a call site names each optional thing it passes.
struct MxfPlanes {                          // one split operand
    const unsigned short* p = nullptr;      // its planes, element (r, k) at ((k / 16) * R + r) * 16 + k % 16
    int64_t stride = 0;                     // plane stride in elements
    const unsigned* maxbits = nullptr;      // f16x2 operand split with the scale of this max-abs word (mxf_maxabs_internal): the epilogue divides by it
};                                          //   (nullptr: bf16x3, or a scale the caller folds into alpha / ad0, e.g. Gram planes k / variance * 2^14)
struct MxfSplitScale { double alpha = 1.0; const float* ad0 = nullptr; int pow0 = 0; };      // the product times alpha * ad0[0]^pow0 (ad0: device scalar)
struct MxfSplitSched { int reserve_cus = 0; };      // CUs the launch leaves to work on other streams
struct MxfSplitOut {                        // ONE of: C (row-major, or in 16-column blocks) / planes
    // lower_only: square output, only tiles / entries on or below the diagonal; blocked: element (m, n) at ((n / 16) * M + m) * 16 + n % 16 (ldc == N)
    float* C = nullptr; int64_t ldc = 0; double beta = 0.0; int lower_only = 0, blocked = 0;
    unsigned* maxout = nullptr;             // raised (atomicMax) to the bit pattern of max |C| by the kernels whose plain store path supports it; others leave it untouched
    // the product as two f16 planes (hi + lo of alpha * A B^T) in the layout of an (M x K' = N) operand, ((n / 16) * M + m) * 16 + n % 16
    unsigned short* planes = nullptr; int64_t pstride = 0;
    int a_lower = 0;                        // (planes only) A is lower triangular: the k loop of a row tile stops at its last row
    // (planes only) ALSO in the transposed orientation, ((m / 16) * N + n) * 16 + m % 16; with avec (M floats) / Upart ((M / 128) x N floats): per
    // 128-row band the sums of avec[m] * (hi + lo)(m, n), in the planes' units -- deterministic, summed by the caller (mxf_upart_reduce_internal)
    unsigned short* planes_t = nullptr; int64_t pstride_t = 0; const float* avec = nullptr; float* Upart = nullptr;
};
// C (M x N) = alpha * A (M x K) B (N x K)^T + beta * C  (gemm_split.hip); mode: the operand format of both
int mxf_gemm_split_internal(mxf_ctx* h, hipStream_t st, int mode, int64_t M, int64_t N, int64_t K, MxfSplitScale scale, MxfPlanes A, MxfPlanes B,
                            MxfSplitOut out, MxfSplitSched sched = {});
// gemm_bt.hip (r06): the same product, f16x2, with the second operand stored K-MAJOR -- C (M x N) = alpha * ad0[0] / scales * A (M x K) Bt (K x N),
// Bt = the planes of the (btR >= K rows, k' = N) operand, element (k, n) at ((n / 16) * btR + k) * 16 + n % 16: the T product of the SVGP step
// reads the SAME Kuf planes as Psi2.  scale.pow0 is 0 or 1; out: C or blocked C with maxout, beta == 0, a full product.
// optional row U[n] = uscale * ad0[0] / scale(Bt) * sum_k w[k] Bt[k][n]; wscratch: 2 K halves + one word, caller-owned
struct MxfBtURow { const float* w = nullptr; float* U = nullptr; double uscale = 1.0; void* wscratch = nullptr; };
bool mxf_gemm_bt_ok(int64_t M, int64_t N, int64_t K);
int mxf_gemm_bt_internal(mxf_ctx* h, hipStream_t st, int64_t M, int64_t N, int64_t K, MxfSplitScale scale, MxfPlanes A, MxfPlanes Bt, int64_t btR,
                         MxfSplitOut out, MxfBtURow u = {}, MxfSplitSched sched = {});
// Gram matrix cov(Xmin[r], Xmaj[k]) (r < R, k < Kn) as two f16 planes (float32 inputs, stationary kernels; gram.hip), plane element (r, k) at
// ((k / 16) * R + r) * 16 + k % 16
struct MxfGramPlanes {
    int kind = 0; int64_t R = 0, Kn = 0; int Q = 0;
    const float* Xmin = nullptr; const float* Xmaj = nullptr; const float* ls = nullptr; int ard = 0; const float* var = nullptr;
    unsigned short* planes = nullptr; int64_t pstride = 0;      // 2 * pstride elements, pstride = mxf_split_plane_elems(R, Kn)
    float* scratch = nullptr;                                   // mxf_gram_planes_scratch_bytes() bytes, caller-owned: two of these run concurrently on different streams
    // optional fused product U[p][r] = sum_k w[k][p] cov(Xmin[r], Xmaj[k]): w (Kn x Pw), U (Pw x ldU); see gram_planes_lean_kernel
    const float* w = nullptr; int Pw = 0; float* U = nullptr; int64_t ldU = 0;
    // optional per-row weights (period entries, index taken modulo period) on the major / minor index
    const float* majs = nullptr; const float* mins = nullptr; int64_t period = 1;
};
size_t mxf_gram_planes_scratch_bytes(int64_t R, int64_t Kn, int Q);
int mxf_gram_planes_internal(mxf_ctx* h, hipStream_t st, const MxfGramPlanes& d);

// whiten.hip: two f16 planes of an (R x K) operand -> the planes of its transpose (K x R); U != nullptr: U[k] = scale[0] * sc2 * sum_r a[r] x(r, k)
int mxf_upart_reduce_internal(mxf_ctx* h, int64_t N, int nparts, const float* Upart, const float* scale, float sc2, float* U, hipStream_t st);
int mxf_planes_transpose_internal(mxf_ctx* h, int64_t R, int64_t K, const unsigned short* in, int64_t pin, unsigned short* out, int64_t pout,
                                  const float* a, const float* scale, float sc2, float* U, hipStream_t st);

// One SVGP call (composite.hip), the same kind of descriptor: each entry point names what it passes; mxf_svgp_logpdf, _het and _mat of
// include/mxf_gp.h document the operands.
struct MxfSvgp {
    int kind = MXF_K_RBF, dtype = 0, S = 1; int64_t B = 0, M = 0; int Q = 1, P = 0;
    const void* X = nullptr; int64_t sX = 0; const void* Y = nullptr; int64_t sY = 0; const void* Z = nullptr;
    const void* noise = nullptr; int64_t nrows = 1; int ncols = 1;
    const void* mu = nullptr; const void* W = nullptr; const void* sdiag = nullptr; const void* ls = nullptr; int ard = 0; const void* var = nullptr;
    double jitter = 0.0, scaling = 1.0, gscale = 1.0;
    void* logL = nullptr; int* info = nullptr; int want_grad = 0;
    void* dX = nullptr; void* dY = nullptr; void* dZ = nullptr; void* dnoise = nullptr; void* dmu = nullptr; void* dW = nullptr; void* dSdiag = nullptr;
    void* dls = nullptr; void* dvar = nullptr;
    void* stream = nullptr;
    // optional: the caller's own Grams in place of X, Z and the covariance parameters, and their gradients
    const void* Kuu = nullptr; const void* Kuf = nullptr; const void* Kdiag = nullptr; void* dKuu = nullptr; void* dKuf = nullptr; void* dKdiag = nullptr;
};
// the probe build's Psi2 knobs, read once
inline const SvgpKnobs& mxf_svgp_knobs() {
    static const SvgpKnobs k = {MXF_KNOB("MXF_SVGP_PSI2_KA", -1), (int)MXF_KNOB("MXF_SVGP_PSI2_RA", 148), MXF_KNOB_SET("MXF_SVGP_PSI2_RA"),
                                (int)MXF_KNOB("MXF_SVGP_PSI2_RB", 16), MXF_KNOB_SET("MXF_SVGP_PSI2_RB")};
    return k;
}
