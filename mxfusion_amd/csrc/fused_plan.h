// Grids, chunk sizes, accumulation paths, scratch layouts and refusals of the row-owned launchers (rff.hip, kmv.hip, psi.hip, nearest.hip,
// knn.hip), of the per-row small-matrix launcher vecchia.hip and
// the grid of the per-sample reductions (unidist.h, likelihood.hip, robustmax.hip), as pure functions of the request: plain C++, no HIP,
// checked on the host by tests/host/fused_plan_check.cpp, nearest_plan_check.cpp and vecchia_plan_check.cpp.  The tile sizes are the kernels' own: the
// .hip files read them from here.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mxf_gp.h"      // MXF_PSI_MAX_Q, MXF_RFF_MAX_Q, MXF_KMV_MAX_Q, MXF_KNN_MAX_*, MXF_VECCHIA_MAX_P

constexpr int RFF_RB = 128;         // rows (threads) per workgroup
constexpr int RFF_DCH = 64;         // values of d summed in T between two additions to the double register
constexpr int RFF_JB = 16;          // weights per feature and pass (one scalar load)
constexpr int RFF_JB_SMALL = 4;     // the same for J <= RFF_JB_SMALL
constexpr int RFF_TARGET = 1024;    // workgroups the split of d aims for

constexpr int KMV_RB = 128;         // rows (threads) per workgroup
constexpr int KMV_CH = 64;          // values of n2 summed in T between two additions to the double register
constexpr int KMV_JB = 16;          // columns of V per pair and pass (one scalar load)
constexpr int KMV_JB_SMALL = 4;     // the same for J <= KMV_JB_SMALL
constexpr int KMV_TARGET = 1024;    // workgroups the split of n2 aims for
constexpr int KMV_WG = 64;          // weights of the bilinear form per prep launch (a kernel argument)

constexpr int PSI_TILE = 16;        // pair-owned: a workgroup of 256 threads owns PSI_TILE x PSI_TILE pairs
constexpr int PSI_ROWS = 64;        // pair-owned: rows summed in T between two additions to the double register
constexpr int PSI_RB = 128;         // row-owned Psi2 reverse pass: rows (threads) per workgroup
constexpr int PSI_R1 = 256;         // row-owned Psi1 kernels: rows (threads) per workgroup
constexpr int PSI_MCH = 32;         // row-owned Psi1 kernels: the m of one chunk
constexpr int PSI_TARGET = 2048;    // workgroups the splits aim for
constexpr int PSI_JB = 4;           // row-owned contraction: weight matrices per pass (a pair's PSI_JB weights are one scalar load)

static inline int64_t mxf_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t mxf_clampi(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }
// Q padded to the register tile the row-owned kernels are compiled for
static inline int mxf_qp(int Q) { return Q <= 4 ? 4 : (Q <= 8 ? 8 : 16); }

struct Carver {   // bump allocator over a scratch buffer in 256-byte granules; with a null base it only counts
    char* base; size_t off = 0;
    explicit Carver(void* p) : base((char*)p) {}
    template <typename U> U* take(size_t n) { U* p = base ? (U*)(base + off) : nullptr; off += (n * sizeof(U) + 255) / 256 * 256; return p; }
};
// the byte offset of the next piece: the plans below run their list once over a counting Carver, and the launcher adds the offsets to its allocation
static inline size_t mxf_piece(Carver& cv, size_t bytes) { const size_t at = cv.off; cv.take<char>(bytes); return at; }

// what every plan below starts with.  rc != 0: the call is refused with that code and this text (nothing else in the plan is valid then)
struct FusedRefusal {
    int rc = 0; char refusal[192] = "";
    void refuse(int code, const char* why) { rc = code; snprintf(refusal, sizeof(refusal), "%s", why); }
    __attribute__((format(printf, 3, 4))) void refusef(int code, const char* fmt, ...) {      // the texts that carry numbers
        va_list ap; va_start(ap, fmt); rc = code; vsnprintf(refusal, sizeof(refusal), fmt, ap); va_end(ap);
    }
    void refuse_q(int Q, int limit) { rc = -3; snprintf(refusal, sizeof(refusal), "Q = %d above the limit of %d input dimensions", Q, limit); }
};
static inline bool stride_ok(int64_t ss, int64_t one_sample) { return ss == 0 || ss == one_sample; }

// Grid of the kernels that close each (sample, chunk of rows) pair with ONE atomic into out[s] (univariate_ps_kernel, lik_kernel,
// robustmax_kernel).  The cap on same-address atomics (grid_for_reduce: ~15 ns apiece at the L2) holds PER SAMPLE here, S addresses take them
// in parallel: up to 512 chunks of 256 rows per sample, fewer where S of them would pass 8192 workgroups (32 per CU), and a grid of at most
// 65 536 workgroups that loops over the rest of the pairs.
struct PerSamplePlan { int chunks; unsigned grid; };
static inline PerSamplePlan per_sample_plan(int S, int64_t n) {
    int64_t c = (n + 255) / 256;
    if (c > 512) c = 512;
    const int64_t fit = 8192 / (int64_t)S;
    if (c > fit) c = fit;
    if (c < 1) c = 1;
    int64_t g = (int64_t)S * c;
    if (g > 65536) g = 65536;
    return {(int)c, (unsigned)g};
}

// The reduction axis of R values over grid.y: values per workgroup row (a multiple of `unit`) and the number of such rows -- 1 unless the
// blocks of rb rows of N alone, times S, leave the device with fewer than `target` workgroups
struct ReduceSplit { int64_t ch; int rows; };
static inline ReduceSplit reduce_split(int S, int64_t N, int64_t R, int rb, int unit, int target) {
    const int64_t want = mxf_clampi(mxf_cdiv(target, mxf_cdiv(N, rb) * S), 1, mxf_clampi(mxf_cdiv(R, unit), 1, 65535));
    const int64_t ch = mxf_cdiv(mxf_cdiv(R, want), unit) * unit;
    return {ch, (int)mxf_cdiv(R, ch)};
}

// ---- rff.hip -----------------------------------------------------------------------------------------------------------------------------
struct RffRequest {
    size_t esize = 4; bool bwd = false;
    int S = 0; int64_t N = 0, D = 0; int Q = 0, J = 0;
    int64_t ss_X = 0, ss_Om = 0, ss_ph = 0, ss_W = 0;      // sample strides in elements, 0 = shared
    bool has_X = false, has_Om = false, has_ph = false, has_W = false, has_out = false, has_G = false, has_dX = false;
};
struct RffPlan : FusedRefusal {
    int qp = 0, jb = 0, npass = 0;      // the kernels' <QP, JB>; passes over d of jb weights each
    int64_t ch = 0; int rows = 0;       // values of d per workgroup row, and the rows (grid[1])
    unsigned grid[3] = {1, 1, 1};       // of rff_fwd_kernel / rff_bwd_kernel
    int own_X = 0;
    // what is summed across threads goes through doubles: the forward results under a split of d; the gradient under a split or a shared X.
    // scratch_sum: in zeroed scratch, narrowed or folded once (a float64 gradient is summed in the caller's buffer itself)
    bool summed = false, scratch_sum = false;
    int64_t n_prep = 0, n_out = 0, n_dx = 0;      // items of the prep launch, elements of out and of dX
    int64_t ss_om = 0, ss_ph = 0, ss_wb = 0;      // sample strides of the prepared operands
    size_t at_om = 0, at_ph = 0, at_wb = 0, at_acc = 0, zero_bytes = 0, bytes = 0;      // scratch pieces; [at_acc, at_acc + zero_bytes) is zeroed
};

static inline RffPlan rff_plan(const RffRequest& r) {
    RffPlan p;
    if (r.S < 1 || r.S > 65535 || r.N < 1 || r.D < 1 || r.Q < 1 || r.J < 1) { p.refuse(-2, "1 <= S <= 65535 samples, N, D, Q, J >= 1"); return p; }
    if (r.Q > MXF_RFF_MAX_Q) { p.refuse_q(r.Q, MXF_RFF_MAX_Q); return p; }
    if (r.N > ((int64_t)1 << 31) || r.D > ((int64_t)1 << 24) || r.J > (1 << 16)) { p.refuse(-2, "N <= 2^31, D <= 2^24, J <= 2^16"); return p; }
    if (!r.has_X || !r.has_Om || !r.has_ph || !r.has_W) { p.refuse(-2, "null X, Omega, phase or W"); return p; }
    if (r.bwd ? (!r.has_G || !r.has_dX) : !r.has_out) { p.refuse(-2, r.bwd ? "null G or dX_acc" : "null out"); return p; }
    if (!stride_ok(r.ss_X, r.N * r.Q) || !stride_ok(r.ss_Om, r.D * r.Q) || !stride_ok(r.ss_ph, r.D) || !stride_ok(r.ss_W, r.D * r.J)) {
        p.refuse(-2, "a sample stride must be 0 or the elements of one sample (X: N Q; Omega: D Q; phase: D; W: D J)");
        return p;
    }
    p.qp = mxf_qp(r.Q);
    p.jb = r.J <= RFF_JB_SMALL ? RFF_JB_SMALL : RFF_JB;
    p.npass = (int)mxf_cdiv(r.J, p.jb);
    p.own_X = r.ss_X != 0;
    const int64_t S_om = r.ss_Om ? r.S : 1, S_ph = r.ss_ph ? r.S : 1, S_W = r.ss_W ? r.S : 1;
    const ReduceSplit sp = reduce_split(r.S, r.N, r.D, RFF_RB, RFF_DCH, RFF_TARGET);
    p.ch = sp.ch; p.rows = sp.rows;
    p.grid[0] = (unsigned)mxf_cdiv(r.N, RFF_RB); p.grid[1] = (unsigned)p.rows; p.grid[2] = (unsigned)r.S;
    p.n_out = (int64_t)r.S * r.N * r.J; p.n_dx = (p.own_X ? r.S : 1) * r.N * r.Q;
    p.summed = r.bwd ? (p.rows > 1 || (!p.own_X && r.S > 1)) : p.rows > 1;
    p.scratch_sum = p.summed && !(r.bwd && r.esize == 8);
    p.n_prep = (S_om + S_ph + S_W * p.npass) * r.D;
    p.ss_om = r.ss_Om ? r.D * p.qp : 0; p.ss_ph = r.ss_ph ? r.D : 0; p.ss_wb = r.ss_W ? (int64_t)p.npass * r.D * p.jb : 0;
    Carver cv(nullptr);
    p.at_om = mxf_piece(cv, (size_t)(S_om * r.D) * p.qp * r.esize);
    p.at_ph = mxf_piece(cv, (size_t)(S_ph * r.D) * r.esize);
    p.at_wb = mxf_piece(cv, (size_t)(S_W * p.npass * r.D) * p.jb * r.esize);
    p.zero_bytes = (p.scratch_sum ? (size_t)(r.bwd ? p.n_dx : p.n_out) : 0) * sizeof(double);
    p.at_acc = mxf_piece(cv, p.zero_bytes);
    p.bytes = cv.off;
    return p;
}

// ---- kmv.hip -----------------------------------------------------------------------------------------------------------------------------
struct KmvRequest {
    size_t esize = 4; bool bwd = false;
    int S = 0; int64_t N = 0, N2 = 0; int Q = 0, J = 0, ard = 0;      // N2 is ignored on a square product (no X2)
    int64_t ss_X = 0, ss_X2 = 0, ss_ls = 0, ss_var = 0, ss_da = 0, ss_V = 0, ss_A = 0;
    bool has_X = false, has_X2 = false, has_ls = false, has_var = false, has_da = false, has_V = false, has_out = false, has_A = false, has_w = false,
         has_dls = false, has_dvar = false;
};
struct KmvPlan : FusedRefusal {
    int qp = 0, jb = 0, npass = 0;      // the kernels' <QP, JB>; passes over n2 of jb columns of V each
    bool square = false; int64_t N2 = 0, ss_Z = 0;      // the second operand: X2, or X itself
    int64_t S_z = 1, S_V = 1;           // samples of the prepared operands
    int64_t ch = 0; int rows = 0;       // values of n2 per workgroup row, and the rows (grid[1])
    unsigned grid[3] = {1, 1, 1};       // of kmv_fwd_kernel / kmv_bwd_kernel
    int gp = 0;                         // passes per launch of kmv_prep_v_kernel: all of them, or the KMV_WG weights of the reverse mode
    int64_t n_prep_z = 0, n_out = 0;
    int64_t ss_zs = 0, ss_vb = 0;       // sample strides of the prepared operands
    // zeroed doubles: the forward results under a split of n2; the sums of the reverse mode, (S, QP) then (S) at at_dv
    size_t n_zero = 0;
    size_t at_zs = 0, at_vb = 0, at_zero = 0, at_dv = 0, bytes = 0;
};
// launch of kmv_prep_v_kernel that starts at pass0: its passes and its items
struct KmvPrepV { int np; int64_t items; };
static inline KmvPrepV kmv_prep_v(const KmvPlan& p, int pass0) {
    const int np = (int)mxf_clampi(p.npass - pass0, 1, p.gp);
    return {np, p.S_V * np * p.N2};
}

static inline KmvPlan kmv_plan(const KmvRequest& r) {
    KmvPlan p;
    p.square = !r.has_X2;
    const int64_t N2 = p.N2 = p.square ? r.N : r.N2;
    p.ss_Z = p.square ? r.ss_X : r.ss_X2;
    if (r.S < 1 || r.S > 65535 || r.N < 1 || N2 < 1 || r.Q < 1 || r.J < 1) { p.refuse(-2, "1 <= S <= 65535 samples, N, N2, Q, J >= 1"); return p; }
    if (r.Q > MXF_KMV_MAX_Q) { p.refuse_q(r.Q, MXF_KMV_MAX_Q); return p; }
    if (r.N > ((int64_t)1 << 31) || N2 > ((int64_t)1 << 31) || r.J > (1 << 16)) { p.refuse(-2, "N, N2 <= 2^31, J <= 2^16"); return p; }
    if (!r.has_X || !r.has_ls || !r.has_var || !r.has_V) { p.refuse(-2, "null X, lengthscale, variance or V"); return p; }
    if (r.bwd) {
        if (!r.has_A || !r.has_w) { p.refuse(-2, "null A or w"); return p; }
        if (!r.has_dls && !r.has_dvar) { p.refuse(-2, "null dls_acc and dvar_acc"); return p; }
    } else if (!r.has_out) { p.refuse(-2, "null out"); return p; }
    if (!stride_ok(r.ss_X, r.N * r.Q) || (!p.square && !stride_ok(r.ss_X2, N2 * r.Q)) || !stride_ok(r.ss_ls, r.ard ? r.Q : 1) || !stride_ok(r.ss_var, 1) ||
        (r.has_da && !stride_ok(r.ss_da, 1)) || !stride_ok(r.ss_V, N2 * r.J) || (r.bwd && !stride_ok(r.ss_A, r.N * r.J))) {
        p.refuse(-2, "a sample stride must be 0 or the elements of one sample (X: N Q; X2: N2 Q; lengthscale: Q or 1; variance, diag_add: 1; "
                     "V: N2 J; A: N J)");
        return p;
    }
    p.qp = mxf_qp(r.Q);
    p.jb = r.J <= KMV_JB_SMALL ? KMV_JB_SMALL : KMV_JB;
    p.npass = (int)mxf_cdiv(r.J, p.jb);
    p.S_z = (p.ss_Z || r.ss_ls) ? r.S : 1; p.S_V = r.ss_V ? r.S : 1;
    const ReduceSplit sp = reduce_split(r.S, r.N, N2, KMV_RB, KMV_CH, KMV_TARGET);
    p.ch = sp.ch; p.rows = sp.rows;
    p.grid[0] = (unsigned)mxf_cdiv(r.N, KMV_RB); p.grid[1] = (unsigned)p.rows; p.grid[2] = (unsigned)r.S;
    p.gp = r.bwd ? KMV_WG / p.jb : p.npass;
    p.n_prep_z = p.S_z * N2; p.n_out = (int64_t)r.S * r.N * r.J;
    p.ss_zs = p.S_z > 1 ? N2 * p.qp : 0; p.ss_vb = p.S_V > 1 ? (int64_t)p.npass * N2 * p.jb : 0;
    p.n_zero = r.bwd ? (size_t)r.S * (p.qp + 1) : (p.rows > 1 ? (size_t)p.n_out : 0);
    Carver cv(nullptr);
    p.at_zs = mxf_piece(cv, (size_t)(p.S_z * N2) * p.qp * r.esize);
    p.at_vb = mxf_piece(cv, (size_t)(p.S_V * p.npass * N2) * p.jb * r.esize);
    p.at_zero = mxf_piece(cv, p.n_zero * sizeof(double));
    p.at_dv = p.at_zero + (size_t)r.S * p.qp * sizeof(double);
    p.bytes = cv.off;
    return p;
}

// ---- psi.hip -----------------------------------------------------------------------------------------------------------------------------
// rows of N over grid.y of psi2_pairs_kernel: until PSI_TARGET workgroups exist, at most one chunk per PSI_ROWS rows
static inline int64_t psi_pairs(int64_t M) { const int64_t nt = mxf_cdiv(M, PSI_TILE); return nt * (nt + 1) / 2; }
static inline int psi_pairs_rch(int S, int64_t N, int64_t M) {
    return (int)mxf_clampi(mxf_cdiv(PSI_TARGET, psi_pairs(M) * S), 1, mxf_clampi(mxf_cdiv(N, PSI_ROWS), 1, 65535));
}
// strides over m on grid.y of psi2_bwd_rows_kernel and psi2_quad_rows_kernel: until PSI_TARGET workgroups exist, at most one per m
static inline int psi_rows_mch(int S, int64_t N, int64_t M) {
    return (int)mxf_clampi(mxf_cdiv(PSI_TARGET, mxf_cdiv(N, PSI_RB) * S), 1, mxf_clampi(M, 1, 65535));
}

struct PsiRequest {
    size_t esize = 4;
    int S = 0; int64_t N = 0, M = 0; int Q = 0, ard = 0;
    int64_t ss_mu = 0, ss_s = 0, ss_Z = 0, ss_ls = 0, ss_var = 0;
    bool has_mu = false, has_s = false, has_Z = false, has_ls = false, has_var = false;
    bool has_Psi1 = false, has_Psi2 = false;                                                      // forward
    bool has_G1 = false, has_G2 = false, has_dmu = false, has_ds = false, has_dZ = false, has_dls = false, has_dvar = false;      // reverse
    int J = 0; int64_t ss_A = 0; bool has_A = false, has_R = false;                               // contraction
};
// One struct for the three calls; each plan fills what its launcher reads.  Scratch: z and z / 2 (zf, zh), the rows of psi_prep_kernel, then
// the call's own pieces; [at_zero, at_zero + zero_bytes) is zeroed.  An absent piece has offset 0.
struct PsiPlan : FusedRefusal {
    int qp = 0;
    int64_t n_prep = 0, n_mm = 0;       // items of psi_prep_kernel; S M M: of the mirror / weight kernels
    unsigned grid1[3] = {1, 1, 1};      // psi1_fwd_kernel / psi1_bwd_kernel
    int rch = 1; unsigned grid_pairs[3] = {1, 1, 1};      // psi2_pairs_kernel
    int mch = 1; unsigned grid_rows[3] = {1, 1, 1};       // psi2_bwd_rows_kernel / psi2_quad_rows_kernel
    // reverse: which Psi2 passes run; wide: float32, the three large gradients are summed in scratch doubles and folded (end[]: the segments)
    bool pairs_pass = false, rows_pass = false, wide = false, fold = false, close = false;
    int own_mu = 0, own_s = 0, own_Z = 0, own_l = 0, own_v = 0;
    int64_t n_mu = 0, n_s = 0, n_Z = 0, end[3] = {0, 0, 0};
    int npass = 0; int64_t n_out = 0;   // contraction: passes of PSI_JB weight matrices; elements of R
    bool split = false;                 // contraction: m is split, the results meet in zeroed doubles at at_acc
    size_t at_z = 0, at_zh = 0, at_rows = 0, at_acc = 0, at_wt = 0, at_l2 = 0, at_dv = 0, at_big = 0, at_zero = 0, zero_bytes = 0, bytes = 0;
};

static inline bool psi_refused(const PsiRequest& r, bool quad, PsiPlan& p) {
    if (r.S < 1 || r.S > 65535 || r.N < 1 || r.M < 1 || r.Q < 1) { p.refuse(-2, "1 <= S <= 65535 samples, N, M, Q >= 1"); return true; }
    if (r.Q > MXF_PSI_MAX_Q) { p.refuse_q(r.Q, MXF_PSI_MAX_Q); return true; }
    if (r.M > ((int64_t)1 << 20) || r.N > ((int64_t)1 << 31)) { p.refuse(-2, "M <= 2^20, N <= 2^31"); return true; }
    if (!r.has_mu || !r.has_s || !r.has_Z || !r.has_ls || !r.has_var) { p.refuse(-2, "null mu, s, Z, lengthscale or variance"); return true; }
    if (!stride_ok(r.ss_mu, r.N * r.Q) || !stride_ok(r.ss_s, r.N * r.Q) || !stride_ok(r.ss_Z, r.M * r.Q) || !stride_ok(r.ss_ls, r.ard ? r.Q : 1) ||
        !stride_ok(r.ss_var, 1)) {
        p.refuse(-2, "a sample stride must be 0 or the elements of one sample (mu, s: N Q; Z: M Q; lengthscale: Q or 1; variance: 1)");
        return true;
    }
    if (quad) {
        if (r.J < 1 || !r.has_A || !r.has_R) { p.refuse(-2, "J >= 1 weight matrices, A and R not null"); return true; }
        if (!stride_ok(r.ss_A, (int64_t)r.J * r.M * r.M)) { p.refuse(-2, "the sample stride of A must be 0 or J M M"); return true; }
    }
    return false;
}

// what the three calls share: the register tile, the prep launch, and zf, zh at the head of the scratch
static inline void psi_head(const PsiRequest& r, PsiPlan& p, Carver& cv) {
    p.qp = mxf_qp(r.Q);
    p.n_prep = (int64_t)r.S * (r.N + r.M);
    p.n_mm = (int64_t)r.S * r.M * r.M;
    p.at_z = mxf_piece(cv, (size_t)r.S * r.M * p.qp * r.esize);
    p.at_zh = mxf_piece(cv, (size_t)r.S * r.M * p.qp * r.esize);
}
static inline size_t psi_rows_bytes(const PsiRequest& r, const PsiPlan& p) { return (size_t)r.S * r.N * (2 * p.qp + 2) * r.esize; }
static inline void psi_grid1(const PsiRequest& r, PsiPlan& p) {
    p.grid1[0] = (unsigned)mxf_cdiv(r.N, PSI_R1); p.grid1[1] = (unsigned)mxf_cdiv(r.M, PSI_MCH); p.grid1[2] = (unsigned)r.S;
}
static inline void psi_grid_pairs(const PsiRequest& r, PsiPlan& p) {
    p.rch = psi_pairs_rch(r.S, r.N, r.M);
    p.grid_pairs[0] = (unsigned)psi_pairs(r.M); p.grid_pairs[1] = (unsigned)p.rch; p.grid_pairs[2] = (unsigned)r.S;
}
static inline void psi_grid_rows(const PsiRequest& r, PsiPlan& p) {
    p.mch = psi_rows_mch(r.S, r.N, r.M);
    p.grid_rows[0] = (unsigned)mxf_cdiv(r.N, PSI_RB); p.grid_rows[1] = (unsigned)p.mch; p.grid_rows[2] = (unsigned)r.S;
}

static inline PsiPlan psi_fwd_plan(const PsiRequest& r) {
    PsiPlan p;
    if (psi_refused(r, false, p)) return p;
    Carver cv(nullptr);
    psi_head(r, p, cv);
    psi_grid1(r, p);
    if (r.has_Psi2) {
        psi_grid_pairs(r, p);
        p.at_rows = mxf_piece(cv, psi_rows_bytes(r, p));
        p.zero_bytes = (size_t)p.n_mm * sizeof(double);
        p.at_zero = p.at_acc = mxf_piece(cv, p.zero_bytes);
    }
    p.bytes = cv.off;
    return p;
}

static inline PsiPlan psi_bwd_plan(const PsiRequest& r) {
    PsiPlan p;
    if (psi_refused(r, false, p)) return p;
    Carver cv(nullptr);
    psi_head(r, p, cv);
    p.own_mu = r.ss_mu != 0; p.own_s = r.ss_s != 0; p.own_Z = r.ss_Z != 0; p.own_l = r.ss_ls != 0; p.own_v = r.ss_var != 0;
    p.n_mu = (p.own_mu ? r.S : 1) * r.N * r.Q; p.n_s = (p.own_s ? r.S : 1) * r.N * r.Q; p.n_Z = (p.own_Z ? r.S : 1) * r.M * r.Q;
    p.end[0] = p.n_mu; p.end[1] = p.n_mu + p.n_s; p.end[2] = p.n_mu + p.n_s + p.n_Z;
    p.pairs_pass = r.has_G2 && (r.has_dZ || r.has_dls || r.has_dvar);
    p.rows_pass = r.has_G2 && (r.has_dmu || r.has_ds || r.has_dls);
    p.wide = r.esize == 4;
    p.fold = p.wide && (r.has_dmu || r.has_ds || r.has_dZ);
    p.close = r.has_dls || r.has_dvar;
    psi_grid1(r, p);
    if (p.pairs_pass) { psi_grid_pairs(r, p); p.at_rows = mxf_piece(cv, psi_rows_bytes(r, p)); }
    if (p.rows_pass) { psi_grid_rows(r, p); p.at_wt = mxf_piece(cv, (size_t)p.n_mm * r.esize); }
    // zeroed doubles, back to back: dl2 (S, QP), dvar (S), and for float32 the three large gradients (the segments of one mxf_fold_kernel)
    p.at_zero = cv.off;
    p.at_l2 = mxf_piece(cv, (size_t)r.S * p.qp * sizeof(double));
    p.at_dv = mxf_piece(cv, (size_t)r.S * sizeof(double));
    p.at_big = mxf_piece(cv, p.wide ? (size_t)p.end[2] * sizeof(double) : 0);
    p.bytes = cv.off;
    p.zero_bytes = p.bytes - p.at_zero;
    return p;
}

static inline PsiPlan psi_quad_plan(const PsiRequest& r) {
    PsiPlan p;
    if (psi_refused(r, true, p)) return p;
    Carver cv(nullptr);
    psi_head(r, p, cv);
    psi_grid_rows(r, p);
    p.npass = (int)mxf_cdiv(r.J, PSI_JB);
    p.n_out = (int64_t)r.S * r.N * r.J;
    p.split = p.mch > 1;
    p.at_wt = mxf_piece(cv, (size_t)p.n_mm * PSI_JB * r.esize);
    p.zero_bytes = p.split ? (size_t)p.n_out * sizeof(double) : 0;
    p.at_zero = p.at_acc = mxf_piece(cv, p.zero_bytes);
    p.bytes = cv.off;
    return p;
}

// ---- nearest.hip -------------------------------------------------------------------------------------------------------------------------
constexpr int NEAREST_RB = 128;     // rows (threads) per workgroup

struct NearestRequest {
    size_t esize = 4; bool step = false;      // step: mxf_kmeans_step, else mxf_nearest
    int64_t N = 0, M = 0; int Q = 0;
    bool has_X = false, has_C = false, has_idx = false;                                      // idx is required by mxf_nearest only
    bool has_Cnew = false, has_counts = false, has_inertia = false, alias = false;          // step; alias: C_new == C
};
// Scratch: the centres padded to QP (cp), then for a step the zeroed accumulators back to back: M QP double sums, M 64-bit counts and
// the inertia, [at_zero, at_zero + zero_bytes).  An absent piece has offset 0.
struct NearestPlan : FusedRefusal {
    int qp = 0;
    unsigned grid = 1;                  // of nearest_kernel: blocks of NEAREST_RB rows; M is not split
    int64_t n_prep = 0, n_close = 0;    // items of nearest_prep_kernel (M) and of kmeans_close_kernel (M, step only)
    size_t at_cp = 0, at_sums = 0, at_counts = 0, at_inertia = 0, at_zero = 0, zero_bytes = 0, bytes = 0;
};

static inline NearestPlan nearest_plan(const NearestRequest& r) {
    NearestPlan p;
    if (r.N < 1 || r.M < 1 || r.Q < 1) { p.refuse(-2, "N, M, Q >= 1"); return p; }
    if (r.Q > MXF_NEAREST_MAX_Q) { p.refuse_q(r.Q, MXF_NEAREST_MAX_Q); return p; }
    if (r.N > ((int64_t)1 << 31) || r.M > ((int64_t)1 << 31) - 1) { p.refuse(-2, "N <= 2^31, M <= 2^31 - 1"); return p; }
    if (!r.has_X || !r.has_C) { p.refuse(-2, "null X or C"); return p; }
    if (r.step) {
        if (!r.has_Cnew || !r.has_counts || !r.has_inertia) { p.refuse(-2, "null C_new, counts or inertia"); return p; }
        if (r.alias) { p.refuse(-2, "C_new must not alias C"); return p; }
    } else if (!r.has_idx) { p.refuse(-2, "null idx"); return p; }
    p.qp = mxf_qp(r.Q);
    p.grid = (unsigned)mxf_cdiv(r.N, NEAREST_RB);
    p.n_prep = r.M;
    Carver cv(nullptr);
    p.at_cp = mxf_piece(cv, (size_t)r.M * p.qp * r.esize);
    if (r.step) {
        p.n_close = r.M;
        p.at_zero = cv.off;
        p.at_sums = mxf_piece(cv, (size_t)r.M * p.qp * sizeof(double));
        p.at_counts = mxf_piece(cv, (size_t)r.M * sizeof(int64_t));
        p.at_inertia = mxf_piece(cv, sizeof(double));
        p.zero_bytes = cv.off - p.at_zero;
    }
    p.bytes = cv.off;
    return p;
}

// ---- knn.hip -----------------------------------------------------------------------------------------------------------------------------
constexpr int KNN_RB = 128;         // rows (threads) per workgroup

// slots of the register list the kernel is compiled for
static inline int mxf_kp(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : 32); }

struct KnnRequest {
    size_t esize = 4;
    int64_t N = 0, Nc = 0; int Q = 0, k = 0; bool causal = false;
    bool has_X = false, has_C = false, has_idx = false, same = false;      // same: C == X
};
// Scratch: the candidates padded to QP (cp)
struct KnnPlan : FusedRefusal {
    int qp = 0, kp = 0;                 // the kernel's <QP, KP>
    unsigned grid = 1;                  // of knn_kernel: blocks of KNN_RB rows; the candidates are not split
    int64_t n_prep = 0;                 // items of knn_prep_kernel (Nc)
    size_t at_cp = 0, bytes = 0;
};

static inline KnnPlan knn_plan(const KnnRequest& r) {
    KnnPlan p;
    if (r.N < 1 || r.Nc < 1 || r.Q < 1 || r.k < 1) { p.refuse(-2, "N, Nc, Q, k >= 1"); return p; }
    if (r.Q > MXF_KNN_MAX_Q) { p.refuse_q(r.Q, MXF_KNN_MAX_Q); return p; }
    if (r.k > MXF_KNN_MAX_K) { p.refusef(-3, "k = %d above the limit of %d neighbours", r.k, MXF_KNN_MAX_K); return p; }
    if (r.N > ((int64_t)1 << 31) || r.Nc > ((int64_t)1 << 31) - 1) { p.refuse(-2, "N <= 2^31, Nc <= 2^31 - 1"); return p; }
    if (!r.has_X || !r.has_C || !r.has_idx) { p.refuse(-2, "null X, C or idx"); return p; }
    if (r.causal && (!r.same || r.Nc != r.N)) { p.refuse(-2, "a causal search takes C == X and Nc == N"); return p; }
    p.qp = mxf_qp(r.Q);
    p.kp = mxf_kp(r.k);
    p.grid = (unsigned)mxf_cdiv(r.N, KNN_RB);
    p.n_prep = r.Nc;
    Carver cv(nullptr);
    p.at_cp = mxf_piece(cv, (size_t)r.Nc * p.qp * r.esize);
    p.bytes = cv.off;
    return p;
}

// ---- vecchia.hip -------------------------------------------------------------------------------------------------------------------------
constexpr int VECCHIA_ROWS = 2;         // rows of the data set (groups of 32 lanes, a tile each) per workgroup
constexpr int VECCHIA_MAX_GRID = 4096;  // workgroups; each takes further rows in a loop and closes with one atomic per sum

enum { VECCHIA_COND = 0, VECCHIA_LOGPDF = 1, VECCHIA_BWD = 2 };
struct VecchiaRequest {
    size_t esize = 4; int call = VECCHIA_LOGPDF;
    int64_t Nt = 0, N = 0; int Q = 0, P = 0, k = 0;      // Nt: the predictor's rows (ignored by the other two)
    bool has_Xt = false, has_X = false, has_Y = false, has_nbr = false, has_ls = false, has_var = false, has_noise = false;
    bool has_mean = false, has_vout = false;             // cond
    bool has_value = false;                              // logpdf
    bool has_g = false, has_dY = false;                  // bwd
};
// Scratch: zeroed doubles, n_acc of them: the value (logpdf), or the QP sums of the lengthscale, the variance's and the noise's (bwd)
struct VecchiaPlan : FusedRefusal {
    int qp = 0;
    int64_t rows = 0;                   // Nt or N
    unsigned grid = 1;                  // workgroups of VECCHIA_ROWS rows, at most VECCHIA_MAX_GRID
    int n_acc = 0;
    size_t at_acc = 0, zero_bytes = 0, bytes = 0;
    size_t dy_bytes = 0;                // of dY, zeroed before the scatter (0: no dY)
};

static inline VecchiaPlan vecchia_plan(const VecchiaRequest& r) {
    VecchiaPlan p;
    const bool cond = r.call == VECCHIA_COND;
    if (r.N < 1 || r.Q < 1 || r.P < 1 || r.k < 1 || (cond && r.Nt < 1)) { p.refuse(-2, "N, Nt, Q, P, k >= 1"); return p; }
    if (r.Q > MXF_KNN_MAX_Q) { p.refuse_q(r.Q, MXF_KNN_MAX_Q); return p; }
    if (r.k > MXF_KNN_MAX_K) { p.refusef(-3, "k = %d above the limit of %d neighbours", r.k, MXF_KNN_MAX_K); return p; }
    if (r.P > MXF_VECCHIA_MAX_P) { p.refusef(-3, "P = %d above the limit of %d output columns", r.P, MXF_VECCHIA_MAX_P); return p; }
    if (r.N > ((int64_t)1 << 31) - 1 || (cond && r.Nt > ((int64_t)1 << 31) - 1)) { p.refuse(-2, "N, Nt <= 2^31 - 1"); return p; }
    if (!r.has_X || !r.has_Y || !r.has_nbr || !r.has_ls || !r.has_var || !r.has_noise) {
        p.refuse(-2, "null X, Y, nbr, lengthscale, variance or noise");
        return p;
    }
    if (cond && (!r.has_Xt || !r.has_mean || !r.has_vout)) { p.refuse(-2, "null Xt, mean_out or var_out"); return p; }
    if (r.call == VECCHIA_LOGPDF && !r.has_value) { p.refuse(-2, "null value_out"); return p; }
    if (r.call == VECCHIA_BWD && !r.has_g) { p.refuse(-2, "null g"); return p; }
    p.qp = mxf_qp(r.Q);
    p.rows = cond ? r.Nt : r.N;
    p.grid = (unsigned)mxf_clampi(mxf_cdiv(p.rows, VECCHIA_ROWS), 1, VECCHIA_MAX_GRID);
    p.n_acc = cond ? 0 : (r.call == VECCHIA_LOGPDF ? 1 : p.qp + 2);
    Carver cv(nullptr);
    p.zero_bytes = (size_t)p.n_acc * sizeof(double);
    p.at_acc = mxf_piece(cv, p.zero_bytes);
    p.bytes = cv.off;
    p.dy_bytes = (r.call == VECCHIA_BWD && r.has_dY) ? (size_t)r.N * r.P * r.esize : 0;
    return p;
}
