// Fused Gram pass of the intrinsic coregionalisation model and its reverse mode (gfx950): mxf_gram_icm, mxf_gram_icm_bwd.
//
//   K[s, i, j] = k(x_i, x'_j) B[s|0, idx[i], idx2[j]],   k one of the four stationary kinds.
//
// Without it the product of a stationary kernel and a Coregionalize kernel is three N x N2 passes forward (a Gram, a gathered B, their
// product) and, in reverse, a recomputed Gram, two more N x N2 temporaries and an index_put of N N2 elements for dB.  Here: one pass and one
// write forward; one read of dK in reverse, nothing of size N x N2 stored.  The launch shapes are gram_icm_plan.h.
//
// Mapping (wave64, both passes, as gram_diff.hip): lane <-> column, so that rows of K are written and rows of dK read coalesced; a workgroup
// of 256 lanes owns a tile of 256 columns and a band of rows whose raw coordinates and output indices are staged in LDS 64 rows at a time.
// B of the sample lies in LDS (at most 8 KB).  A lane's column has one output index b, a row's index a is wave-uniform: the lanes of a wave
// read B[a][b] from at most T distinct words of one LDS row.  The distance is formed from the raw coordinates: d = x - z first, r2 = sum_q
// d_q^2 / l_q^2 after (gram2.hip's order: coincident points give r2 = 0 exactly).
// Reverse: column-side sums (dX2) live in registers and leave with one atomic per value; row-side sums (dX) are reduce-scattered across the
// wave per row, accumulated in an LDS band and flushed once; dls and dvar are block-reduced in double.  dB: lane `tid` owns the LDS words
// dBp[a][tid], a = 0..T-1, and adds the pair's dK k to dBp[idx[row]][tid] with a plain read and write (consecutive lanes, consecutive banks;
// no atomic: nobody else touches the word).  At the end each lane folds its T words into the workgroup's T x T double partial dBs[a][b] (T
// LDS atomics per lane, once), and the workgroup adds the partial to the double accumulator with T x T global atomics.
#include "common.h"
#include "shared_grad.h"
#include "gram_icm_plan.h"

namespace {

constexpr int TR = MXF_ICM_TR, COLS = MXF_ICM_COLS;

template <typename T>
struct IcmArgs {
    const T* X; const T* X2; const int32_t* idx; const int32_t* idx2; const T* ls; const T* var; const T* B; const T* diag;
    T* K; const T* dK;
    T* dX; T* dX2; double* dls; double* dvar; double* dB;
    int64_t N, N2, ldk, rb;
    int64_t sX, sX2, sls, svar, sB, sdiag, sK;
    int Q, Tn, ard, square;
    unsigned o_ridx, o_Bs, o_racc, o_dBp, o_dBs, o_red;      // byte offsets into the dynamic LDS block (GramIcmPlan)
    T jitter;
};

// e^x for x <= 0 (gram_bwd.hip's forms: the hardware exp2 of x log2(e) in float, the bare exponential of common.h in double)
__device__ __forceinline__ float icm_expnp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ double icm_expnp(double x) { return mxf_exp_nonpos_f64(x); }

// unit-variance covariance k and slope w = dk / d(r2) of the scaled squared distance (Matern: r2 clipped at 1e-14, the un-clipped r2 in the
// 5/3 r^2 term, as gram.hip and gram_bwd.hip)
template <typename T, int KIND>
__device__ __forceinline__ void icm_cov(T r2, T& k, T& w) {
    if (KIND == MXF_K_RBF) { k = icm_expnp((T)-0.5 * r2); w = (T)-0.5 * k; return; }
    const bool clipped = r2 < (T)1e-14;
    const T r = sqrt(clipped ? (T)1e-14 : r2);
    if (KIND == MXF_K_MATERN12) { k = icm_expnp(-r); w = clipped ? (T)0 : -k / ((T)2 * r); return; }
    if (KIND == MXF_K_MATERN32) {
        const T s3 = (T)1.7320508075688772, e = icm_expnp(-s3 * r);
        k = ((T)1 + s3 * r) * e; w = clipped ? (T)0 : (T)-1.5 * e; return;
    }
    const T s5 = (T)2.23606797749979, e = icm_expnp(-s5 * r);
    k = ((T)1 + s5 * r + (T)(5.0 / 3.0) * r2) * e;
    w = clipped ? (T)(5.0 / 3.0) * e : (T)(-5.0 / 6.0) * ((T)1 + s5 * r) * e;
}

__device__ __forceinline__ int icm_clamp(int i, int Tn) { return i < 0 ? 0 : (i >= Tn ? Tn - 1 : i); }

// rows [rt, rt + TR) of X (zeros beyond rend and beyond Q) into xs[TR][QT], their clamped output indices into ridx[TR]
template <typename T, int QT>
__device__ __forceinline__ void icm_stage_rows(const T* __restrict__ X, const int32_t* __restrict__ idx, int64_t rt, int64_t rend, int Q, int Tn, T* xs, int* ridx) {
    for (int i = threadIdx.x; i < TR * QT; i += COLS) {
        const int r = i / QT, q = i % QT;
        const int64_t row = rt + r;
        xs[i] = (row < rend && q < Q) ? X[row * Q + q] : (T)0;
    }
    if (threadIdx.x < TR) {
        const int64_t row = rt + threadIdx.x;
        ridx[threadIdx.x] = row < rend ? icm_clamp(idx[row], Tn) : 0;
    }
}

template <typename T, int KIND, int QT>
__global__ __launch_bounds__(256) void gram_icm_kernel(IcmArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* xs = reinterpret_cast<T*>(smem_raw);                          // [TR][QT]
    int* ridx = reinterpret_cast<int*>(smem_raw + a.o_ridx);         // [TR]
    T* Bs = reinterpret_cast<T*>(smem_raw + a.o_Bs);                 // [Tn][Tn]
    const int tid = threadIdx.x, s = blockIdx.z, Tn = a.Tn;
    const int64_t r0 = (int64_t)blockIdx.y * TR, rend = (r0 + TR < a.N) ? r0 + TR : a.N;
    const int64_t col = (int64_t)blockIdx.x * COLS + tid;
    const bool cvalid = col < a.N2;
    const T* __restrict__ Bg = a.B + (int64_t)s * a.sB;
    for (int i = tid; i < Tn * Tn; i += COLS) Bs[i] = Bg[i];
    icm_stage_rows<T, QT>(a.X + (int64_t)s * a.sX, a.idx, r0, rend, a.Q, Tn, xs, ridx);
    const T* __restrict__ X2 = a.X2 + (int64_t)s * a.sX2;
    const T* __restrict__ ls = a.ls + (int64_t)s * a.sls;
    T z[QT], il2[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        z[q] = (cvalid && q < a.Q) ? X2[col * a.Q + q] : (T)0;
        const T il = q < a.Q ? (T)1 / ls[a.ard ? q : 0] : (T)0;
        il2[q] = il * il;
    }
    const int jc = cvalid ? icm_clamp(a.idx2[col], Tn) : 0;
    const T variance = a.var[(int64_t)s * a.svar];
    const T dadd = (a.diag ? a.diag[(int64_t)s * a.sdiag] : (T)0) + a.jitter;
    T* __restrict__ K = a.K + (int64_t)s * a.sK;
    __syncthreads();
    const int rmax = (int)(rend - r0);
    for (int r = 0; r < rmax; ++r) {
        T r2 = 0;
#pragma unroll
        for (int q = 0; q < QT; ++q) { const T d = xs[r * QT + q] - z[q]; r2 = fma(d * d, il2[q], r2); }
        T k, w;
        icm_cov<T, KIND>(r2, k, w);
        k = variance * k * Bs[ridx[r] * Tn + jc];
        if (a.square && r0 + r == col) k += dadd;
        if (cvalid) K[(r0 + r) * a.ldk + col] = k;
    }
}

template <typename T, int KIND, int QT>
__global__ __launch_bounds__(256) void gram_icm_bwd_kernel(IcmArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* xs = reinterpret_cast<T*>(smem_raw);                          // [TR][QT]
    int* ridx = reinterpret_cast<int*>(smem_raw + a.o_ridx);         // [TR]
    T* Bs = reinterpret_cast<T*>(smem_raw + a.o_Bs);                 // [Tn][Tn]
    T* racc = reinterpret_cast<T*>(smem_raw + a.o_racc);             // [rb][QT]
    T* dBp = reinterpret_cast<T*>(smem_raw + a.o_dBp);               // [Tn][COLS]   (dB asked for)
    double* dBs = reinterpret_cast<double*>(smem_raw + a.o_dBs);     // [Tn][Tn]     (dB asked for)
    double* red = reinterpret_cast<double*>(smem_raw + a.o_red);     // [16]
    const int tid = threadIdx.x, lane = tid & 63, s = blockIdx.z, Tn = a.Tn, Q = a.Q;
    const int64_t r0 = (int64_t)blockIdx.y * a.rb, rend = (r0 + a.rb < a.N) ? r0 + a.rb : a.N;
    const int64_t col = (int64_t)blockIdx.x * COLS + tid;
    const bool cvalid = col < a.N2;
    const T* __restrict__ X = a.X + (int64_t)s * a.sX;
    const T* __restrict__ X2 = a.X2 + (int64_t)s * a.sX2;
    const T* __restrict__ ls = a.ls + (int64_t)s * a.sls;
    const T* __restrict__ dK = a.dK + (int64_t)s * a.sK;
    const T* __restrict__ Bg = a.B + (int64_t)s * a.sB;
    const bool wantB = a.dB != nullptr, rowside = a.dX != nullptr;
    for (int i = tid; i < Tn * Tn; i += COLS) Bs[i] = Bg[i];
    for (int64_t i = tid; i < (rend - r0) * QT; i += COLS) racc[i] = (T)0;
    if (wantB) {
        for (int t = 0; t < Tn; ++t) dBp[t * COLS + tid] = (T)0;
        for (int i = tid; i < Tn * Tn; i += COLS) dBs[i] = 0.0;
    }
    T z[QT], gz[QT], gl[QT], il2[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        z[q] = (cvalid && q < Q) ? X2[col * Q + q] : (T)0;
        const T il = q < Q ? (T)1 / ls[a.ard ? q : 0] : (T)0;
        il2[q] = il * il; gz[q] = 0; gl[q] = 0;
    }
    const int jc = cvalid ? icm_clamp(a.idx2[col], Tn) : 0;
    const T variance = a.var[(int64_t)s * a.svar];
    T gvar = 0;

    for (int64_t rt = r0; rt < rend; rt += TR) {
        __syncthreads();
        icm_stage_rows<T, QT>(X, a.idx, rt, rend, Q, Tn, xs, ridx);
        __syncthreads();
        const int rmax = (int)((rend - rt) < TR ? (rend - rt) : TR);
        for (int r = 0; r < rmax; ++r) {
            const T g = cvalid ? dK[(rt + r) * a.ldk + col] : (T)0;
            const int ir = ridx[r];                       // wave-uniform
            T d[QT], r2 = 0;
#pragma unroll
            for (int q = 0; q < QT; ++q) { d[q] = xs[r * QT + q] - z[q]; r2 = fma(d[q] * d[q], il2[q], r2); }
            T k, w;
            icm_cov<T, KIND>(r2, k, w);
            const T ge = g * Bs[ir * Tn + jc];            // the effective cotangent of the stationary factor
            gvar = fma(ge, k, gvar);
            if (wantB) dBp[ir * COLS + tid] = fma(g * variance, k, dBp[ir * COLS + tid]);
            const T W2 = (T)2 * ge * w * variance;        // 2 dL / d(r2)
            T tq[QT];
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const T t = W2 * d[q] * il2[q];           // dL / dx_q of this pair
                gz[q] -= t;
                gl[q] = fma(-t, d[q], gl[q]);             // dL / dl_q times l_q
                tq[q] = t;
            }
            if (rowside) {                                // this wave's 64 columns of the row: one reduce-scatter, one LDS atomic from Q lanes
                T* ra = racc + (rt + r - r0) * QT;
                const T rs = row_reduce_scatter<T, QT>(tq, lane);
                if constexpr (sizeof(T) == 4) {
                    const float v = wave_rows_sum(rs);
                    if (lane < QT && lane < Q) lds_add(ra + lane, v);
                } else {
                    const int l16 = lane & 15;
                    if (l16 < QT && l16 < Q) lds_add(ra + l16, rs);
                }
            }
        }
    }
    // column side: both roles flow into dX in the square case
    T* dXc = a.square ? a.dX : a.dX2;
    const int64_t sXc = a.square ? a.sX : a.sX2;
    if (dXc && cvalid) {
#pragma unroll
        for (int q = 0; q < QT; ++q)
            if (q < Q) atomic_add(dXc + (int64_t)s * sXc + col * Q + q, gz[q]);
    }
    __syncthreads();
    if (rowside)
        for (int64_t i = tid; i < (rend - r0) * QT; i += COLS) {
            const int q = (int)(i % QT);
            if (q < Q) atomic_add(a.dX + (int64_t)s * a.sX + (r0 + i / QT) * Q + q, racc[i]);
        }
    if (wantB) {      // each lane's T words into the workgroup's T x T partial, then one global atomic per entry
        if (cvalid)
            for (int t = 0; t < Tn; ++t) {
                const T v = dBp[t * COLS + tid];
                if (v != (T)0) lds_add(dBs + t * Tn + jc, (double)v);
            }
        __syncthreads();
        double* dBg = a.dB + (a.sB ? (int64_t)s * Tn * Tn : 0);
        for (int i = tid; i < Tn * Tn; i += COLS)
            if (dBs[i] != 0.0) atomic_add(dBg + i, dBs[i]);
    }
    if (a.dls) {
        double* dl = a.dls + (int64_t)s * a.sls;
        if (a.ard) {
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const double v = block_sum<double>((double)gl[q], red);
                if (tid == 0 && q < Q) atomic_add(dl + q, v / (double)ls[q]);
            }
        } else {
            T v = 0;
#pragma unroll
            for (int q = 0; q < QT; ++q) v += gl[q];
            const double t = block_sum<double>((double)v, red);
            if (tid == 0) atomic_add(dl, t / (double)ls[0]);
        }
    }
    if (a.dvar) {
        const double v = block_sum<double>((double)gvar, red);
        if (tid == 0) atomic_add(a.dvar + (int64_t)s * a.svar, v);
    }
}

struct IcmCall {
    int kind, dtype, S; int64_t N, N2; int Q, T;
    const void* X; int64_t sX; const void* X2; int64_t sX2; const int32_t* idx; const int32_t* idx2;
    const void* ls; int ard; int64_t sls; const void* var; int64_t svar; const void* B; int64_t sB;
    const void* diag; int64_t sdiag; double jitter;
    void* K; const void* dK; int64_t ldk, sK;
    void* dX; void* dX2; void* dls; void* dvar; void* dB;
    bool bwd;
};

template <typename T, int KIND, int QT>
int launch(mxf_ctx* h, const IcmCall& d, const GramIcmPlan& p, const SharedSums& sums, hipStream_t st) {
    IcmArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.square = d.X2 == nullptr;
    a.X = (const T*)d.X; a.sX = d.sX; a.X2 = a.square ? a.X : (const T*)d.X2; a.sX2 = a.square ? d.sX : d.sX2;
    a.idx = d.idx; a.idx2 = a.square ? d.idx : d.idx2;
    a.ls = (const T*)d.ls; a.sls = d.sls; a.var = (const T*)d.var; a.svar = d.svar; a.B = (const T*)d.B; a.sB = d.sB;
    a.diag = (const T*)d.diag; a.sdiag = d.sdiag; a.jitter = (T)d.jitter;
    a.K = (T*)d.K; a.dK = (const T*)d.dK; a.ldk = d.ldk; a.sK = d.sK;
    a.dX = (T*)d.dX; a.dX2 = a.square ? nullptr : (T*)d.dX2; a.dB = sums.acc[0]; a.dls = sums.acc[1]; a.dvar = sums.acc[2];
    a.N = d.N; a.N2 = a.square ? d.N : d.N2; a.rb = p.rb; a.Q = d.Q; a.Tn = d.T; a.ard = d.ard;
    a.o_ridx = (unsigned)p.ridx; a.o_Bs = (unsigned)p.Bs; a.o_racc = (unsigned)p.racc; a.o_dBp = (unsigned)p.dBp; a.o_dBs = (unsigned)p.dBs; a.o_red = (unsigned)p.red;
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    if (d.bwd) {
        if (p.lds_bytes > 64 * 1024) {      // raised once per instantiation and device, to the plan's bound: not a host call per training step
            static bool raised[64] = {};
            const int dev = h->device;
            if (dev < 0 || dev >= 64 || !raised[dev]) {
                MXF_HIP(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&gram_icm_bwd_kernel<T, KIND, QT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MXF_ICM_LDS_MAX));
                if (dev >= 0 && dev < 64) raised[dev] = true;
            }
        }
        hipLaunchKernelGGL((gram_icm_bwd_kernel<T, KIND, QT>), grid, dim3(COLS), p.lds_bytes, st, a);
    } else {
        hipLaunchKernelGGL((gram_icm_kernel<T, KIND, QT>), grid, dim3(COLS), p.lds_bytes, st, a);
    }
    return 0;
}

template <typename T>
int icm_typed(mxf_ctx* h, const char* name, const IcmCall& d, const GramIcmPlan& p, hipStream_t st) {
    SharedSums sums = SharedSums();
    if (d.bwd) {
        const int64_t nls = d.ard ? d.Q : 1;
        const int rc = shared_sums_open<T>(h, name, {{d.dB, (d.sB ? d.S : 1) * (int64_t)d.T * d.T}, {d.dls, (d.sls ? d.S : 1) * nls}, {d.dvar, d.svar ? d.S : 1}}, st, &sums);
        if (rc) return rc;
    }
    const int rc = dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52>(d.kind, [&](auto kd) {
        return dispatch<1, 2, 4, 8, 16>(p.QT, [&](auto qt) { return launch<T, decltype(kd)::value, decltype(qt)::value>(h, d, p, sums, st); });
    });
    if (rc == NO_CASE) MXF_FAIL(h, -2, "%s: no kernel for kind %d, Q tile %d", name, d.kind, p.QT);
    if (rc) return rc;
    MXF_LAUNCH_CHECK(h);
    if (d.bwd) shared_sums_close(sums, st);
    return 0;
}

int gram_icm_call(mxf_ctx* h, const char* name, const IcmCall& d, hipStream_t st) {
    if (d.dtype != MXF_F32 && d.dtype != MXF_F64) return mxf_bad_dtype(h, name, d.dtype);
    GramIcmRequest r;
    r.kind = d.kind; r.elem_size = mxf_esize(d.dtype); r.bwd = d.bwd; r.S = d.S; r.N = d.N; r.N2 = d.N2; r.Q = d.Q; r.T = d.T;
    r.ard = d.ard != 0; r.square = d.X2 == nullptr;
    r.has_X = d.X != nullptr; r.has_idx = d.idx != nullptr; r.has_idx2 = d.idx2 != nullptr; r.has_ls = d.ls != nullptr; r.has_var = d.var != nullptr;
    r.has_B = d.B != nullptr; r.has_K = d.bwd ? d.dK != nullptr : d.K != nullptr; r.want_dB = d.dB != nullptr;
    r.sX = d.sX; r.sX2 = d.sX2; r.sls = d.sls; r.svar = d.svar; r.sB = d.sB; r.sdiag = d.sdiag; r.ldk = d.ldk; r.sK = d.sK;
    const GramIcmPlan p = gram_icm_plan(r);
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    if (d.bwd && !d.dX && !d.dls && !d.dvar && !d.dB && (r.square || !d.dX2)) return 0;      // nothing is asked for
    return d.dtype == MXF_F32 ? icm_typed<float>(h, name, d, p, st) : icm_typed<double>(h, name, d, p, st);
}

}  // namespace

extern "C" int mxf_gram_icm(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int T,
                            const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2, const int32_t* idx, const int32_t* idx2,
                            const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                            const void* B, int64_t strideS_B, const void* diag_add, int64_t strideS_diag, double jitter,
                            void* K_out, int64_t ldk, int64_t strideS_K, void* stream) {
    if (!h) return -1;
    return gram_icm_call(h, "mxf_gram_icm",
                         {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .T = T, .X = X, .sX = strideS_X, .X2 = X2, .sX2 = strideS_X2,
                          .idx = idx, .idx2 = idx2, .ls = lengthscale, .ard = ard, .sls = strideS_ls, .var = variance, .svar = strideS_var,
                          .B = B, .sB = strideS_B, .diag = X2 ? nullptr : diag_add, .sdiag = strideS_diag, .jitter = X2 ? 0.0 : jitter,
                          .K = K_out, .dK = nullptr, .ldk = ldk, .sK = strideS_K,
                          .dX = nullptr, .dX2 = nullptr, .dls = nullptr, .dvar = nullptr, .dB = nullptr, .bwd = false},
                         (hipStream_t)stream);
}

extern "C" int mxf_gram_icm_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int T,
                                const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2, const int32_t* idx, const int32_t* idx2,
                                const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                                const void* B, int64_t strideS_B, const void* dK, int64_t lddk, int64_t strideS_dK,
                                void* dX, void* dX2, void* dls, void* dvar, void* dB, void* stream) {
    if (!h) return -1;
    return gram_icm_call(h, "mxf_gram_icm_bwd",
                         {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .T = T, .X = X, .sX = strideS_X, .X2 = X2, .sX2 = strideS_X2,
                          .idx = idx, .idx2 = idx2, .ls = lengthscale, .ard = ard, .sls = strideS_ls, .var = variance, .svar = strideS_var,
                          .B = B, .sB = strideS_B, .diag = nullptr, .sdiag = 0, .jitter = 0.0,
                          .K = nullptr, .dK = dK, .ldk = lddk, .sK = strideS_dK,
                          .dX = dX, .dX2 = dX2, .dls = dls, .dvar = dvar, .dB = dB, .bwd = true},
                         (hipStream_t)stream);
}
