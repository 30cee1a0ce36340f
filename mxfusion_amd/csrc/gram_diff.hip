// Difference-form Gram pass and its reverse mode (gfx950): Periodic, RationalQuadratic and SpectralMixture (mxf_gram_diff, mxf_gram_diff_bwd).
//
// These covariances are functions of the per-dimension differences tau_d = x_d - x'_d, not of one scaled distance, so they do not fit the
// pre-scaled-coordinate kernels of gram.hip / gram_bwd.hip.  The per-pair math is gram_diff.h (host-checkable); the launch shapes are
// gram_diff_plan.h.
//
// Mapping (wave64, both passes): lane <-> column, so that rows of K are written and rows of dK read coalesced; a workgroup of 256 lanes owns
// a tile of 256 columns and a band of rows whose raw coordinates are staged in LDS 64 rows at a time.  tau is formed from the raw
// coordinates (x - z first), the components' constants are prepared once per workgroup into LDS.
// Forward: K = sum_a amp_a k_a(tau), one store per pair.
// Reverse: K is recomputed; nothing of size N x N2 is stored.  The component loop is OUTERMOST: a lane then carries the 1 + 2 QT parameter sums
//          of ONE component in registers (136 sums for SpectralMixture at A = Q = 8 would not fit) and its constants are wave-uniform; dK is
//          re-read per component (from L2: a workgroup's slab is rb x 256 values).  Column-side sums (dX2) live in registers and leave with one
//          atomic per value; row-side sums (dX) are reduce-scattered across the wave per row and accumulated in an LDS band across components
//          and flushed once; parameter sums are reduced once per component and workgroup.
#include "common.h"
#include "gram_diff_plan.h"

#define MXF_GD_FNS
// float: the hardware's sine / cosine take revolutions (the reduced phase as it is), e^x is exp2 of the pre-scaled argument -- the
// formulation of the existing Gram kernels; double: the library functions and the bare exponential of common.h
template <typename T> __host__ __device__ __forceinline__ T gd_sin_rev(T u);
template <typename T> __host__ __device__ __forceinline__ T gd_cos_rev(T u);
template <typename T> __host__ __device__ __forceinline__ T gd_exp_nonpos(T x);
template <typename T> __host__ __device__ __forceinline__ T gd_log1p(T x);
#if defined(__HIP_DEVICE_COMPILE__)
#define MXF_GD_DEV(dev, host) dev
#else
#define MXF_GD_DEV(dev, host) host
#endif
template <> __host__ __device__ __forceinline__ float gd_sin_rev<float>(float u) { return MXF_GD_DEV(__builtin_amdgcn_sinf(u), sinf(6.283185307179586477f * u)); }
template <> __host__ __device__ __forceinline__ float gd_cos_rev<float>(float u) { return MXF_GD_DEV(__builtin_amdgcn_cosf(u), cosf(6.283185307179586477f * u)); }
template <> __host__ __device__ __forceinline__ float gd_exp_nonpos<float>(float x) { return MXF_GD_DEV(__builtin_amdgcn_exp2f(x * 1.44269504088896340736f), expf(x)); }
template <> __host__ __device__ __forceinline__ double gd_exp_nonpos<double>(double x) { return MXF_GD_DEV(mxf_exp_nonpos_f64(x), exp(x)); }
template <> __host__ __device__ __forceinline__ double gd_sin_rev<double>(double u) { return sin(6.283185307179586477 * u); }
template <> __host__ __device__ __forceinline__ double gd_cos_rev<double>(double u) { return cos(6.283185307179586477 * u); }
template <> __host__ __device__ __forceinline__ float gd_log1p<float>(float x) { return log1pf(x); }
template <> __host__ __device__ __forceinline__ double gd_log1p<double>(double x) { return log1p(x); }
#include "gram_diff.h"

namespace {

constexpr int TR = MXF_GD_TR, COLS = MXF_GD_COLS;

template <typename T>
struct GdArgs {
    const T* X; const T* X2; const T* p0; const T* p1; const T* p2; const T* diag;
    T* K; const T* dK;
    T* dX; T* dX2; T* dp0; T* dp1; T* dp2;
    int64_t N, N2, ldk, rb;
    int64_t sX, sX2, sp0, sp1, sp2, sdiag, sK;
    int Q, A, ard, square;
    T jitter;
};

// the constants of every component, prepared by the first A lanes
template <typename T, int KIND, int QT>
__device__ __forceinline__ void prepare_all(const GdArgs<T>& a, int s, GdComp<T, QT>* comp) {
    const int nc = KIND == MXF_KD_SM ? a.A : 1;
    if ((int)threadIdx.x < nc) {
        const int c = threadIdx.x;
        const T* p1 = a.p1 + (int64_t)s * a.sp1 + (KIND == MXF_KD_SM ? c * a.Q : 0);
        const T* p2 = a.p2 + (int64_t)s * a.sp2 + (KIND == MXF_KD_SM ? c * a.Q : 0);
        gd_prepare<T, KIND, QT>(a.Q, KIND == MXF_KD_SM ? 1 : a.ard, a.p0[(int64_t)s * a.sp0 + c], p1, p2, comp[c]);
    }
}

// rows [rt, rt + TR) of X (zeros beyond rend and beyond Q) into xs[TR][QT]
template <typename T, int QT>
__device__ __forceinline__ void stage_rows(const T* __restrict__ X, int64_t rt, int64_t rend, int Q, T* xs) {
    for (int i = threadIdx.x; i < TR * QT; i += COLS) {
        const int r = i / QT, q = i % QT;
        const int64_t row = rt + r;
        xs[i] = (row < rend && q < Q) ? X[row * Q + q] : (T)0;
    }
}

template <typename T, int KIND, int QT>
__global__ __launch_bounds__(256) void gram_diff_kernel(GdArgs<T> a) {
    constexpr int NC = KIND == MXF_KD_SM ? MXF_GD_SM_MAX_A : 1;
    __shared__ T xs[TR * QT];
    __shared__ GdComp<T, QT> comp[NC];
    const int tid = threadIdx.x, s = blockIdx.z;
    const int64_t r0 = (int64_t)blockIdx.y * TR, rend = (r0 + TR < a.N) ? r0 + TR : a.N;
    const int64_t col = (int64_t)blockIdx.x * COLS + tid;
    const bool cvalid = col < a.N2;
    const int nc = KIND == MXF_KD_SM ? a.A : 1;
    prepare_all<T, KIND, QT>(a, s, comp);
    stage_rows<T, QT>(a.X + (int64_t)s * a.sX, r0, rend, a.Q, xs);
    const T* __restrict__ X2 = a.X2 + (int64_t)s * a.sX2;
    T z[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) z[q] = (cvalid && q < a.Q) ? X2[col * a.Q + q] : (T)0;
    const T dadd = (a.diag ? a.diag[(int64_t)s * a.sdiag] : (T)0) + a.jitter;
    T* __restrict__ K = a.K + (int64_t)s * a.sK;
    __syncthreads();
    const int rmax = (int)(rend - r0);
    for (int r = 0; r < rmax; ++r) {
        T tau[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) tau[q] = xs[r * QT + q] - z[q];
        T k = 0;
        for (int c = 0; c < nc; ++c) k = fma(comp[c].amp, gd_value<T, KIND, QT>(tau, comp[c]), k);
        if (a.square && r0 + r == col) k += dadd;
        if (cvalid) K[(r0 + r) * a.ldk + col] = k;
    }
}

template <typename T, int KIND, int QT>
__global__ __launch_bounds__(256) void gram_diff_bwd_kernel(GdArgs<T> a) {
    constexpr int NC = KIND == MXF_KD_SM ? MXF_GD_SM_MAX_A : 1;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* racc = reinterpret_cast<T*>(smem_raw);      // [rb][QT]
    __shared__ T xs[TR * QT];
    __shared__ GdComp<T, QT> comp[NC];
    __shared__ T red[16];
    const int tid = threadIdx.x, lane = tid & 63, s = blockIdx.z;
    const int64_t r0 = (int64_t)blockIdx.y * a.rb, rend = (r0 + a.rb < a.N) ? r0 + a.rb : a.N;
    const int64_t col = (int64_t)blockIdx.x * COLS + tid;
    const bool cvalid = col < a.N2;
    const int Q = a.Q, nc = KIND == MXF_KD_SM ? a.A : 1;
    const T* __restrict__ X = a.X + (int64_t)s * a.sX;
    const T* __restrict__ X2 = a.X2 + (int64_t)s * a.sX2;
    const T* __restrict__ dK = a.dK + (int64_t)s * a.sK;
    prepare_all<T, KIND, QT>(a, s, comp);
    for (int64_t i = tid; i < (rend - r0) * QT; i += COLS) racc[i] = (T)0;
    T z[QT], gz[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) { z[q] = (cvalid && q < Q) ? X2[col * Q + q] : (T)0; gz[q] = 0; }
    T* dXc = a.square ? a.dX : a.dX2;
    const int64_t sXc = a.square ? a.sX : a.sX2;
    const bool rowside = a.dX != nullptr;
    const bool want1 = a.dp1 != nullptr, want2 = a.dp2 != nullptr;

    for (int c = 0; c < nc; ++c) {
        __syncthreads();                   // comp[] is written; the previous component's reads of xs and red are over
        const GdComp<T, QT> cc = comp[c];
        T g0 = 0, g1[QT], g2[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) { g1[q] = 0; g2[q] = 0; }
        for (int64_t rt = r0; rt < rend; rt += TR) {
            __syncthreads();
            stage_rows<T, QT>(X, rt, rend, Q, xs);
            __syncthreads();
            const int rmax = (int)((rend - rt) < TR ? (rend - rt) : TR);
            for (int r = 0; r < rmax; ++r) {
                const T g = cvalid ? dK[(rt + r) * a.ldk + col] : (T)0;
                T tau[QT], dtau[QT], t1[QT], t2[QT];
#pragma unroll
                for (int q = 0; q < QT; ++q) tau[q] = xs[r * QT + q] - z[q];
                const T k = gd_grad<T, KIND, QT>(tau, cc, dtau, t1, t2);
                g0 = fma(g, k, g0);
                const T W = g * cc.amp;
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    if (want1) g1[q] = fma(g, t1[q], g1[q]);
                    if (want2) g2[q] = fma(g, t2[q], g2[q]);
                    dtau[q] *= W;              // dL / dtau_q of this pair and component
                    gz[q] -= dtau[q];
                }
                if (rowside) {                 // this wave's 64 columns of the row: one reduce-scatter, one LDS atomic from Q lanes
                    T* ra = racc + (rt + r - r0) * QT;
                    const T rs = row_reduce_scatter<T, QT>(dtau, lane);
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
        // this component's parameter sums: one reduction per workgroup, scaled to the raw operand's gradient by thread 0
        const int64_t o0 = (int64_t)s * a.sp0 + (KIND == MXF_KD_SM ? c : 0);
        const int64_t o1 = (int64_t)s * a.sp1 + (KIND == MXF_KD_SM ? c * Q : 0), o2 = (int64_t)s * a.sp2 + (KIND == MXF_KD_SM ? c * Q : 0);
        const bool ard1 = KIND == MXF_KD_SM || a.ard, ard2 = KIND == MXF_KD_SM || (KIND == MXF_KD_PERIODIC && a.ard);
        if (a.dp0) { const T v = block_sum<T>(g0, red); if (tid == 0) atomic_add(a.dp0 + o0, v); }
        if (want1) {
            T tot = 0;
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const T v = block_sum<T>(g1[q], red);
                if (tid == 0 && q < Q) {
                    const T f = gd_finish<T, KIND>(1, cc.amp, a.p1[o1 + (ard1 ? q : 0)], (T)1, v);
                    if (ard1) atomic_add(a.dp1 + o1 + q, f); else tot += f;
                }
            }
            if (tid == 0 && !ard1) atomic_add(a.dp1 + o1, tot);
        }
        if (want2) {
            T tot = 0;
            constexpr int N2T = KIND == MXF_KD_RQ ? 1 : QT;      // alpha: one sum
#pragma unroll
            for (int q = 0; q < N2T; ++q) {
                const T v = block_sum<T>(g2[q], red);
                if (tid == 0 && q < Q) {
                    const T f = gd_finish<T, KIND>(2, cc.amp, (T)1, a.p2[o2 + (ard2 ? q : 0)], v);
                    if (ard2) atomic_add(a.dp2 + o2 + q, f); else tot += f;
                }
            }
            if (tid == 0 && !ard2) atomic_add(a.dp2 + o2, tot);
        }
    }
    // column side: both roles flow into dX in the square case
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
}

struct GdCall {
    int kind, dtype, S; int64_t N, N2; int Q, A;
    const void* X; int64_t sX; const void* X2; int64_t sX2;
    const void* p0; int64_t sp0; const void* p1; int64_t sp1; const void* p2; int64_t sp2; int ard;
    const void* diag; int64_t sdiag; double jitter;
    void* K; const void* dK; int64_t ldk, sK;
    void* dX; void* dX2; void* dp0; void* dp1; void* dp2;
    bool bwd;
};

template <typename T, int KIND, int QT>
void launch(const GdCall& d, const GramDiffPlan& p, hipStream_t st) {
    GdArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.square = d.X2 == nullptr;
    a.X = (const T*)d.X; a.sX = d.sX; a.X2 = a.square ? a.X : (const T*)d.X2; a.sX2 = a.square ? d.sX : d.sX2;
    a.p0 = (const T*)d.p0; a.sp0 = d.sp0; a.p1 = (const T*)d.p1; a.sp1 = d.sp1; a.p2 = (const T*)d.p2; a.sp2 = d.sp2;
    a.diag = (const T*)d.diag; a.sdiag = d.sdiag; a.jitter = (T)d.jitter;
    a.K = (T*)d.K; a.dK = (const T*)d.dK; a.ldk = d.ldk; a.sK = d.sK;
    a.dX = (T*)d.dX; a.dX2 = a.square ? nullptr : (T*)d.dX2; a.dp0 = (T*)d.dp0; a.dp1 = (T*)d.dp1; a.dp2 = (T*)d.dp2;
    a.N = d.N; a.N2 = a.square ? d.N : d.N2; a.rb = p.rb; a.Q = d.Q; a.A = d.A; a.ard = d.ard;
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    if (d.bwd) hipLaunchKernelGGL((gram_diff_bwd_kernel<T, KIND, QT>), grid, dim3(COLS), p.lds_bytes, st, a);
    else hipLaunchKernelGGL((gram_diff_kernel<T, KIND, QT>), grid, dim3(COLS), 0, st, a);
}

template <typename T, int KIND>
int launch_q(const GdCall& d, const GramDiffPlan& p, hipStream_t st) {
    if constexpr (KIND == MXF_KD_SM) return dispatch<1, 2, 4, 8>(p.QT, [&](auto qt) { launch<T, KIND, decltype(qt)::value>(d, p, st); return 0; });
    else return dispatch<1, 2, 4, 8, 16>(p.QT, [&](auto qt) { launch<T, KIND, decltype(qt)::value>(d, p, st); return 0; });
}

int gram_diff_call(mxf_ctx* h, const char* name, const GdCall& d, hipStream_t st) {
    if (d.dtype != MXF_F32 && d.dtype != MXF_F64) return mxf_bad_dtype(h, name, d.dtype);
    GramDiffRequest r;
    r.kind = d.kind; r.elem_size = mxf_esize(d.dtype); r.bwd = d.bwd; r.S = d.S; r.N = d.N; r.N2 = d.N2; r.Q = d.Q; r.A = d.A; r.square = d.X2 == nullptr;
    r.has_X = d.X != nullptr; r.has_p = d.p0 && d.p1 && d.p2; r.has_K = d.bwd ? d.dK != nullptr : d.K != nullptr;
    r.sX = d.sX; r.sX2 = d.sX2; r.sp0 = d.sp0; r.sp1 = d.sp1; r.sp2 = d.sp2; r.sdiag = d.sdiag; r.ldk = d.ldk; r.sK = d.sK;
    const GramDiffPlan p = gram_diff_plan(r);
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    if (d.bwd && !d.dX && !d.dp0 && !d.dp1 && !d.dp2 && (r.square || !d.dX2)) return 0;      // nothing is asked for
    const int rc = dispatch<MXF_F32, MXF_F64>(d.dtype, [&](auto dt) {
        using T = mxf_elem_t<decltype(dt)::value>;
        return dispatch<MXF_KD_PERIODIC, MXF_KD_RQ, MXF_KD_SM>(d.kind, [&](auto kd) { return launch_q<T, decltype(kd)::value>(d, p, st); });
    });
    if (rc) MXF_FAIL(h, -2, "%s: no kernel for kind %d, Q tile %d", name, d.kind, p.QT);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

extern "C" int mxf_gram_diff(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int A,
                             const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                             const void* p0, int64_t strideS_p0, const void* p1, int64_t strideS_p1, const void* p2, int64_t strideS_p2, int ard,
                             const void* diag_add, int64_t strideS_diag, double jitter,
                             void* K_out, int64_t ldk, int64_t strideS_K, void* stream) {
    if (!h) return -1;
    return gram_diff_call(h, "mxf_gram_diff",
                          {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .A = A, .X = X, .sX = strideS_X, .X2 = X2, .sX2 = strideS_X2,
                           .p0 = p0, .sp0 = strideS_p0, .p1 = p1, .sp1 = strideS_p1, .p2 = p2, .sp2 = strideS_p2, .ard = ard,
                           .diag = X2 ? nullptr : diag_add, .sdiag = strideS_diag, .jitter = X2 ? 0.0 : jitter,
                           .K = K_out, .dK = nullptr, .ldk = ldk, .sK = strideS_K,
                           .dX = nullptr, .dX2 = nullptr, .dp0 = nullptr, .dp1 = nullptr, .dp2 = nullptr, .bwd = false},
                          (hipStream_t)stream);
}

extern "C" int mxf_gram_diff_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int A,
                                 const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                                 const void* p0, int64_t strideS_p0, const void* p1, int64_t strideS_p1, const void* p2, int64_t strideS_p2, int ard,
                                 const void* dK, int64_t lddk, int64_t strideS_dK,
                                 void* dX, void* dX2, void* dp0, void* dp1, void* dp2, void* stream) {
    if (!h) return -1;
    return gram_diff_call(h, "mxf_gram_diff_bwd",
                          {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .A = A, .X = X, .sX = strideS_X, .X2 = X2, .sX2 = strideS_X2,
                           .p0 = p0, .sp0 = strideS_p0, .p1 = p1, .sp1 = strideS_p1, .p2 = p2, .sp2 = strideS_p2, .ard = ard,
                           .diag = nullptr, .sdiag = 0, .jitter = 0.0,
                           .K = nullptr, .dK = dK, .ldk = lddk, .sK = strideS_dK,
                           .dX = dX, .dX2 = dX2, .dp0 = dp0, .dp1 = dp1, .dp2 = dp2, .bwd = true},
                          (hipStream_t)stream);
}
