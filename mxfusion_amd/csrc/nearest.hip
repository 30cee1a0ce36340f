// Nearest-centre assignment and one Lloyd iteration of k-means (gfx950): the primitive of initialising inducing inputs from data.
//   idx[n] = argmin_m sum_q (X[n,q] - C[m,q])^2,  d2[n] = that minimum                                                     (N)
//   C_new[m] = mean of the rows assigned to m (C[m] where none is), counts[m], inertia = sum_n d2[n]                         (M, Q), (M), (1)
// No reference counterpart: the reference draws its inducing inputs from a standard normal.
//
// Nothing of size N x M is stored.  Row-owned, as kmv_fwd_kernel of kmv.hip: a thread owns a row n with its x in registers (Q padded to
// QP = 4 / 8 / 16 with zeros); the centres, padded to QP once per call by the prep kernel, are uniform over the wavefront and arrive as
// scalar loads.  The distance is the difference form summed in T; m is scanned in ascending order with a strict <, so the smallest index wins
// an exact tie.  M is not split: the row blocks alone fill the device from N ~ 33 000 up, and a small N is a small problem.
//
// The step adds, after the assignment, a thread's row into zeroed double scratch (M x QP sums, M 64-bit counts) with atomics; the inertia
// is reduced per wavefront in double, then one atomic.  The close kernel divides, narrows with one rounding and copies C[m] where the
// count is 0.  No LDS pre-reduction of the sums.
#include "common.h"
#include "fused_plan.h"      // NEAREST_RB; nearest_plan

namespace {

// cp (M, QP): the centres padded with zeros
template <typename T, int QP>
__global__ __launch_bounds__(256) void nearest_prep_kernel(int64_t M, int Q, const T* __restrict__ C, T* __restrict__ cp) {
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int q = 0; q < QP; ++q) cp[m * QP + q] = q < Q ? C[m * Q + q] : (T)0;
    }
}

// idx, d2 (either may be null) and, with STEP, the sums of the Lloyd iteration.  A dead thread scans for the last row and writes nothing.
template <typename T, int QP, bool STEP>
__global__ __launch_bounds__(NEAREST_RB) void nearest_kernel(int64_t N, int64_t M, int Q, const T* __restrict__ X, const T* __restrict__ cp,
                                                             int32_t* __restrict__ idx, T* __restrict__ d2, double* __restrict__ sums,
                                                             unsigned long long* __restrict__ cnt, double* __restrict__ inertia) {
    const int64_t n = (int64_t)blockIdx.x * NEAREST_RB + threadIdx.x;
    const bool live = n < N;
    const T* row = X + (live ? n : N - 1) * Q;
    T x[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) x[q] = q < Q ? row[q] : (T)0;
    T best = (T)INFINITY;
    int32_t bi = 0;
    for (int64_t m = 0; m < M; ++m) {         // c_m is uniform over the wavefront: scalar loads
        const T* c = cp + m * QP;
        T red = 0;
#pragma unroll
        for (int q = 0; q < QP; ++q) { const T d = x[q] - c[q]; red = fma(d, d, red); }
        if (red < best) { best = red; bi = (int32_t)m; }
    }
    if (live) {
        if (idx) idx[n] = bi;
        if (d2) d2[n] = best;
    }
    if (STEP) {
        if (live) {
#pragma unroll
            for (int q = 0; q < QP; ++q)
                if (q < Q) atomic_add(sums + (int64_t)bi * QP + q, (double)x[q]);
            atomicAdd(cnt + bi, 1ull);
        }
        const double t = wave_sum(live ? (double)best : 0.0);
        if ((threadIdx.x & 63) == 0) atomic_add(inertia, t);
    }
}

// C_new[m] = sums[m] / counts[m], rounded once, or C[m] where the count is 0; counts and the inertia leave the scratch
template <typename T, int QP>
__global__ __launch_bounds__(256) void kmeans_close_kernel(int64_t M, int Q, const T* __restrict__ C, const double* __restrict__ sums,
                                                           const unsigned long long* __restrict__ cnt, const double* __restrict__ inertia_acc,
                                                           T* __restrict__ C_new, int64_t* __restrict__ counts, double* __restrict__ inertia) {
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = cnt[m];
        counts[m] = (int64_t)k;
        for (int q = 0; q < Q; ++q) C_new[m * Q + q] = k ? (T)(sums[m * QP + q] / (double)k) : C[m * Q + q];
        if (m == 0) inertia[0] = inertia_acc[0];
    }
}

struct NearestArgs {
    int dtype = MXF_F32; int64_t N = 0, M = 0; int Q = 0;
    const void *X = nullptr, *C = nullptr; int32_t* idx = nullptr; void* d2 = nullptr;                 // mxf_nearest
    void* C_new = nullptr; int64_t* counts = nullptr; double* inertia = nullptr;                       // mxf_kmeans_step
};

// ask the plan (fused_plan.h: nearest_plan), carve, launch
template <typename T, int QP>
int nearest_launch(mxf_handle h, const char* name, const NearestArgs& a, const NearestPlan& p, bool step, hipStream_t st) {
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    T* cp = (T*)(ws + p.at_cp);
    hipLaunchKernelGGL((nearest_prep_kernel<T, QP>), dim3(grid_for(p.n_prep)), dim3(256), 0, st, a.M, a.Q, (const T*)a.C, cp);
    if (!step) {
        hipLaunchKernelGGL((nearest_kernel<T, QP, false>), dim3(p.grid), dim3(NEAREST_RB), 0, st, a.N, a.M, a.Q, (const T*)a.X, (const T*)cp, a.idx,
                           (T*)a.d2, (double*)nullptr, (unsigned long long*)nullptr, (double*)nullptr);
    } else {
        MXF_HIP(h, hipMemsetAsync(ws + p.at_zero, 0, p.zero_bytes, st));
        double *sums = (double*)(ws + p.at_sums), *iacc = (double*)(ws + p.at_inertia);
        unsigned long long* cnt = (unsigned long long*)(ws + p.at_counts);
        hipLaunchKernelGGL((nearest_kernel<T, QP, true>), dim3(p.grid), dim3(NEAREST_RB), 0, st, a.N, a.M, a.Q, (const T*)a.X, (const T*)cp, a.idx,
                           (T*)nullptr, sums, cnt, iacc);
        hipLaunchKernelGGL((kmeans_close_kernel<T, QP>), dim3(grid_for(p.n_close)), dim3(256), 0, st, a.M, a.Q, (const T*)a.C, (const double*)sums,
                           (const unsigned long long*)cnt, (const double*)iacc, (T*)a.C_new, a.counts, a.inertia);
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

int run(mxf_handle h, const char* name, const NearestArgs& a, bool step, void* stream) {
    if (!h) return -1;
    if (a.dtype != MXF_F32 && a.dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, a.dtype);
    const NearestPlan p = nearest_plan({.esize = mxf_esize(a.dtype), .step = step, .N = a.N, .M = a.M, .Q = a.Q, .has_X = a.X != nullptr,
                                        .has_C = a.C != nullptr, .has_idx = a.idx != nullptr, .has_Cnew = a.C_new != nullptr,
                                        .has_counts = a.counts != nullptr, .has_inertia = a.inertia != nullptr,
                                        .alias = step && a.C_new == a.C});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    return dispatch<MXF_F32, MXF_F64>(a.dtype, [&](auto dt) {
        return dispatch<4, 8, 16>(p.qp, [&](auto qp) {
            return nearest_launch<mxf_elem_t<decltype(dt)::value>, decltype(qp)::value>(h, name, a, p, step, (hipStream_t)stream);
        });
    });
}

}  // namespace

extern "C" int mxf_nearest(mxf_handle h, int dtype, int64_t N, int64_t M, int Q, const void* X, const void* C, int32_t* idx, void* d2, void* stream) {
    const NearestArgs a = {.dtype = dtype, .N = N, .M = M, .Q = Q, .X = X, .C = C, .idx = idx, .d2 = d2};
    return run(h, "mxf_nearest", a, false, stream);
}

extern "C" int mxf_kmeans_step(mxf_handle h, int dtype, int64_t N, int64_t M, int Q, const void* X, const void* C, void* C_new, int32_t* idx,
                               int64_t* counts, double* inertia, void* stream) {
    const NearestArgs a = {.dtype = dtype, .N = N, .M = M, .Q = Q, .X = X, .C = C, .idx = idx, .C_new = C_new, .counts = counts, .inertia = inertia};
    return run(h, "mxf_kmeans_step", a, true, stream);
}
