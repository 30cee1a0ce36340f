// The k nearest rows of C for every row of X, all of them or (causal) only the rows that precede it (gfx950): the neighbour search of
// nearest-neighbour (Vecchia) GP regression.
//   idx[n, 0..k) = the candidates j (j < n with causal, else j < Nc) with the k smallest sum_q (X[n,q] - C[j,q])^2, d2[n, 0..k) those sums
// No reference counterpart.
//
// Nothing of size N x Nc is stored.  Row-owned, as nearest_kernel of nearest.hip: a thread owns a row n with its x in registers (Q padded to
// QP = 4 / 8 / 16 with zeros); the candidates, padded to QP once per call by the prep kernel, are uniform over the wavefront and arrive as
// scalar loads.  The running list is KP = 8 / 16 / 32 register slots (k rounded up), sorted ascending; a candidate is compared with the
// list's worst first -- the common case is that one compare -- and otherwise inserted by a fully unrolled pass of selects, so no register
// array is indexed dynamically and nothing spills.  Candidates are scanned in ascending j and every compare is a strict <, so the list is
// sorted by (d2, j) lexicographically.  A causal scan stops at the largest n of the wavefront.  The candidates are not split: the row blocks
// alone fill the device from N ~ 33 000 up.
#include "common.h"
#include "fused_plan.h"      // KNN_RB; knn_plan

namespace {

// cp (Nc, QP): the candidates padded with zeros
template <typename T, int QP>
__global__ __launch_bounds__(256) void knn_prep_kernel(int64_t Nc, int Q, const T* __restrict__ C, T* __restrict__ cp) {
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < Nc; m += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int q = 0; q < QP; ++q) cp[m * QP + q] = q < Q ? C[m * Q + q] : (T)0;
    }
}

// idx (N, k) and d2 (N, k; may be null).  A dead thread reads the last row, takes no candidate and writes nothing.
template <typename T, int QP, int KP>
__global__ __launch_bounds__(KNN_RB) void knn_kernel(int64_t N, int64_t Nc, int Q, int k, int causal, const T* __restrict__ X,
                                                     const T* __restrict__ cp, int32_t* __restrict__ idx, T* __restrict__ d2) {
    const int64_t n = (int64_t)blockIdx.x * KNN_RB + threadIdx.x;
    const bool live = n < N;
    const T* row = X + (live ? n : N - 1) * Q;
    T x[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) x[q] = q < Q ? row[q] : (T)0;
    T bd[KP];
    int32_t bi[KP];
#pragma unroll
    for (int t = 0; t < KP; ++t) { bd[t] = (T)INFINITY; bi[t] = -1; }
    // the candidates of this thread are j < lim; the wavefront scans to the largest lim of its rows
    const int64_t lim = !live ? 0 : (causal ? n : Nc);
    const int64_t wave_first = (int64_t)blockIdx.x * KNN_RB + (threadIdx.x & ~63);
    int64_t end = Nc;
    if (causal) { end = wave_first + 63; if (end > N - 1) end = N - 1; }          // the last live row of the wavefront
    end = (int64_t)__builtin_amdgcn_readfirstlane((int)end);                       // (uniform: the loads below stay scalar; end < 2^31)
    for (int64_t j = 0; j < end; ++j) {
        const T* c = cp + j * QP;
        T red = 0;
#pragma unroll
        for (int q = 0; q < QP; ++q) { const T d = x[q] - c[q]; red = fma(d, d, red); }
        if (j < lim && red < bd[KP - 1]) {
            // slot t takes its left neighbour where the candidate goes further left, the candidate where it goes here, else stays
#pragma unroll
            for (int t = KP - 1; t >= 1; --t) {
                const bool shift = red < bd[t - 1], here = red < bd[t];
                bd[t] = shift ? bd[t - 1] : (here ? red : bd[t]);
                bi[t] = shift ? bi[t - 1] : (here ? (int32_t)j : bi[t]);
            }
            const bool first = red < bd[0];
            bd[0] = first ? red : bd[0];
            bi[0] = first ? (int32_t)j : bi[0];
        }
    }
    if (live) {
#pragma unroll
        for (int t = 0; t < KP; ++t) {
            if (t < k) {
                idx[n * k + t] = bi[t];
                if (d2) d2[n * k + t] = bd[t];
            }
        }
    }
}

struct KnnArgs {
    int dtype = MXF_F32; int64_t N = 0, Nc = 0; int Q = 0, k = 0, causal = 0;
    const void *X = nullptr, *C = nullptr; int32_t* idx = nullptr; void* d2 = nullptr;
};

// ask the plan (fused_plan.h: knn_plan), carve, launch
template <typename T, int QP, int KP>
int knn_launch(mxf_handle h, const KnnArgs& a, const KnnPlan& p, hipStream_t st) {
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "mxf_knn: out of memory for %zu bytes of scratch", p.bytes);
    T* cp = (T*)(ws + p.at_cp);
    hipLaunchKernelGGL((knn_prep_kernel<T, QP>), dim3(grid_for(p.n_prep)), dim3(256), 0, st, a.Nc, a.Q, (const T*)a.C, cp);
    hipLaunchKernelGGL((knn_kernel<T, QP, KP>), dim3(p.grid), dim3(KNN_RB), 0, st, a.N, a.Nc, a.Q, a.k, a.causal, (const T*)a.X, (const T*)cp, a.idx,
                       (T*)a.d2);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

extern "C" int mxf_knn(mxf_handle h, int dtype, int64_t N, int64_t Nc, int Q, int k, int causal, const void* X, const void* C, int32_t* idx, void* d2,
                       void* stream) {
    if (!h) return -1;
    if (dtype != MXF_F32 && dtype != MXF_F64) MXF_FAIL(h, -2, "mxf_knn: bad dtype %d", dtype);
    const KnnArgs a = {.dtype = dtype, .N = N, .Nc = Nc, .Q = Q, .k = k, .causal = causal != 0, .X = X, .C = C, .idx = idx, .d2 = d2};
    const KnnPlan p = knn_plan({.esize = mxf_esize(dtype), .N = N, .Nc = Nc, .Q = Q, .k = k, .causal = causal != 0, .has_X = X != nullptr,
                                .has_C = C != nullptr, .has_idx = idx != nullptr, .same = C == X});
    if (p.rc) MXF_FAIL(h, p.rc, "mxf_knn: %s", p.refusal);
    return dispatch<MXF_F32, MXF_F64>(dtype, [&](auto dt) {
        return dispatch<4, 8, 16>(p.qp, [&](auto qp) {
            return dispatch<8, 16, 32>(p.kp, [&](auto kp) {
                return knn_launch<mxf_elem_t<decltype(dt)::value>, decltype(qp)::value, decltype(kp)::value>(h, a, p, (hipStream_t)stream);
            });
        });
    });
}
