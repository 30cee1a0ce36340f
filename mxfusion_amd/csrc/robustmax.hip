// Robust-max multi-class likelihood under the marginals of a sparse variational GP (gfx950): a row of C latent values f_c ~ N(m_c, v)
// sharing one variance, a label y in {0 .. C-1}, p(y | f) = 1 - eps where f_y is the largest and eps / (C - 1) elsewhere
// (Hernandez-Lobato et al. 2011).  With p = P(f_y is the largest) by Gauss-Hermite quadrature over f_y (likelihood.h has the one-row math):
//   E[log p(y | f)] = L0 + p (L1 - L0),   L1 = log(1 - eps),   L0 = log(eps / (C - 1))
// and the gradients in m and v are the exact derivatives of the quadrature sum -- not Price's theorem: the integrand couples the C values of
// a row.  No reference counterpart: the reference has no non-Gaussian GP likelihood.
//
// The plan of likelihood.hip: n nq (C - 1) evaluations of log Phi over C + 2 loads per row, so the transcendental rate bounds it; the nodes
// travel in the kernel arguments (index uniform over the wavefront: scalar loads); a thread owns one row, a workgroup takes (sample, chunk)
// pairs off a one-dimensional grid and closes each with one block sum and ONE atomic into out[s]; dm, dv and probs have one writer per
// element and need no atomics.  The row lives in registers: the kernels are compiled for C padded to 4, 8, 16 and 32 with every loop over
// the classes unrolled, so no register array is indexed by a run-time value (the label selects through compares), and a padded class
// enters no product (no scratch up to C = 16; the instantiation for C <= 32 keeps part of the row there).  The label is read as an
// integer clamped to [0, C - 1]: no label value can index outside the row.
// Nothing is allocated and no table is read from global memory, so the entry points capture into a hipGraph.
#include "common.h"
#include "likelihood.h"

namespace {

template <typename T>
struct RmNodes { T x[MXF_LIK_MAX_NODES], w[MXF_LIK_MAX_NODES]; int nq; };

struct RmArgs {
    int S; int64_t n; int C;
    const void* y; int64_t ss_y;
    const void* m; int64_t ss_m;
    const void* v; int64_t ss_v;
    const void* cot; double scale, l0, dl;      // L0 and L1 - L0
    void *out, *dm, *dv;       // RM_EXPECT: out (S), dm (S, n, C), dv (S, n); RM_PROBS: out = probs (S, n, C)
};
enum { RM_EXPECT = 0, RM_PROBS = 1 };

// a label as the kernel reads it: truncated toward zero and clamped to [0, C - 1]; NaN reads as 0
template <typename T>
__device__ __forceinline__ int rm_label(T y, int C) { return y > (T)0 ? (y < (T)(C - 1) ? (int)y : C - 1) : 0; }

template <typename T, int CP, int MODE>
__global__ __launch_bounds__(256) void robustmax_kernel(int S, int64_t n, int C, int chunks, const T* __restrict__ y, int64_t ss_y,
                                                        const T* __restrict__ m, int64_t ss_m, const T* __restrict__ v, int64_t ss_v,
                                                        const RmNodes<T> q, const T* __restrict__ cot, T scale, T l0, T dl,
                                                        T* __restrict__ out, T* __restrict__ dm, T* __restrict__ dv) {
    __shared__ T red[16];
    const int64_t pairs = (int64_t)S * chunks, nC = n * C;
    const bool grad = MODE == RM_EXPECT && (dm || dv);
    for (int64_t p = blockIdx.x; p < pairs; p += gridDim.x) {       // (uniform over the workgroup: block_sum's barriers are safe)
        const int64_t s = p / chunks, ch = p - s * chunks;
        const T *ms = m + s * ss_m, *vs = v + s * ss_v;
        T acc = 0;
        for (int64_t r = ch * 256 + threadIdx.x; r < n; r += (int64_t)chunks * 256) {
            T mr[CP], g[CP], gv = 0;
#pragma unroll
            for (int c = 0; c < CP; ++c) mr[c] = c < C ? ms[r * C + c] : (T)0;
            const T vr = vs[r];
            if constexpr (MODE == RM_PROBS) {
                for (int j = 0; j < C; ++j) out[s * nC + r * C + j] = mxf_robustmax_row<T, CP, false>(C, j, mr, vr, q, g, gv);
            } else {
                const int yi = rm_label<T>(y[s * ss_y + r], C);
                if (grad) {
                    const T w = (cot ? cot[s] * scale : scale) * dl;
                    acc += l0 + dl * mxf_robustmax_row<T, CP, true>(C, yi, mr, vr, q, g, gv);
                    if (dm) {
#pragma unroll
                        for (int c = 0; c < CP; ++c)
                            if (c < C) dm[s * nC + r * C + c] += w * g[c];
                    }
                    if (dv) dv[s * n + r] += w * gv;
                } else {
                    acc += l0 + dl * mxf_robustmax_row<T, CP, false>(C, yi, mr, vr, q, g, gv);
                }
            }
        }
        if constexpr (MODE == RM_EXPECT) {
            acc = block_sum<T>(acc, red);
            if (threadIdx.x == 0) atomic_add(out + s, acc * scale);
        }
    }
}

// Grid: lik_plan of likelihood.hip restated -- up to 512 chunks of 256 rows per sample, fewer where S of them would pass 8192 workgroups, at
// most 65 536 workgroups that loop over the rest of the pairs; out[s] receives `chunks` atomics whatever S is.
struct RmPlan { int chunks; unsigned grid; };
static inline RmPlan rm_plan(int S, int64_t n) {
    int64_t c = (n + 255) / 256;
    if (c > 512) c = 512;
    const int64_t fit = 8192 / (int64_t)S;
    if (c > fit) c = fit;
    if (c < 1) c = 1;
    int64_t g = (int64_t)S * c;
    if (g > 65536) g = 65536;
    return {(int)c, (unsigned)g};
}

template <typename T, int CP>
void launch_cp(const RmArgs& a, const RmNodes<T>& q, int mode, hipStream_t st) {
    const RmPlan p = rm_plan(a.S, a.n);
    const dim3 grid(p.grid), block(256);
#define MXF_RM_LAUNCH(MODE)                                                                                                               \
    hipLaunchKernelGGL((robustmax_kernel<T, CP, MODE>), grid, block, 0, st, a.S, a.n, a.C, p.chunks, (const T*)a.y, a.ss_y, (const T*)a.m, \
                       a.ss_m, (const T*)a.v, a.ss_v, q, (const T*)a.cot, (T)a.scale, (T)a.l0, (T)a.dl, (T*)a.out, (T*)a.dm, (T*)a.dv)
    if (mode == RM_PROBS) MXF_RM_LAUNCH(RM_PROBS);
    else MXF_RM_LAUNCH(RM_EXPECT);
#undef MXF_RM_LAUNCH
}

template <typename T>
void launch(const RmArgs& a, int nq, const double* nodes, const double* weights, int mode, hipStream_t st) {
    RmNodes<T> q;
    q.nq = nq;
    for (int k = 0; k < MXF_LIK_MAX_NODES; ++k) {
        q.x[k] = k < nq ? (T)(1.41421356237309504880 * nodes[k]) : (T)0;
        q.w[k] = k < nq ? (T)(0.56418958354775628695 * weights[k]) : (T)0;
    }
    if (a.C <= 4) launch_cp<T, 4>(a, q, mode, st);
    else if (a.C <= 8) launch_cp<T, 8>(a, q, mode, st);
    else if (a.C <= 16) launch_cp<T, 16>(a, q, mode, st);
    else launch_cp<T, 32>(a, q, mode, st);
}

// argument checks shared by the entry points (those of run() in likelihood.hip), then the launch
int run(mxf_handle h, const char* name, int dtype, const RmArgs& a, int nq, const double* nodes, const double* weights, int mode, void* stream) {
    if (!h) return -1;
    if (a.n <= 0 || a.S <= 0) return 0;
    if (a.C < 2 || a.C > MXF_ROBUSTMAX_MAX_C) MXF_FAIL(h, -3, "%s: C = %d outside the 2 to %d classes of a row", name, a.C, MXF_ROBUSTMAX_MAX_C);
    if (dtype != MXF_F32 && dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, dtype);
    if (nq < 1 || nq > MXF_LIK_MAX_NODES || !nodes || !weights)
        MXF_FAIL(h, -2, "%s: 1 <= nq <= %d quadrature nodes and weights (host arrays), got nq = %d", name, MXF_LIK_MAX_NODES, nq);
    if (!a.m || !a.v || (mode == RM_EXPECT && !a.y)) MXF_FAIL(h, -2, "%s: null y, m or v", name);
    if ((a.ss_y != 0 && a.ss_y != a.n) || (a.ss_m != 0 && a.ss_m != a.n * a.C) || (a.ss_v != 0 && a.ss_v != a.n))
        MXF_FAIL(h, -2, "%s: a sample stride must be 0 or the elements of one sample (y, v: n; m: n C)", name);
    if (dtype == MXF_F32) launch<float>(a, nq, nodes, weights, mode, (hipStream_t)stream);
    else launch<double>(a, nq, nodes, weights, mode, (hipStream_t)stream);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

extern "C" int mxf_robustmax_expect(mxf_handle h, int dtype, int S, int64_t n, int C, const void* y, int64_t strideS_y, const void* m,
                                    int64_t strideS_m, const void* v, int64_t strideS_v, int nq, const double* nodes, const double* weights,
                                    double eps, const void* cot, double scale, void* out_acc, void* dm_acc, void* dv_acc, void* stream) {
    if (h && n > 0 && S > 0 && !(eps > 0.0 && eps < 1.0)) MXF_FAIL(h, -2, "mxf_robustmax_expect: eps = %g outside (0, 1)", eps);
    if (h && n > 0 && S > 0 && !out_acc) MXF_FAIL(h, -2, "mxf_robustmax_expect: null out");
    const double l0 = C >= 2 ? log(eps / (double)(C - 1)) : 0.0, l1 = log1p(-eps);
    const RmArgs a = {S, n, C, y, strideS_y, m, strideS_m, v, strideS_v, cot, scale, l0, l1 - l0, out_acc, dm_acc, dv_acc};
    return run(h, "mxf_robustmax_expect", dtype, a, nq, nodes, weights, RM_EXPECT, stream);
}

extern "C" int mxf_robustmax_probs(mxf_handle h, int dtype, int S, int64_t n, int C, const void* m, int64_t strideS_m, const void* v,
                                   int64_t strideS_v, int nq, const double* nodes, const double* weights, void* probs, void* stream) {
    if (h && n > 0 && S > 0 && !probs) MXF_FAIL(h, -2, "mxf_robustmax_probs: null probs");
    const RmArgs a = {S, n, C, nullptr, 0, m, strideS_m, v, strideS_v, nullptr, 1.0, 0.0, 1.0, probs, nullptr, nullptr};
    return run(h, "mxf_robustmax_probs", dtype, a, nq, nodes, weights, RM_PROBS, stream);
}
