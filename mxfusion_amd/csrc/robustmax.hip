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
#include "fused_plan.h"      // per_sample_plan
#include "likelihood.h"

namespace {

struct RmArgs {
    int S = 0; int64_t n = 0; int C = 0;
    const void* y = nullptr; int64_t ss_y = 0;
    const void* m = nullptr; int64_t ss_m = 0;
    const void* v = nullptr; int64_t ss_v = 0;
    const void* cot = nullptr; double scale = 1.0, l0 = 0.0, dl = 1.0;      // L0 and L1 - L0
    void *out = nullptr, *dm = nullptr, *dv = nullptr;       // RM_EXPECT: out (S), dm (S, n, C), dv (S, n); RM_PROBS: out = probs (S, n, C)
};
enum { RM_EXPECT = 0, RM_PROBS = 1 };

// a label as the kernel reads it: truncated toward zero and clamped to [0, C - 1]; NaN reads as 0
template <typename T>
__device__ __forceinline__ int rm_label(T y, int C) { return y > (T)0 ? (y < (T)(C - 1) ? (int)y : C - 1) : 0; }

template <typename T, int CP, int MODE>
__global__ __launch_bounds__(256) void robustmax_kernel(int S, int64_t n, int C, int chunks, const T* __restrict__ y, int64_t ss_y,
                                                        const T* __restrict__ m, int64_t ss_m, const T* __restrict__ v, int64_t ss_v,
                                                        const MxfQuadNodes<T> q, const T* __restrict__ cot, T scale, T l0, T dl,
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

// Grid: per_sample_plan of fused_plan.h; out[s] receives `chunks` atomics whatever S is.
template <typename T, int CP, int MODE>
int rm_launch(const RmArgs& a, const MxfQuadNodes<T>& q, hipStream_t st) {
    const PerSamplePlan p = per_sample_plan(a.S, a.n);
    hipLaunchKernelGGL((robustmax_kernel<T, CP, MODE>), dim3(p.grid), dim3(256), 0, st, a.S, a.n, a.C, p.chunks, (const T*)a.y, a.ss_y, (const T*)a.m,
                       a.ss_m, (const T*)a.v, a.ss_v, q, (const T*)a.cot, (T)a.scale, (T)a.l0, (T)a.dl, (T*)a.out, (T*)a.dm, (T*)a.dv);
    return 0;
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
    dispatch<MXF_F32, MXF_F64>(dtype, [&](auto dt) {
        using T = mxf_elem_t<decltype(dt)::value>;
        const MxfQuadNodes<T> q = mxf_quad_nodes<T>(nq, nodes, weights);
        return dispatch<4, 8, 16, 32>(a.C <= 4 ? 4 : (a.C <= 8 ? 8 : (a.C <= 16 ? 16 : 32)), [&](auto cp) {       // the row padded to registers
            return dispatch<RM_EXPECT, RM_PROBS>(
                mode, [&](auto md) { return rm_launch<T, decltype(cp)::value, decltype(md)::value>(a, q, (hipStream_t)stream); });
        });
    });
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
    const RmArgs a = {.S = S, .n = n, .C = C, .y = y, .ss_y = strideS_y, .m = m, .ss_m = strideS_m, .v = v, .ss_v = strideS_v, .cot = cot, .scale = scale,
                      .l0 = l0, .dl = l1 - l0, .out = out_acc, .dm = dm_acc, .dv = dv_acc};
    return run(h, "mxf_robustmax_expect", dtype, a, nq, nodes, weights, RM_EXPECT, stream);
}

extern "C" int mxf_robustmax_probs(mxf_handle h, int dtype, int S, int64_t n, int C, const void* m, int64_t strideS_m, const void* v,
                                   int64_t strideS_v, int nq, const double* nodes, const double* weights, void* probs, void* stream) {
    if (h && n > 0 && S > 0 && !probs) MXF_FAIL(h, -2, "mxf_robustmax_probs: null probs");
    const RmArgs a = {.S = S, .n = n, .C = C, .m = m, .ss_m = strideS_m, .v = v, .ss_v = strideS_v, .scale = 1.0, .l0 = 0.0, .dl = 1.0, .out = probs};
    return run(h, "mxf_robustmax_probs", dtype, a, nq, nodes, weights, RM_PROBS, stream);
}
