// Gauss-Hermite expectations of a non-Gaussian likelihood under the marginals N(f; m, v) of a sparse variational GP (gfx950):
//   E[g(f)] ~ sum_k w_k g(m + sqrt(2 max(v, 0)) x_k),   w_k the Gauss-Hermite weights over sqrt(pi),   g = log p(y | f)  (likelihood.h)
// with d/dm = sum_k w_k g'(f_k), the exact derivative of that sum, and d/dv = 1/2 sum_k w_k g''(f_k): Price's theorem, which equals the
// derivative of the sum only up to the quadrature error (include/mxf_gp.h) but is finite at v = 0, where the chain rule through
// sqrt(v) is 0 / 0.  No reference counterpart: the reference has no non-Gaussian GP likelihood.
//
// Streaming: three loads per element under nq link-function evaluations, so the transcendental rate bounds it, not memory.  The nodes
// travel in the kernel arguments (two arrays of MXF_LIK_MAX_NODES, scaled on the host to sqrt(2) x_k and w_k / sqrt(pi) and rounded to
// T once): the index k is uniform over the wavefront, so they are scalar loads from the argument segment and nothing is re-read from a
// table in global memory; the library allocates and copies nothing.  A thread owns one row of m (its P columns share v and the
// sqrt), a workgroup takes (sample, chunk) pairs off a one-dimensional grid and closes each with one block sum and ONE atomic into out[s]
// (per_sample_plan of fused_plan.h, as univariate_ps_kernel); the gradients and the un-reduced outputs have one writer per element and need no atomics.
#include "common.h"
#include "fused_plan.h"      // per_sample_plan
#include "likelihood.h"

namespace {

struct LikArgs {
    int S = 0; int64_t n = 0; int P = 0;
    const void* y = nullptr; int64_t ss_y = 0;
    const void* m = nullptr; int64_t ss_m = 0;
    const void* v = nullptr; int64_t ss_v = 0;
    const void* cot = nullptr; double scale = 1.0;
    void *out = nullptr, *dm = nullptr, *dv = nullptr;       // LIK_REDUCED: out (S), dm (S, n, P), dv (S, n); LIK_ELEM: out (S, n, P); LIK_MOMENTS: out = E[mu], dm = E[mu^2], both (S, n, P)
};
enum { LIK_REDUCED = 0, LIK_ELEM = 1, LIK_MOMENTS = 2 };

template <typename T, int KIND, int MODE>
__global__ __launch_bounds__(256) void lik_kernel(int S, int64_t n, int P, int chunks, const T* __restrict__ y, int64_t ss_y,
                                                  const T* __restrict__ m, int64_t ss_m, const T* __restrict__ v, int64_t ss_v,
                                                  const MxfQuadNodes<T> q, const T* __restrict__ cot, T scale, T* __restrict__ out,
                                                  T* __restrict__ dm, T* __restrict__ dv) {
    __shared__ T red[16];
    const int64_t pairs = (int64_t)S * chunks, nP = n * P;
    const bool grad = MODE == LIK_REDUCED && (dm || dv);
    for (int64_t p = blockIdx.x; p < pairs; p += gridDim.x) {       // (uniform over the workgroup: block_sum's barriers are safe)
        const int64_t s = p / chunks, c = p - s * chunks;
        const T *ys = y ? y + s * ss_y : nullptr, *ms = m + s * ss_m, *vs = v + s * ss_v;
        const T w = MODE == LIK_REDUCED ? (cot ? cot[s] * scale : scale) : scale;
        T acc = 0;
        for (int64_t r = c * 256 + threadIdx.x; r < n; r += (int64_t)chunks * 256) {
            const T vr = vs[r], sd = sqrt(vr > (T)0 ? vr : (T)0);       // (the nodes carry the sqrt 2)
            T gv = 0;
            for (int j = 0; j < P; ++j) {
                const int64_t e = r * P + j;
                const T mr = ms[e];
                if constexpr (MODE == LIK_MOMENTS) {
                    T e1 = 0, e2 = 0;
                    for (int k = 0; k < q.nq; ++k) {
                        const T u = MxfLik<T, KIND>::mu(mr + sd * q.x[k]);
                        e1 += q.w[k] * u;
                        e2 += q.w[k] * u * u;
                    }
                    out[s * nP + e] = e1;
                    dm[s * nP + e] = e2;
                } else {
                    MxfLik<T, KIND> l;
                    l.set(ys[e]);
                    T e0 = 0, e1 = 0, e2 = 0;
                    for (int k = 0; k < q.nq; ++k) {
                        T g, g1, g2;
                        l.eval(mr + sd * q.x[k], g, g1, g2);
                        e0 += q.w[k] * g;
                        e1 += q.w[k] * g1;
                        e2 += q.w[k] * g2;
                    }
                    if constexpr (MODE == LIK_ELEM) out[s * nP + e] = scale * e0;
                    else {
                        acc += e0;
                        if (grad) {
                            if (dm) dm[s * nP + e] += w * e1;
                            gv += e2;
                        }
                    }
                }
            }
            if (grad && dv) dv[s * n + r] += (T)0.5 * w * gv;
        }
        if constexpr (MODE == LIK_REDUCED) {
            if (out) { acc = block_sum<T>(acc, red); if (threadIdx.x == 0) atomic_add(out + s, acc * scale); }
        }
    }
}

template <typename T, int KIND, int MODE>
int lik_launch(const LikArgs& a, const MxfQuadNodes<T>& q, hipStream_t st) {
    const PerSamplePlan p = per_sample_plan(a.S, a.n);
    hipLaunchKernelGGL((lik_kernel<T, KIND, MODE>), dim3(p.grid), dim3(256), 0, st, a.S, a.n, a.P, p.chunks, (const T*)a.y, a.ss_y, (const T*)a.m,
                       a.ss_m, (const T*)a.v, a.ss_v, q, (const T*)a.cot, (T)a.scale, (T*)a.out, (T*)a.dm, (T*)a.dv);
    return 0;
}

// argument checks shared by the entry points, then the launch
int run(mxf_handle h, const char* name, int kind, int dtype, const LikArgs& a, int nq, const double* nodes, const double* weights, int mode,
        void* stream) {
    if (!h) return -1;
    if (a.n <= 0 || a.S <= 0 || a.P <= 0) return 0;
    if (kind < MXF_LIK_BERNOULLI_LOGIT || kind > MXF_LIK_POISSON_EXP) MXF_FAIL(h, -2, "%s: unknown likelihood kind %d", name, kind);
    if (dtype != MXF_F32 && dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, dtype);
    if (nq < 1 || nq > MXF_LIK_MAX_NODES || !nodes || !weights)
        MXF_FAIL(h, -2, "%s: 1 <= nq <= %d quadrature nodes and weights (host arrays), got nq = %d", name, MXF_LIK_MAX_NODES, nq);
    if (!a.m || !a.v || (mode != LIK_MOMENTS && !a.y)) MXF_FAIL(h, -2, "%s: null y, m or v", name);
    if ((a.ss_y != 0 && a.ss_y != a.n * a.P) || (a.ss_m != 0 && a.ss_m != a.n * a.P) || (a.ss_v != 0 && a.ss_v != a.n))
        MXF_FAIL(h, -2, "%s: a sample stride must be 0 or the elements of one sample (y, m: n P; v: n)", name);
    dispatch<MXF_F32, MXF_F64>(dtype, [&](auto dt) {
        using T = mxf_elem_t<decltype(dt)::value>;
        const MxfQuadNodes<T> q = mxf_quad_nodes<T>(nq, nodes, weights);
        return dispatch<MXF_LIK_BERNOULLI_LOGIT, MXF_LIK_BERNOULLI_PROBIT, MXF_LIK_POISSON_EXP>(kind, [&](auto k) {
            return dispatch<LIK_REDUCED, LIK_ELEM, LIK_MOMENTS>(
                mode, [&](auto md) { return lik_launch<T, decltype(k)::value, decltype(md)::value>(a, q, (hipStream_t)stream); });
        });
    });
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

static_assert(MXF_LIK_BERNOULLI_LOGIT == MXF_LIK_KIND_LOGIT && MXF_LIK_BERNOULLI_PROBIT == MXF_LIK_KIND_PROBIT &&
              MXF_LIK_POISSON_EXP == MXF_LIK_KIND_POISSON, "likelihood.h numbers its kinds like include/mxf_gp.h");

extern "C" int mxf_lik_expect(mxf_handle h, int kind, int dtype, int S, int64_t n, int P, const void* y, int64_t strideS_y, const void* m,
                              int64_t strideS_m, const void* v, int64_t strideS_v, int nq, const double* nodes, const double* weights,
                              const void* cot, double scale, void* out_acc, void* dm_acc, void* dv_acc, void* stream) {
    const LikArgs a = {.S = S, .n = n, .P = P, .y = y, .ss_y = strideS_y, .m = m, .ss_m = strideS_m, .v = v, .ss_v = strideS_v, .cot = cot, .scale = scale,
                       .out = out_acc, .dm = dm_acc, .dv = dv_acc};
    return run(h, "mxf_lik_expect", kind, dtype, a, nq, nodes, weights, LIK_REDUCED, stream);
}

extern "C" int mxf_lik_expect_elem(mxf_handle h, int kind, int dtype, int S, int64_t n, int P, const void* y, int64_t strideS_y,
                                   const void* m, int64_t strideS_m, const void* v, int64_t strideS_v, int nq, const double* nodes,
                                   const double* weights, double scale, void* out, void* stream) {
    if (h && n > 0 && S > 0 && P > 0 && !out) MXF_FAIL(h, -2, "mxf_lik_expect_elem: null out");
    const LikArgs a = {.S = S, .n = n, .P = P, .y = y, .ss_y = strideS_y, .m = m, .ss_m = strideS_m, .v = v, .ss_v = strideS_v, .scale = scale, .out = out};
    return run(h, "mxf_lik_expect_elem", kind, dtype, a, nq, nodes, weights, LIK_ELEM, stream);
}

extern "C" int mxf_lik_moments(mxf_handle h, int kind, int dtype, int S, int64_t n, int P, const void* m, int64_t strideS_m, const void* v,
                               int64_t strideS_v, int nq, const double* nodes, const double* weights, void* e1, void* e2, void* stream) {
    if (h && n > 0 && S > 0 && P > 0 && (!e1 || !e2)) MXF_FAIL(h, -2, "mxf_lik_moments: null output");
    const LikArgs a = {.S = S, .n = n, .P = P, .m = m, .ss_m = strideS_m, .v = v, .ss_v = strideS_v, .scale = 1.0, .out = e1, .dm = e2};
    return run(h, "mxf_lik_moments", kind, dtype, a, nq, nodes, weights, LIK_MOMENTS, stream);
}
