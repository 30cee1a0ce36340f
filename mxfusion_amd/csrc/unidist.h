// The elementwise two-parameter log-densities (gfx950) that univariate.hip (Gamma, Gamma by mean and variance, Beta, Laplace, Uniform,
// Bernoulli, Normal by mean and precision) and elementwise.hip (the per-sample Normal) are built from: one evaluation struct per kind, the three kernels over it and
// their launcher.  Everything is in an unnamed namespace: each file instantiates the kinds of its own entry points and nothing is shared
// at link time.
#pragma once
#include "common.h"
#include "fused_plan.h"      // per_sample_plan
#include "special.h"

namespace {

// the Normal by mean and variance as a kind of UniDist; not part of the C ABI (mxf_normal_logpdf_ps* have no `kind` argument)
constexpr int MXF_D_NORMAL_ = 100;

// One (a, b) parameter pair: set() holds what does not depend on x, eval() gives log p(x) and its three partial derivatives.
// The x-free terms of Gamma and Beta are differences of lgamma values of a few hundred (lgamma(100) = 359: one float32 ulp is 3e-5), so
// set() forms them in double for either T -- once per element where the parameters have no sample axis.
template <typename T, int KIND>
struct UniDist {
    T a, b;         // GAMMA_MV: the (alpha, beta) that the mean and variance stand for
    T c;            // the terms of log p without x
    T ca, cb;       // d c / d a, d c / d b
    T inv;          // LAPLACE 1/scale, UNIFORM 1/(high - low), GAMMA_MV and NORMAL 1/variance, NORMAL_PREC 1/precision (with grad only)

    __device__ __forceinline__ void set(T pa, T pb, bool grad) {
        a = pa; b = pb; ca = cb = inv = 0;
        if constexpr (KIND == MXF_D_GAMMA || KIND == MXF_D_GAMMA_MV) {
            if constexpr (KIND == MXF_D_GAMMA_MV) { inv = (T)1 / pb; b = pa * inv; a = pa * b; }
            const T lb = log(b);
            c = (T)((double)a * log((double)b) - mxf_lgamma((double)a));
            if (grad) { ca = lb - mxf_digamma(a); cb = a / b; }
        } else if constexpr (KIND == MXF_D_BETA) {
            c = (T)(mxf_lgamma((double)a + (double)b) - mxf_lgamma((double)a) - mxf_lgamma((double)b));
            if (grad) { const T ps = mxf_digamma(a + b); ca = ps - mxf_digamma(a); cb = ps - mxf_digamma(b); }
        } else if constexpr (KIND == MXF_D_LAPLACE) {
            inv = (T)1 / b;
            c = -log((T)2 * b);
        } else if constexpr (KIND == MXF_D_BERNOULLI) {
            c = 0;                                       // a is prob_true; b is unused (the caller passes a again)
        } else if constexpr (KIND == MXF_D_NORMAL_) {    // the terms of normal_logpdf_kernel (elementwise.hip)
            inv = (T)1 / b;
            c = (T)(-0.5 * 1.8378770664093453) - (T)0.5 * log(b);
        } else if constexpr (KIND == MXF_D_NORMAL_PREC) {
            if (grad) inv = (T)1 / b;
            c = (T)0.5 * log(b) - (T)(0.5 * 1.8378770664093453);
        } else {
            inv = (T)1 / (b - a);
            c = -log(b - a);
        }
    }

    // ga, gb are with respect to the parameters as the caller passed them (GAMMA_MV: mean and variance).  false: x is outside the support,
    // log p = -inf has no gradient -- the caller adds nothing there, whatever the weight (a cotangent of inf or NaN stays out of da, db)
    __device__ __forceinline__ bool eval(T x, T& lp, T& gx, T& ga, T& gb) const {
        if constexpr (KIND == MXF_D_GAMMA || KIND == MXF_D_GAMMA_MV) {
            const T lx = log(x);
            lp = (a - (T)1) * lx - b * x + c;
            gx = (a - (T)1) / x - b;
            const T gA = lx + ca, gB = cb - x;
            if constexpr (KIND == MXF_D_GAMMA_MV) {      // b = m / v, a = m b:  da/dm = 2 b, da/dv = -b^2, db/dm = 1/v, db/dv = -b/v
                ga = (T)2 * b * gA + inv * gB;
                gb = -b * (b * gA + inv * gB);
            } else { ga = gA; gb = gB; }
        } else if constexpr (KIND == MXF_D_BETA) {
            const T lx = log(x), l1x = log1p(-x);
            lp = (a - (T)1) * lx + (b - (T)1) * l1x + c;
            gx = (a - (T)1) / x - (b - (T)1) / ((T)1 - x);
            ga = lx + ca;
            gb = l1x + cb;
        } else if constexpr (KIND == MXF_D_LAPLACE) {
            const T d = x - a, sg = d > (T)0 ? (T)1 : (d < (T)0 ? (T)-1 : (T)0);
            lp = c - fabs(d) * inv;
            gx = -sg * inv;
            ga = sg * inv;
            gb = (fabs(d) * inv - (T)1) * inv;
        } else if constexpr (KIND == MXF_D_BERNOULLI) {
            const T la = log(a), l1a = log1p(-a);
            lp = x * la + ((T)1 - x) * l1a;
            gx = la - l1a;
            ga = x / a - ((T)1 - x) / ((T)1 - a);
            gb = 0;
        } else if constexpr (KIND == MXF_D_NORMAL_) {
            const T d = x - a;
            lp = c - (T)0.5 * d * d * inv;
            gx = -d * inv;
            ga = d * inv;
            gb = (T)0.5 * (d * d * inv * inv - inv);
        } else if constexpr (KIND == MXF_D_NORMAL_PREC) {
            const T d = x - a;
            lp = c - (T)0.5 * b * d * d;
            gx = -b * d;
            ga = b * d;
            gb = (T)0.5 * (inv - d * d);
        } else {
            const bool in = a <= x && x < b;
            lp = in ? c : -(T)INFINITY;
            gx = 0;
            ga = inv;
            gb = -inv;
            return in;
        }
        return true;
    }
};

// out += scale * sum log p(x | a, b);  dx, da, db += w * (d log p / d .)  with  w = scale  or, given a cotangent, w = scale * cot.
// The cotangent is read at cot[s * cs_s + i * cs_i]: (n, 1) for one per sample and element, (1, 0) for the per-sample weights w[s].
// A parameter is a single element (n_p == 1), per element (n_p == n, sample stride 0: its gradient is summed over the samples) or per
// sample and element (sample stride n: its gradient is (S, n) like dx).
template <typename T, int KIND>
__global__ __launch_bounds__(256) void univariate_logpdf_kernel(int S, int64_t n, const T* __restrict__ x, const T* __restrict__ a, int64_t n_a,
                                                                int64_t ss_a, const T* __restrict__ b, int64_t n_b, int64_t ss_b, T scale,
                                                                const T* __restrict__ cot, int64_t cs_s, int64_t cs_i, T* __restrict__ out,
                                                                T* __restrict__ dx, T* __restrict__ da, T* __restrict__ db) {
    __shared__ T red[16];
    const bool grad = dx || da || db, per_sample = ss_a != 0 || ss_b != 0;
    T acc = 0, ga_b = 0, gb_b = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ia = n_a == 1 ? 0 : i, ib = n_b == 1 ? 0 : i;
        UniDist<T, KIND> d;
        if (!per_sample) d.set(a[ia], b[ib], grad);
        T ga = 0, gb = 0;
        for (int s = 0; s < S; ++s) {
            const int64_t e = (int64_t)s * n + i;
            if (per_sample) d.set(a[(int64_t)s * ss_a + ia], b[(int64_t)s * ss_b + ib], grad);
            T lp, gx, pa, pb;
            const bool live = d.eval(x[e], lp, gx, pa, pb);
            acc += lp;
            if (grad && live) {
                const T w = cot ? cot[(int64_t)s * cs_s + i * cs_i] * scale : scale;
                if (dx) dx[e] += w * gx;
                if (ss_a != 0) { if (da) da[e] += w * pa; } else ga += w * pa;
                if (ss_b != 0) { if (db) db[e] += w * pb; } else gb += w * pb;
            }
        }
        if (da && ss_a == 0) { if (n_a == 1) ga_b += ga; else da[i] += ga; }
        if (db && ss_b == 0) { if (n_b == 1) gb_b += gb; else db[i] += gb; }
    }
    if (out) { acc = block_sum<T>(acc, red); if (threadIdx.x == 0) atomic_add(out, acc * scale); }
    if (da && ss_a == 0 && n_a == 1) { ga_b = block_sum<T>(ga_b, red); if (threadIdx.x == 0) atomic_add(da, ga_b); }
    if (db && ss_b == 0 && n_b == 1) { gb_b = block_sum<T>(gb_b, red); if (threadIdx.x == 0) atomic_add(db, gb_b); }
}

// out[s,i] = scale * log p(x[s,i] | a, b), written
template <typename T, int KIND>
__global__ __launch_bounds__(256) void univariate_elem_kernel(int S, int64_t n, const T* __restrict__ x, const T* __restrict__ a, int64_t n_a,
                                                              int64_t ss_a, const T* __restrict__ b, int64_t n_b, int64_t ss_b, T scale,
                                                              T* __restrict__ out) {
    const bool per_sample = ss_a != 0 || ss_b != 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ia = n_a == 1 ? 0 : i, ib = n_b == 1 ? 0 : i;
        UniDist<T, KIND> d;
        if (!per_sample) d.set(a[ia], b[ib], false);
        for (int s = 0; s < S; ++s) {
            const int64_t e = (int64_t)s * n + i;
            if (per_sample) d.set(a[(int64_t)s * ss_a + ia], b[(int64_t)s * ss_b + ib], false);
            T lp, gx, pa, pb;
            d.eval(x[e], lp, gx, pa, pb);
            out[e] = scale * lp;
        }
    }
}

// out[s] += scale * sum_i log p(x[s,i] | a, b).  A workgroup takes (sample, chunk) pairs p = s * chunks + c off a one-dimensional grid --
// S never rides on a 65 535-limited axis, and pairs beyond the grid are looped over -- and walks its chunk's elements i = c * 256 + t,
// + chunks * 256, ...; one block_sum and ONE atomic per pair, so out[s] receives `chunks` atomics whatever S is (per_sample_plan of fused_plan.h).
template <typename T, int KIND>
__global__ __launch_bounds__(256) void univariate_ps_kernel(int S, int64_t n, int chunks, const T* __restrict__ x, const T* __restrict__ a,
                                                            int64_t n_a, int64_t ss_a, const T* __restrict__ b, int64_t n_b, int64_t ss_b,
                                                            T scale, T* __restrict__ out) {
    __shared__ T red[16];
    const bool fixed = n_a == 1 && n_b == 1 && ss_a == 0 && ss_b == 0;       // single-element parameters: set() once per workgroup
    const int64_t pairs = (int64_t)S * chunks;
    UniDist<T, KIND> d;
    if (fixed) d.set(a[0], b[0], false);
    for (int64_t p = blockIdx.x; p < pairs; p += gridDim.x) {       // (uniform over the workgroup: block_sum's barriers are safe)
        const int64_t s = p / chunks, c = p - s * chunks;
        const T* xs = x + s * n;
        const T *as = a + s * ss_a, *bs = b + s * ss_b;
        T acc = 0;
        for (int64_t i = c * 256 + threadIdx.x; i < n; i += (int64_t)chunks * 256) {
            if (!fixed) d.set(as[n_a == 1 ? 0 : i], bs[n_b == 1 ? 0 : i], false);
            T lp, gx, pa, pb;
            d.eval(xs[i], lp, gx, pa, pb);
            acc += lp;
        }
        acc = block_sum<T>(acc, red);
        if (threadIdx.x == 0) atomic_add(out + s, acc * scale);
    }
}

struct UniArgs {
    int S; int64_t n;
    const void *x, *a; int64_t n_a, ss_a;
    const void* b; int64_t n_b, ss_b;
    double scale;
    const void* cot; int64_t cs_s, cs_i;
    void *out, *dx, *da, *db;
};
enum { UNI_REDUCED = 0, UNI_ELEM = 1, UNI_PER_SAMPLE = 2 };       // which kernel: out one scalar (+ reverse mode), out (S, n), out (S)

template <typename T, int KIND>
void uni_launch_kind(const UniArgs& u, int mode, hipStream_t st) {
    const dim3 block(256);
    if (mode == UNI_ELEM)
        hipLaunchKernelGGL((univariate_elem_kernel<T, KIND>), dim3(grid_for(u.n)), block, 0, st, u.S, u.n, (const T*)u.x, (const T*)u.a, u.n_a,
                           u.ss_a, (const T*)u.b, u.n_b, u.ss_b, (T)u.scale, (T*)u.out);
    else if (mode == UNI_PER_SAMPLE) {
        const PerSamplePlan p = per_sample_plan(u.S, u.n);      // (fused_plan.h)
        hipLaunchKernelGGL((univariate_ps_kernel<T, KIND>), dim3(p.grid), block, 0, st, u.S, u.n, p.chunks, (const T*)u.x, (const T*)u.a, u.n_a,
                           u.ss_a, (const T*)u.b, u.n_b, u.ss_b, (T)u.scale, (T*)u.out);
    } else                                                          // (the cap of grid_for_reduce is for the closing atomics)
        hipLaunchKernelGGL((univariate_logpdf_kernel<T, KIND>), dim3(grid_for_reduce(u.n)), block, 0, st, u.S, u.n, (const T*)u.x,
                           (const T*)u.a, u.n_a, u.ss_a, (const T*)u.b, u.n_b, u.ss_b, (T)u.scale, (const T*)u.cot, u.cs_s, u.cs_i, (T*)u.out,
                           (T*)u.dx, (T*)u.da, (T*)u.db);
}

// argument checks shared by every entry point over these kernels; 0: launch, 1: nothing to do, < 0: the status to return
static inline int uni_check(mxf_handle h, const char* name, int dtype, const UniArgs& u) {
    if (!h) return -1;
    if (u.n <= 0 || u.S <= 0) return 1;
    if (dtype != MXF_F32 && dtype != MXF_F64) return mxf_bad_dtype(h, name, dtype);
    if (!u.x || !u.a || !u.b) MXF_FAIL(h, -2, "%s: null x or parameter", name);
    if ((u.n_a != 1 && u.n_a != u.n) || (u.n_b != 1 && u.n_b != u.n)) MXF_FAIL(h, -2, "%s: the parameters must have 1 or n elements", name);
    if ((u.ss_a != 0 && (u.ss_a != u.n || u.n_a != u.n)) || (u.ss_b != 0 && (u.ss_b != u.n || u.n_b != u.n)))
        MXF_FAIL(h, -2, "%s: a parameter's sample stride must be 0, or n with n elements per sample", name);
    return 0;
}

}  // namespace
