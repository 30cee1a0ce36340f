// Log-densities of the univariate family (gfx950): Gamma, Gamma by mean and variance, Beta, Laplace, Uniform, Bernoulli.  Built like
// normal_logpdf_kernel (elementwise.hip): thread i owns element i for all S samples, per-element parameter gradients need no atomics,
// single-element parameters are block-reduced, one atomic per workgroup per scalar.  Launch-bound at the sizes of a prior.
//
// Replaces: Gamma / GammaMeanVariance.log_pdf_impl (components/distributions/gamma.py:45-59, :127-159), Beta.log_pdf_impl
// (beta.py:46-68), Laplace.log_pdf_impl (laplace.py:37-55), Uniform.log_pdf_impl (uniform.py:38-62), Bernoulli.log_pdf_impl
// (bernoulli.py:62-78) + the sum(mean_S(.)) of
// models/factor_graph.py:223, and MXNet autograd through them.
#include "common.h"
#include "special.h"

namespace {

// One (a, b) parameter pair: set() holds what does not depend on x, eval() gives log p(x) and its three partial derivatives.
// The x-free terms of Gamma and Beta are differences of lgamma values of a few hundred (lgamma(100) = 359: one float32 ulp is 3e-5), so
// set() forms them in double for either T -- once per element where the parameters have no sample axis.
template <typename T, int KIND>
struct UniDist {
    T a, b;         // GAMMA_MV: the (alpha, beta) that the mean and variance stand for
    T c;            // the terms of log p without x
    T ca, cb;       // d c / d a, d c / d b
    T inv;          // LAPLACE 1/scale, UNIFORM 1/(high - low), GAMMA_MV 1/variance

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

// out += scale * sum log p(x | a, b);  dx, da, db += w * (d log p / d .)  with  w = scale  or, given a cotangent, w = scale * cot[s,i].
// A parameter is a single element (n_p == 1), per element (n_p == n, sample stride 0: its gradient is summed over the samples) or per
// sample and element (sample stride n: its gradient is (S, n) like dx).
template <typename T, int KIND>
__global__ __launch_bounds__(256) void univariate_logpdf_kernel(int S, int64_t n, const T* __restrict__ x, const T* __restrict__ a, int64_t n_a,
                                                                int64_t ss_a, const T* __restrict__ b, int64_t n_b, int64_t ss_b, T scale,
                                                                const T* __restrict__ cot, T* __restrict__ out, T* __restrict__ dx,
                                                                T* __restrict__ da, T* __restrict__ db) {
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
                const T w = cot ? cot[e] * scale : scale;
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

struct UniArgs {
    int S; int64_t n;
    const void *x, *a; int64_t n_a, ss_a;
    const void* b; int64_t n_b, ss_b;
    double scale;
    const void* cot;
    void *out, *dx, *da, *db;
};

template <typename T, int KIND>
void launch_kind(const UniArgs& u, bool elem, hipStream_t st) {
    const dim3 grid(elem ? grid_for(u.n) : grid_for_reduce(u.n)), block(256);      // (the cap of grid_for_reduce is for the closing atomics)
    if (elem)
        hipLaunchKernelGGL((univariate_elem_kernel<T, KIND>), grid, block, 0, st, u.S, u.n, (const T*)u.x, (const T*)u.a, u.n_a, u.ss_a,
                           (const T*)u.b, u.n_b, u.ss_b, (T)u.scale, (T*)u.out);
    else
        hipLaunchKernelGGL((univariate_logpdf_kernel<T, KIND>), grid, block, 0, st, u.S, u.n, (const T*)u.x, (const T*)u.a, u.n_a, u.ss_a,
                           (const T*)u.b, u.n_b, u.ss_b, (T)u.scale, (const T*)u.cot, (T*)u.out, (T*)u.dx, (T*)u.da, (T*)u.db);
}

template <typename T>
void launch(int kind, const UniArgs& u, bool elem, hipStream_t st) {
    switch (kind) {
        case MXF_D_GAMMA: launch_kind<T, MXF_D_GAMMA>(u, elem, st); break;
        case MXF_D_GAMMA_MV: launch_kind<T, MXF_D_GAMMA_MV>(u, elem, st); break;
        case MXF_D_BETA: launch_kind<T, MXF_D_BETA>(u, elem, st); break;
        case MXF_D_LAPLACE: launch_kind<T, MXF_D_LAPLACE>(u, elem, st); break;
        case MXF_D_BERNOULLI: launch_kind<T, MXF_D_BERNOULLI>(u, elem, st); break;
        default: launch_kind<T, MXF_D_UNIFORM>(u, elem, st); break;
    }
}

// argument checks shared by the three entry points, then the launch
int run(mxf_handle h, const char* name, int kind, int dtype, const UniArgs& u, bool elem, void* stream) {
    if (!h) return -1;
    if (u.n <= 0 || u.S <= 0) return 0;
    if (kind < MXF_D_GAMMA || kind > MXF_D_BERNOULLI) MXF_FAIL(h, -2, "%s: unknown distribution kind %d", name, kind);
    if (dtype != MXF_F32 && dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, dtype);
    if (!u.x || !u.a || !u.b) MXF_FAIL(h, -2, "%s: null x or parameter", name);
    if ((u.n_a != 1 && u.n_a != u.n) || (u.n_b != 1 && u.n_b != u.n)) MXF_FAIL(h, -2, "%s: the parameters must have 1 or n elements", name);
    if ((u.ss_a != 0 && (u.ss_a != u.n || u.n_a != u.n)) || (u.ss_b != 0 && (u.ss_b != u.n || u.n_b != u.n)))
        MXF_FAIL(h, -2, "%s: a parameter's sample stride must be 0, or n with n elements per sample", name);
    if (dtype == MXF_F32) launch<float>(kind, u, elem, (hipStream_t)stream);
    else launch<double>(kind, u, elem, (hipStream_t)stream);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

extern "C" int mxf_univariate_logpdf(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                     const void* b, int64_t n_b, double scale, void* out_acc, void* dx_acc, void* da_acc, void* db_acc,
                                     void* stream) {
    const UniArgs u = {S, n, x, a, n_a, 0, b, n_b, 0, scale, nullptr, out_acc, dx_acc, da_acc, db_acc};
    return run(h, "mxf_univariate_logpdf", kind, dtype, u, false, stream);
}

extern "C" int mxf_univariate_logpdf_elem(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                          int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b, double scale, void* out,
                                          void* stream) {
    if (h && n > 0 && S > 0 && !out) MXF_FAIL(h, -2, "mxf_univariate_logpdf_elem: null out");
    const UniArgs u = {S, n, x, a, n_a, strideS_a, b, n_b, strideS_b, scale, nullptr, out, nullptr, nullptr, nullptr};
    return run(h, "mxf_univariate_logpdf_elem", kind, dtype, u, true, stream);
}

extern "C" int mxf_univariate_logpdf_bwd(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                         int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b, const void* cot, double scale,
                                         void* dx_acc, void* da_acc, void* db_acc, void* stream) {
    if (h && n > 0 && S > 0 && !cot) MXF_FAIL(h, -2, "mxf_univariate_logpdf_bwd: null cotangent");
    const UniArgs u = {S, n, x, a, n_a, strideS_a, b, n_b, strideS_b, scale, cot, nullptr, dx_acc, da_acc, db_acc};
    return run(h, "mxf_univariate_logpdf_bwd", kind, dtype, u, false, stream);
}
