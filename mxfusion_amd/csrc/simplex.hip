// Log-densities that reduce along a class axis of length K (gfx950): Categorical (a log-softmax and a pick, or a dot product with a
// one-hot row) and Dirichlet (a sum of (alpha - 1) log x terms and a log-Beta normaliser), each with its fused reverse mode.
//   A group of W lanes owns one row (s, b): W = 4 for K <= 4, 16 for K <= 16, 64 otherwise, so a wavefront holds 64 / W rows and a
//   workgroup of 256 threads 256 / W.  Lanes stride over K with step W; every reduction over K is a butterfly of shuffles inside the group
//   (no LDS, no barrier).  Every lane of a wavefront reaches every shuffle: a group without a row, and a lane without an element, loads
//   and stores nothing and contributes the neutral element.
//   Reverse mode: a gradient whose operand is shared over the batch axis is summed with atomics into a DOUBLE accumulator
//   (shared_grad.h), as in mvn.hip.  Where a wanted gradient is shared
//   over the samples only, a group owns the batch entry b and loops over s itself: the sum over s is a plain += of elements that this
//   lane alone touches.
// All four calls are launch-bound at the size of a prior and bandwidth-bound at the size of a classification likelihood (the passes over
// a row after the first are served by the caches).
//
// Replaces: Categorical.log_pdf_impl (components/distributions/categorical.py:83-106: log_softmax, pick / broadcast_mul + sum),
// Dirichlet.log_pdf_impl (dirichlet.py:43-65: norm, broadcast_power, prod, gamma) and MXNet autograd through them.
#include "common.h"
#include "shared_grad.h"
#include "special.h"

namespace {

template <int W, typename V>
__device__ __forceinline__ V group_sum(V v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
    return v;
}

template <int W, typename V>
__device__ __forceinline__ V group_max(V v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, W));
    return v;
}

// What the launches of one call share.  x: K per row (the labels of the Categorical: 1 per row), batch stride dense, sample stride ss_x;
// p: the parameter, (S|1, B|1, K).  by_batch (reverse mode): a group owns b and loops over s.
template <typename T>
struct SimplexArgs {
    int S;
    int64_t B;
    int K;
    const T* x; int64_t ss_x;
    const T* p; int64_t ss_p, sb_p;
    int one_hot, normalize;
    T scale;
    int by_batch;
};

// The work of group `item`: the rows (s0 .. s0 + ns - 1, b); a group past the end has live = false and one trip.
struct SimplexItem {
    bool live;
    int64_t b, s0;
    int ns;
    template <typename T>
    __device__ __forceinline__ SimplexItem(const SimplexArgs<T>& a, int64_t item, int64_t items) {
        live = item < items;
        b = live ? (a.by_batch ? item : item % a.B) : 0;
        s0 = live && !a.by_batch ? item / a.B : 0;
        ns = a.by_batch ? a.S : 1;
    }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// Categorical.  The row's log-probabilities are lp_k = (logp_k - m) - log sum_j exp(logp_j - m) with m the row maximum (normalize), or
// logp_k itself (m = 0, log sum = 0: the subtractions are exact).  A row of all -inf has m = -inf and logp - m = NaN.
template <typename T, int W>
struct CatRow {
    const T* lp;
    const T* x;
    T m, lsum, rsum;
    int idx;        // the label, truncated toward zero and clipped to [0, K - 1] (the default mode of MXNet's pick); NaN gives 0

    __device__ __forceinline__ CatRow(const SimplexArgs<T>& a, int64_t s, int64_t b, bool live, int l) {
        lp = a.p + s * a.ss_p + b * a.sb_p;
        x = a.x + s * a.ss_x + b * (a.one_hot ? a.K : 1);
        m = 0; lsum = 0; rsum = 1;
        if (a.normalize) {
            T v = -(T)INFINITY;
            if (live) for (int k = l; k < a.K; k += W) v = fmax(v, lp[k]);
            m = group_max<W>(v);
            T e = 0;
            if (live) for (int k = l; k < a.K; k += W) e += exp(lp[k] - m);
            e = group_sum<W>(e);
            lsum = log(e);
            rsum = (T)1 / e;
        }
        idx = 0;
        if (!a.one_hot && live) {
            const T xv = x[0];
            idx = xv >= (T)(a.K - 1) ? a.K - 1 : (xv > (T)0 ? (int)xv : 0);
        }
    }
    __device__ __forceinline__ T at(int k) const { return (lp[k] - m) - lsum; }
    __device__ __forceinline__ T prob(int k) const { return exp(lp[k] - m) * rsum; }
};

// out[s,b] = scale * lp_idx, or (one_hot) scale * sum_k x_k lp_k
template <typename T, int W>
__global__ __launch_bounds__(256) void categorical_logpdf_kernel(SimplexArgs<T> a, T* __restrict__ out) {
    constexpr int G = 256 / W;
    const int l = threadIdx.x % W, g = threadIdx.x / W;
    const int64_t rows = (int64_t)a.S * a.B;
    for (int64_t base = (int64_t)blockIdx.x * G; base < rows; base += (int64_t)gridDim.x * G) {
        const SimplexItem it(a, base + g, rows);
        const CatRow<T, W> row(a, it.s0, it.b, it.live, l);
        T v = 0;
        if (a.one_hot) {
            if (it.live) for (int k = l; k < a.K; k += W) v += row.x[k] * row.at(k);
            v = group_sum<W>(v);
        } else if (it.live) {
            v = row.at(row.idx);
        }
        if (it.live && l == 0) out[base + g] = a.scale * v;
    }
}

// With w = scale * cot[s,b] and t the one-hot of the label (one_hot: x itself):
//   dlogp_k += w (t_k - p_k sum_j t_j)  (normalize; p = exp(lp))  or  w t_k,     dx_k += w lp_k  (one_hot only)
template <typename T, int W>
__global__ __launch_bounds__(256) void categorical_logpdf_bwd_kernel(SimplexArgs<T> a, const T* __restrict__ cot, T* dlp, T* dx, double* slp) {
    constexpr int G = 256 / W;
    const int l = threadIdx.x % W, g = threadIdx.x / W;
    const int64_t items = a.by_batch ? a.B : (int64_t)a.S * a.B;
    const bool p_atomic = shared_over(true, a.sb_p, a.S, a.B);          // (the sum over s alone is by_batch's loop)
    for (int64_t base = (int64_t)blockIdx.x * G; base < items; base += (int64_t)gridDim.x * G) {
        const SimplexItem it(a, base + g, items);
        for (int64_t s = it.s0; s < it.s0 + it.ns; ++s) {
            const CatRow<T, W> row(a, s, it.b, it.live, l);
            T tsum = 1;
            if (a.one_hot && a.normalize) {
                T v = 0;
                if (it.live) for (int k = l; k < a.K; k += W) v += row.x[k];
                tsum = group_sum<W>(v);
            }
            if (!it.live) continue;
            const T w = a.scale * cot[s * a.B + it.b];
            const int64_t gp = shared_row(a.ss_p, a.sb_p, s, it.b, a.B, a.K), gx = shared_row(a.ss_x, true, s, it.b, a.B, a.K);
            for (int k = l; k < a.K; k += W) {
                if (dlp) {
                    const T t = a.one_hot ? row.x[k] : (k == row.idx ? (T)1 : (T)0);
                    const T v = a.normalize ? w * (t - row.prob(k) * tsum) : w * t;
                    if (p_atomic) atomic_add(slp + gp + k, (double)v); else dlp[gp + k] += v;
                }
                if (dx) dx[gx + k] += w * row.at(k);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Dirichlet.  xt = x / sum_k |x_k| (normalize) or x.  The sum of alpha is double for either T: it feeds lgamma and digamma, whose
// differences against the per-class terms cancel (lgamma(200) = 857: one float32 ulp is 6e-5), as UniDist::set's do.
template <typename T, int W>
struct DirRow {
    const T* x;
    const T* al;
    double sumA;
    T n1;
    int bad;        // some x_k <= 0 or alpha_k <= 0 (or NaN): the row is NaN

    __device__ __forceinline__ DirRow(const SimplexArgs<T>& a, int64_t s, int64_t b, bool live, int l) {
        x = a.x + s * a.ss_x + b * a.K;
        al = a.p + s * a.ss_p + b * a.sb_p;
        double sa = 0;
        T n = 0;
        int bd = 0;
        if (live)
            for (int k = l; k < a.K; k += W) {
                const T xv = x[k], av = al[k];
                sa += (double)av;
                n += fabs(xv);
                bd |= !(xv > (T)0) || !(av > (T)0);
            }
        sumA = group_sum<W>(sa);
        n1 = a.normalize ? group_sum<W>(n) : (T)1;
        bad = group_sum<W>(bd);
    }
    __device__ __forceinline__ T logx(int k) const { return log(x[k] / n1); }
};

// a / b - c with the subtraction kept apart from the division's closing fma: where a / b and c are the same quotient (the Dirichlet's dx at
// K = 1, whose two terms are equal) the difference is exactly zero
__device__ __forceinline__ double quotient_minus(double a, double b, double c) {
#pragma clang fp contract(off)
    const double q = a / b;
    return q - c;
}

// out[s,b] = scale * (sum_k (alpha_k - 1) log xt_k + lgamma(sum alpha) - sum_k lgamma(alpha_k))
template <typename T, int W>
__global__ __launch_bounds__(256) void dirichlet_logpdf_kernel(SimplexArgs<T> a, T* __restrict__ out) {
    constexpr int G = 256 / W;
    const int l = threadIdx.x % W, g = threadIdx.x / W;
    const int64_t rows = (int64_t)a.S * a.B;
    for (int64_t base = (int64_t)blockIdx.x * G; base < rows; base += (int64_t)gridDim.x * G) {
        const SimplexItem it(a, base + g, rows);
        const DirRow<T, W> row(a, it.s0, it.b, it.live, l);
        T t = 0;
        double lg = 0;                                 // sum_k lgamma(alpha_k) - lgamma(sum alpha): the latter is the term of the slot k = K
        if (it.live && !row.bad)
            for (int k = l; k <= a.K; k += W) {
                if (k < a.K) t += (row.al[k] - (T)1) * row.logx(k);
                const double v = mxf_lgamma(k < a.K ? (double)row.al[k] : row.sumA);
                lg += k < a.K ? v : -v;
            }
        t = group_sum<W>(t);
        lg = group_sum<W>(lg);
        if (it.live && l == 0) out[base + g] = row.bad ? (T)NAN : (T)((double)a.scale * ((double)t - lg));
    }
}

// With w = scale * cot[s,b] (NaN for a failed row):
//   dalpha_k += w (log xt_k + psi(sum alpha) - psi(alpha_k)),    dx_j += w ((alpha_j - 1) / x_j - [normalize] sum_k (alpha_k - 1) / sum_k |x_k|)
template <typename T, int W>
__global__ __launch_bounds__(256) void dirichlet_logpdf_bwd_kernel(SimplexArgs<T> a, const T* __restrict__ cot, T* dx, T* dal, double* sal) {
    constexpr int G = 256 / W;
    const int l = threadIdx.x % W, g = threadIdx.x / W;
    const int64_t items = a.by_batch ? a.B : (int64_t)a.S * a.B;
    const bool p_atomic = shared_over(true, a.sb_p, a.S, a.B);          // (the sum over s alone is by_batch's loop)
    for (int64_t base = (int64_t)blockIdx.x * G; base < items; base += (int64_t)gridDim.x * G) {
        const SimplexItem it(a, base + g, items);
        for (int64_t s = it.s0; s < it.s0 + it.ns; ++s) {
            const DirRow<T, W> row(a, s, it.b, it.live, l);
            if (!it.live) continue;
            const T w = row.bad ? (T)NAN : a.scale * cot[s * a.B + it.b];
            const int64_t gp = shared_row(a.ss_p, a.sb_p, s, it.b, a.B, a.K), gx = shared_row(a.ss_x, true, s, it.b, a.B, a.K);
            const double pull = a.normalize ? (row.sumA - (double)a.K) / (double)row.n1 : 0.0;     // both terms of dx in double: they cancel (K = 1: exactly)
            double psiS = 0.0;
            for (int k = l - W; k < a.K; k += W) {         // the first trip (k < 0) is psi(sum alpha): one copy of the digamma code for both
                const double psi = dal ? mxf_digamma<double>(k < 0 ? row.sumA : (double)row.al[k]) : 0.0;
                if (k < 0) { psiS = psi; continue; }
                if (dal) {
                    const T v = w * (T)((double)row.logx(k) + psiS - psi);
                    if (p_atomic) atomic_add(sal + gp + k, (double)v); else dal[gp + k] += v;
                }
                if (dx) dx[gx + k] += w * (T)quotient_minus((double)row.al[k] - 1.0, (double)row.x[k], pull);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct SimplexCall {
    const char* name;
    int dtype, S; int64_t B; int K;
    const void* x; int64_t ss_x;
    const void* p; int64_t ss_p, sb_p;
    int one_hot, normalize;
    double scale;
    bool labels;        // x holds one element per row (the Categorical without one-hot encoding)
    bool bwd, dirichlet;
};

// out (forward), or cot and the gradient buffers of the parameter and of x (reverse: either may be null).  The parameter's gradient is
// summed in double (shared_grad.h) where it is shared over the batch axis.
template <typename T>
int launch(mxf_handle h, const SimplexCall& c, const SimplexPlan& p, void* out, const void* cot, void* dp, void* dx, hipStream_t st) {
    SharedSums sums;
    if (int rc = shared_sums_open<T>(h, c.name, {{dp, p.n_sum}}, st, &sums)) return rc;
    const SimplexArgs<T> a = {.S = c.S, .B = c.B, .K = c.K, .x = (const T*)c.x, .ss_x = c.ss_x, .p = (const T*)c.p, .ss_p = c.ss_p, .sb_p = c.sb_p,
                              .one_hot = c.one_hot, .normalize = c.normalize, .scale = (T)c.scale, .by_batch = p.by_batch ? 1 : 0};
    dispatch<4, 16, 64>(p.bucket, [&](auto w) {
        constexpr int W = decltype(w)::value;
        const dim3 grid(p.grid), block(256);
        if (!c.bwd && c.dirichlet) hipLaunchKernelGGL((dirichlet_logpdf_kernel<T, W>), grid, block, 0, st, a, (T*)out);
        else if (!c.bwd) hipLaunchKernelGGL((categorical_logpdf_kernel<T, W>), grid, block, 0, st, a, (T*)out);
        else if (c.dirichlet) hipLaunchKernelGGL((dirichlet_logpdf_bwd_kernel<T, W>), grid, block, 0, st, a, (const T*)cot, (T*)dx, (T*)dp, sums.acc[0]);
        else hipLaunchKernelGGL((categorical_logpdf_bwd_kernel<T, W>), grid, block, 0, st, a, (const T*)cot, (T*)dp, (T*)dx, sums.acc[0]);
        return 0;
    });
    shared_sums_close(sums, st);
    return 0;
}

int run(mxf_handle h, const SimplexCall& c, void* out, const void* cot, void* dp, void* dx, void* stream) {
    if (!h) return -1;
    const SimplexPlan p = simplex_plan({.dtype = c.dtype, .bwd = c.bwd, .dirichlet = c.dirichlet, .S = c.S, .B = c.B, .K = c.K, .ss_x = c.ss_x,
                                        .ss_p = c.ss_p, .sb_p = c.sb_p, .one_hot = c.one_hot != 0, .labels = c.labels, .has_x = c.x != nullptr,
                                        .has_p = c.p != nullptr, .has_out = out != nullptr, .has_cot = cot != nullptr, .has_dp = dp != nullptr,
                                        .has_dx = dx != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", c.name, p.refusal);
    if (p.empty) return 0;
    return mxf_typed(h, c.name, c.dtype, [&](auto t) { return launch<decltype(t)>(h, c, p, out, cot, dp, dx, (hipStream_t)stream); });
}

}  // namespace

extern "C" int mxf_categorical_logpdf(mxf_handle h, int dtype, int S, int64_t B, int K, const void* logp, int64_t strideS_lp,
                                      int64_t strideB_lp, const void* x, int64_t strideS_x, int one_hot, int normalize, double scale,
                                      void* out, void* stream) {
    const SimplexCall c = {.name = "mxf_categorical_logpdf", .dtype = dtype, .S = S, .B = B, .K = K, .x = x, .ss_x = strideS_x, .p = logp,
                           .ss_p = strideS_lp, .sb_p = strideB_lp, .one_hot = one_hot != 0, .normalize = normalize != 0, .scale = scale,
                           .labels = one_hot == 0};
    return run(h, c, out, nullptr, nullptr, nullptr, stream);
}

extern "C" int mxf_categorical_logpdf_bwd(mxf_handle h, int dtype, int S, int64_t B, int K, const void* logp, int64_t strideS_lp,
                                          int64_t strideB_lp, const void* x, int64_t strideS_x, int one_hot, int normalize, const void* cot,
                                          double scale, void* dlogp_acc, void* dx_acc, void* stream) {
    const SimplexCall c = {.name = "mxf_categorical_logpdf_bwd", .dtype = dtype, .S = S, .B = B, .K = K, .x = x, .ss_x = strideS_x, .p = logp,
                           .ss_p = strideS_lp, .sb_p = strideB_lp, .one_hot = one_hot != 0, .normalize = normalize != 0, .scale = scale,
                           .labels = one_hot == 0, .bwd = true};
    return run(h, c, nullptr, cot, dlogp_acc, dx_acc, stream);
}

extern "C" int mxf_dirichlet_logpdf(mxf_handle h, int dtype, int S, int64_t B, int K, const void* x, int64_t strideS_x, const void* alpha,
                                    int64_t strideS_a, int64_t strideB_a, int normalize, double scale, void* out, void* stream) {
    const SimplexCall c = {.name = "mxf_dirichlet_logpdf", .dtype = dtype, .S = S, .B = B, .K = K, .x = x, .ss_x = strideS_x, .p = alpha,
                           .ss_p = strideS_a, .sb_p = strideB_a, .one_hot = 1, .normalize = normalize != 0, .scale = scale, .dirichlet = true};
    return run(h, c, out, nullptr, nullptr, nullptr, stream);
}

extern "C" int mxf_dirichlet_logpdf_bwd(mxf_handle h, int dtype, int S, int64_t B, int K, const void* x, int64_t strideS_x, const void* alpha,
                                        int64_t strideS_a, int64_t strideB_a, int normalize, const void* cot, double scale, void* dx_acc,
                                        void* dalpha_acc, void* stream) {
    const SimplexCall c = {.name = "mxf_dirichlet_logpdf_bwd", .dtype = dtype, .S = S, .B = B, .K = K, .x = x, .ss_x = strideS_x, .p = alpha,
                           .ss_p = strideS_a, .sb_p = strideB_a, .one_hot = 1, .normalize = normalize != 0, .scale = scale, .bwd = true,
                           .dirichlet = true};
    return run(h, c, nullptr, cot, dalpha_acc, dx_acc, stream);
}
