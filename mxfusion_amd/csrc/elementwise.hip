// Elementwise / reduction kernels of the Monte-Carlo ELBO loop (gfx950): softplus transform,
// Normal log-pdf with fused reverse mode and wavefront-shuffle reductions, reparameterised sampling
// and its reverse mode, MXNet-Adam.  All HBM-bound streaming kernels: 16-byte loads where the layout
// allows, grid-stride, one atomic per block for the scalar sums.
//
// Replaces: PositiveTransformation (components/variables/var_trans.py:63-91), Normal.log_pdf_impl /
// draw_samples_impl (components/distributions/normal.py:52-92), NormalMeanPrecision.draw_samples_impl (normal.py:286-306) + the sum(mean_S(.)) of
// models/factor_graph.py:223, and gluon.Trainer.step(adam) of inference/batch_loop.py:46-60.  The per-sample Normal (mxf_normal_logpdf_ps*)
// is the Normal kind of the kernels in unidist.h.
#include "common.h"
#include "unidist.h"

namespace {

constexpr double LOG2PI = 1.8378770664093453;

template <typename T> __device__ __forceinline__ T softplus_f(T x) {
    // log(1+exp(x)) = max(x,0) + log1p(exp(-|x|))  (overflow-safe form of MXNet's softrelu)
    return fmax(x, (T)0) + log1p(exp(-fabs(x)));
}
template <typename T> __device__ __forceinline__ T sigmoid_f(T x) {
    return x >= (T)0 ? (T)1 / ((T)1 + exp(-x)) : exp(x) / ((T)1 + exp(x));
}

template <typename T>
__global__ void softplus_fwd_kernel(int64_t n, const T* __restrict__ x, T* __restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = softplus_f<T>(x[i]);
}
template <typename T>
__global__ void softplus_bwd_kernel(int64_t n, const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dx[i] += dy[i] * sigmoid_f<T>(x[i]);
}

template <typename T>
__global__ void reparam_kernel(int S, int64_t n, const T* __restrict__ mean, const T* __restrict__ var, const T* __restrict__ eps,
                               T* __restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T m = mean[i], sd = sqrt(var[i]);
        for (int s = 0; s < S; ++s) x[(int64_t)s * n + i] = fma(eps[(int64_t)s * n + i], sd, m);
    }
}

template <typename T>
__global__ void reparam_bwd_kernel(int S, int64_t n, const T* __restrict__ var, const T* __restrict__ eps, const T* __restrict__ dx,
                                   T* __restrict__ dmean, T* __restrict__ dvar) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        T gm = 0, gv = 0;
        for (int s = 0; s < S; ++s) {
            const T g = dx[(int64_t)s * n + i];
            gm += g;
            gv = fma(g, eps[(int64_t)s * n + i], gv);
        }
        if (dmean) dmean[i] += gm;
        if (dvar) dvar[i] += gv * (T)0.5 / sqrt(var[i]);
    }
}

// the draw by mean and precision: x = mean + eps / sqrt(precision)
template <typename T>
__global__ void reparam_prec_kernel(int S, int64_t n, const T* __restrict__ mean, const T* __restrict__ prec, const T* __restrict__ eps,
                                    T* __restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T m = mean[i], isd = (T)1 / sqrt(prec[i]);
        for (int s = 0; s < S; ++s) x[(int64_t)s * n + i] = fma(eps[(int64_t)s * n + i], isd, m);
    }
}

// d x / d precision = -eps precision^(-3/2) / 2
template <typename T>
__global__ void reparam_prec_bwd_kernel(int S, int64_t n, const T* __restrict__ prec, const T* __restrict__ eps, const T* __restrict__ dx,
                                        T* __restrict__ dmean, T* __restrict__ dprec) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        T gm = 0, gp = 0;
        for (int s = 0; s < S; ++s) {
            const T g = dx[(int64_t)s * n + i];
            gm += g;
            gp = fma(g, eps[(int64_t)s * n + i], gp);
        }
        if (dmean) dmean[i] += gm;
        if (dprec) { const T p = prec[i]; dprec[i] += gp * (T)-0.5 / (p * sqrt(p)); }
    }
}

// out += scale * sum logN(x|mean,var); dx += scale * dlogN/dx ...; thread i owns element i for all S samples,
// so dmean/dvar need no atomics when they are per-element; broadcast (single-element) mean/var are block-reduced.
template <typename T>
__global__ __launch_bounds__(256) void normal_logpdf_kernel(int S, int64_t n, const T* __restrict__ x, const T* __restrict__ mean,
                                                            int64_t n_mean, const T* __restrict__ var, int64_t n_var, T scale,
                                                            T* __restrict__ out, T* __restrict__ dx, T* __restrict__ dmean,
                                                            T* __restrict__ dvar) {
    __shared__ T red[16];
    T acc = 0, gm_b = 0, gv_b = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T m = mean[n_mean == 1 ? 0 : i], v = var[n_var == 1 ? 0 : i];
        const T iv = (T)1 / v;
        const T c = (T)(-0.5 * LOG2PI) - (T)0.5 * log(v);
        T gm = 0, gv = 0;
        for (int s = 0; s < S; ++s) {
            const T d = x[(int64_t)s * n + i] - m;
            acc += c - (T)0.5 * d * d * iv;
            const T g = -d * iv * scale;                 // d/dx
            if (dx) dx[(int64_t)s * n + i] += g;
            gm -= g;                                      // d/dmean = -d/dx
            gv += scale * (T)0.5 * (d * d * iv * iv - iv);   // d/dvar
        }
        if (dmean) { if (n_mean == 1) gm_b += gm; else dmean[i] += gm; }
        if (dvar) { if (n_var == 1) gv_b += gv; else dvar[i] += gv; }
    }
    acc = block_sum<T>(acc, red);
    if (threadIdx.x == 0 && out) atomic_add(out, acc * scale);
    if (dmean && n_mean == 1) { gm_b = block_sum<T>(gm_b, red); if (threadIdx.x == 0) atomic_add(dmean, gm_b); }
    if (dvar && n_var == 1) { gv_b = block_sum<T>(gv_b, red); if (threadIdx.x == 0) atomic_add(dvar, gv_b); }
}

template <typename T>
__global__ void adam_kernel(int64_t n, T* __restrict__ w, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, T lr_t, T b1,
                            T b2, T eps, T rescale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T gi = g[i] * rescale;
        const T mi = b1 * m[i] + ((T)1 - b1) * gi;
        const T vi = b2 * v[i] + ((T)1 - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        w[i] -= lr_t * mi / (sqrt(vi) + eps);
    }
}

// out[s][n] = sum_m A[s][m][n] * B[s][m][n]   (F.sum(A*B, axis=-2): gp_regression.py:181, svgp_regression.py:166-169)
template <typename T>
__global__ void coldot_kernel(int64_t M, int64_t N, const T* __restrict__ A, int64_t lda, int64_t sA, const T* __restrict__ B, int64_t ldb,
                              int64_t sB, T* __restrict__ out) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const T* a = A + (int64_t)blockIdx.y * sA;
    const T* b = B + (int64_t)blockIdx.y * sB;
    T acc = 0;
    for (int64_t m = 0; m < M; ++m) acc = fma(a[m * lda + n], b[m * ldb + n], acc);
    out[(int64_t)blockIdx.y * N + n] = acc;
}

// few columns (the rollout's one test point per trajectory: N = 64, M = 1000): a thread per column leaves the chip idle and walks the rows
// serially (224 us at that shape); here a workgroup owns 16 columns and spreads the rows over 16 lanes each, combined through LDS
template <typename T>
__global__ __launch_bounds__(256) void coldot_small_kernel(int64_t M, int64_t N, const T* __restrict__ A, int64_t lda, int64_t sA,
                                                           const T* __restrict__ B, int64_t ldb, int64_t sB, T* __restrict__ out) {
    __shared__ T part[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int64_t n = (int64_t)blockIdx.x * 16 + cx;
    const T* a = A + (int64_t)blockIdx.y * sA;
    const T* b = B + (int64_t)blockIdx.y * sB;
    T acc = 0;
    if (n < N)
        for (int64_t m = ry; m < M; m += 16) acc = fma(a[m * lda + n], b[m * ldb + n], acc);
    part[ry][cx] = acc;
    __syncthreads();
    if (ry == 0 && n < N) {
        T t = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += part[r][cx];
        out[(int64_t)blockIdx.y * N + n] = t;
    }
}

// make_diagonal (util/customop.py:22-81): out[b][i][j] = (i == j) ? a[b][i] : 0; its reverse mode extracts the diagonal of the cotangent
template <typename T>
__global__ void make_diagonal_kernel(int64_t total, int64_t n, const T* __restrict__ a, T* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = e % n, i = (e / n) % n, b = e / (n * n);
        out[e] = (i == j) ? a[b * n + i] : (T)0;
    }
}
template <typename T>
__global__ void diag_of_kernel(int64_t total, int64_t n, const T* __restrict__ g, T* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e % n, b = e / n;
        out[e] = g[(b * n + i) * n + i];
    }
}


}  // namespace

extern "C" int mxf_softplus_fwd(mxf_handle h, int dtype, int64_t n, const void* x, void* y, void* stream) {
    if (!h) return -1;
    if (n <= 0) return 0;
    return mxf_typed(h, "mxf_softplus_fwd", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((softplus_fwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (const T*)x, (T*)y);
    });
}

extern "C" int mxf_softplus_bwd(mxf_handle h, int dtype, int64_t n, const void* x, const void* dy, void* dx_acc, void* stream) {
    if (!h) return -1;
    if (n <= 0) return 0;
    return mxf_typed(h, "mxf_softplus_bwd", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((softplus_bwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (const T*)x, (const T*)dy, (T*)dx_acc);
    });
}

extern "C" int mxf_normal_reparam(mxf_handle h, int dtype, int S, int64_t n, const void* mean, const void* var, const void* eps,
                                  void* x, void* stream) {
    if (!h) return -1;
    if (n <= 0 || S <= 0) return 0;
    return mxf_typed(h, "mxf_normal_reparam", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((reparam_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, S, n, (const T*)mean, (const T*)var, (const T*)eps, (T*)x);
    });
}

extern "C" int mxf_normal_reparam_bwd(mxf_handle h, int dtype, int S, int64_t n, const void* var, const void* eps, const void* dx,
                                      void* dmean_acc, void* dvar_acc, void* stream) {
    if (!h) return -1;
    if (n <= 0 || S <= 0) return 0;
    return mxf_typed(h, "mxf_normal_reparam_bwd", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((reparam_bwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, S, n, (const T*)var, (const T*)eps, (const T*)dx, (T*)dmean_acc, (T*)dvar_acc);
    });
}

extern "C" int mxf_normal_reparam_prec(mxf_handle h, int dtype, int S, int64_t n, const void* mean, const void* precision, const void* eps,
                                       void* x, void* stream) {
    if (!h) return -1;
    if (n <= 0 || S <= 0) return 0;
    if (!mean || !precision || !eps || !x) MXF_FAIL(h, -2, "mxf_normal_reparam_prec: null argument");
    return mxf_typed(h, "mxf_normal_reparam_prec", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((reparam_prec_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, S, n, (const T*)mean, (const T*)precision, (const T*)eps, (T*)x);
    });
}

extern "C" int mxf_normal_reparam_prec_bwd(mxf_handle h, int dtype, int S, int64_t n, const void* precision, const void* eps, const void* dx,
                                           void* dmean_acc, void* dprecision_acc, void* stream) {
    if (!h) return -1;
    if (n <= 0 || S <= 0) return 0;
    if (!precision || !eps || !dx) MXF_FAIL(h, -2, "mxf_normal_reparam_prec_bwd: null argument");
    return mxf_typed(h, "mxf_normal_reparam_prec_bwd", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((reparam_prec_bwd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, S, n, (const T*)precision, (const T*)eps,
                           (const T*)dx, (T*)dmean_acc, (T*)dprecision_acc);
    });
}

extern "C" int mxf_normal_logpdf(mxf_handle h, int dtype, int S, int64_t n, const void* x, const void* mean, int64_t n_mean,
                                 const void* var, int64_t n_var, double scale, void* out_acc, void* dx_acc, void* dmean_acc,
                                 void* dvar_acc, void* stream) {
    if (!h) return -1;
    if (n <= 0 || S <= 0) return 0;
    if ((n_mean != 1 && n_mean != n) || (n_var != 1 && n_var != n)) MXF_FAIL(h, -2, "mxf_normal_logpdf: mean/var must have 1 or n elements");
    return mxf_typed(h, "mxf_normal_logpdf", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((normal_logpdf_kernel<T>), dim3(grid_for_reduce(n)), dim3(256), 0, (hipStream_t)stream, S, n, (const T*)x, (const T*)mean,
                           n_mean, (const T*)var, n_var, (T)scale, (T*)out_acc, (T*)dx_acc, (T*)dmean_acc, (T*)dvar_acc);
    });
}

// the per-sample sums and their reverse mode: univariate_ps_kernel / univariate_logpdf_kernel (unidist.h) with the Normal's evaluation struct
static int normal_ps_run(mxf_handle h, const char* name, int dtype, const UniArgs& u, int mode, void* stream) {
    if (const int rc = uni_check(h, name, dtype, u)) return rc < 0 ? rc : 0;
    return mxf_typed(h, name, dtype, [&](auto t) { uni_launch_kind<decltype(t), MXF_D_NORMAL_>(u, mode, (hipStream_t)stream); });
}

extern "C" int mxf_normal_logpdf_ps(mxf_handle h, int dtype, int S, int64_t n, const void* x, const void* mean, int64_t n_mean,
                                    int64_t strideS_mean, const void* var, int64_t n_var, int64_t strideS_var, double scale, void* out_acc,
                                    void* stream) {
    if (h && n > 0 && S > 0 && !out_acc) MXF_FAIL(h, -2, "mxf_normal_logpdf_ps: null out");
    const UniArgs u = {.S = S, .n = n, .x = x, .a = mean, .n_a = n_mean, .ss_a = strideS_mean, .b = var, .n_b = n_var, .ss_b = strideS_var,
                       .scale = scale, .out = out_acc};
    return normal_ps_run(h, "mxf_normal_logpdf_ps", dtype, u, UNI_PER_SAMPLE, stream);
}

extern "C" int mxf_normal_logpdf_ps_bwd(mxf_handle h, int dtype, int S, int64_t n, const void* x, const void* mean, int64_t n_mean,
                                        int64_t strideS_mean, const void* var, int64_t n_var, int64_t strideS_var, const void* w, double scale,
                                        void* dx_acc, void* dmean_acc, void* dvar_acc, void* stream) {
    if (h && n > 0 && S > 0 && !w) MXF_FAIL(h, -2, "mxf_normal_logpdf_ps_bwd: null weights");
    const UniArgs u = {.S = S, .n = n, .x = x, .a = mean, .n_a = n_mean, .ss_a = strideS_mean, .b = var, .n_b = n_var, .ss_b = strideS_var,
                       .scale = scale, .cot = w, .cs_s = 1, .cs_i = 0, .dx = dx_acc, .da = dmean_acc, .db = dvar_acc};
    return normal_ps_run(h, "mxf_normal_logpdf_ps_bwd", dtype, u, UNI_REDUCED, stream);
}

extern "C" int mxf_adam_step(mxf_handle h, int dtype, int64_t n, void* w, const void* g, void* m, void* v, double lr, double beta1,
                             double beta2, double epsilon, double rescale_grad, int t, void* stream) {
    if (!h) return -1;
    if (n <= 0) return 0;
    if (t < 1) MXF_FAIL(h, -2, "mxf_adam_step: t must be >= 1");
    const double lr_t = lr * sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t));
    return mxf_typed(h, "mxf_adam_step", dtype, [&](auto e) {
        using T = decltype(e);
        hipLaunchKernelGGL((adam_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (T*)w, (const T*)g, (T*)m, (T*)v, (T)lr_t, (T)beta1,
                           (T)beta2, (T)epsilon, (T)rescale_grad);
    });
}

// out[0] = sum_i g[i] if all g[i] agree to 1e-6 relative, NaN otherwise (n small: the upstream gradient of the per-sample log-pdfs)
template <typename T>
__global__ __launch_bounds__(64) void uniform_sum_kernel(int64_t n, const T* __restrict__ g, T* __restrict__ out) {
    T s = 0, lo = g[0], hi = g[0];
    for (int64_t i = threadIdx.x; i < n; i += 64) { const T v = g[i]; s += v; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64); lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi; }
    if (threadIdx.x == 0) {
        const T mean = s / (T)n, a = mean < 0 ? -mean : mean;
        out[0] = (hi - lo <= (T)1e-6 * a) ? s : (T)NAN;
    }
}

extern "C" int mxf_uniform_sum(mxf_handle h, int dtype, int64_t n, const void* g, void* out, void* stream) {
    if (!h) return -1;
    if (n <= 0 || !g || !out) MXF_FAIL(h, -2, "mxf_uniform_sum: bad argument");
    return mxf_typed(h, "mxf_uniform_sum", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((uniform_sum_kernel<T>), dim3(1), dim3(64), 0, (hipStream_t)stream, n, (const T*)g, (T*)out);
    });
}

// MXNet SGD (optimizer 'sgd' of gluon.Trainer): g = rescale * grad + wd * w; momentum == 0: w -= lr g; else mom = momentum mom - lr g, w += mom
template <typename T>
__global__ void sgd_kernel(int64_t n, T* __restrict__ w, const T* __restrict__ g, T* __restrict__ mom, T lr, T momentum, T wd, T rescale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T gi = g[i] * rescale + wd * w[i];
        if (mom) { const T mi = momentum * mom[i] - lr * gi; mom[i] = mi; w[i] += mi; }
        else w[i] -= lr * gi;
    }
}

extern "C" int mxf_sgd_step(mxf_handle h, int dtype, int64_t n, void* w, const void* g, void* mom, double lr, double momentum, double wd,
                            double rescale_grad, void* stream) {
    if (!h) return -1;
    if (n <= 0) return 0;
    return mxf_typed(h, "mxf_sgd_step", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((sgd_kernel<T>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (T*)w, (const T*)g, (T*)mom, (T)lr, (T)momentum, (T)wd, (T)rescale_grad);
    });
}

// The other optimisers gluon.Trainer is commonly driven with by name (batch_loop.py:46-49 hands `optimizer` to the Trainer): MXNet's
// update rules as documented for its 1.x python optimisers (API knowledge -- there is no reference-held vector for them: parity unpinned).
//   g = rescale * grad (+ wd * w where the rule folds weight decay into the gradient)
//   RMSPROP (non-centred): n = (1 - gamma1) g^2 + gamma1 n;  w -= lr g / sqrt(n + eps)                      [s1 = n;  p1 = gamma1]
//   ADAGRAD: h += g^2;  w -= lr (g / sqrt(h + eps) + wd w)                                                   [s1 = h]
//   ADADELTA: a = rho a + (1 - rho) g^2;  d = sqrt(b + eps) / sqrt(a + eps) g;  b = rho b + (1 - rho) d^2;  w -= d + wd w   [s1 = a, s2 = b; p1 = rho]
//   NAG: m = momentum m + g;  w -= lr (g + momentum m)                                                       [s1 = m;  p1 = momentum]
template <typename T, int KIND>
__global__ void opt_kernel(int64_t n, T* __restrict__ w, const T* __restrict__ g, T* __restrict__ s1, T* __restrict__ s2, T lr, T p1, T eps, T wd,
                           T rescale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T wi = w[i];
        if (KIND == MXF_OPT_RMSPROP) {
            const T gi = g[i] * rescale + wd * wi;
            const T ni = ((T)1 - p1) * gi * gi + p1 * s1[i];
            s1[i] = ni;
            w[i] = wi - lr * gi / sqrt(ni + eps);
        } else if (KIND == MXF_OPT_ADAGRAD) {
            const T gi = g[i] * rescale;
            const T hi = s1[i] + gi * gi;
            s1[i] = hi;
            w[i] = wi - lr * (gi / sqrt(hi + eps) + wd * wi);
        } else if (KIND == MXF_OPT_ADADELTA) {
            const T gi = g[i] * rescale;
            const T ai = p1 * s1[i] + ((T)1 - p1) * gi * gi;
            const T di = sqrt(s2[i] + eps) / sqrt(ai + eps) * gi;
            s1[i] = ai;
            s2[i] = p1 * s2[i] + ((T)1 - p1) * di * di;
            w[i] = wi - (di + wd * wi);
        } else {
            const T gi = g[i] * rescale + wd * wi;
            const T mi = p1 * s1[i] + gi;
            s1[i] = mi;
            w[i] = wi - lr * (gi + p1 * mi);
        }
    }
}

extern "C" int mxf_opt_step(mxf_handle h, int kind, int dtype, int64_t n, void* w, const void* g, void* s1, void* s2, double lr, double p1, double epsilon,
                            double wd, double rescale_grad, void* stream) {
    if (!h) return -1;
    if (n <= 0) return 0;
    if (!w || !g || !s1 || (kind == MXF_OPT_ADADELTA && !s2)) MXF_FAIL(h, -2, "mxf_opt_step: null argument");
    const int rc = dispatch<MXF_OPT_RMSPROP, MXF_OPT_ADAGRAD, MXF_OPT_ADADELTA, MXF_OPT_NAG>(kind, [&](auto k) {
        return mxf_typed(h, "mxf_opt_step", dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((opt_kernel<T, decltype(k)::value>), dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, (T*)w, (const T*)g, (T*)s1,
                               (T*)s2, (T)lr, (T)p1, (T)epsilon, (T)wd, (T)rescale_grad);
        });
    });
    if (rc == NO_CASE) MXF_FAIL(h, -2, "mxf_opt_step: unknown optimiser kind %d", kind);
    return rc;
}

extern "C" int mxf_coldot(mxf_handle h, int dtype, int S, int64_t M, int64_t N, const void* A, int64_t lda, int64_t strideS_A,
                          const void* B, int64_t ldb, int64_t strideS_B, void* out, void* stream) {
    if (!h) return -1;
    if (S <= 0 || N <= 0) return 0;
    const ColdotPlan p = coldot_plan(S, M, N);      // (pointwise_plan.h)
    return mxf_typed(h, "mxf_coldot", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((p.small ? coldot_small_kernel<T> : coldot_kernel<T>), dim3(p.grid[0], p.grid[1]), dim3(256), 0, (hipStream_t)stream, M, N,
                           (const T*)A, lda, strideS_A, (const T*)B, ldb, strideS_B, (T*)out);
    });
}

extern "C" int mxf_make_diagonal(mxf_handle h, int dtype, int64_t batch, int64_t n, const void* a, void* out, void* stream) {
    if (!h) return -1;
    if (batch <= 0 || n <= 0) return 0;
    const int64_t total = batch * n * n;
    return mxf_typed(h, "mxf_make_diagonal", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((make_diagonal_kernel<T>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, total, n, (const T*)a, (T*)out);
    });
}

extern "C" int mxf_diag_of(mxf_handle h, int dtype, int64_t batch, int64_t n, const void* g, void* out, void* stream) {
    if (!h) return -1;
    if (batch <= 0 || n <= 0) return 0;
    const int64_t total = batch * n;
    return mxf_typed(h, "mxf_diag_of", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((diag_of_kernel<T>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, total, n, (const T*)g, (T*)out);
    });
}
