// Nearest-neighbour (Vecchia) GP regression (gfx950): every row of the data set conditioned on at most k <= 32 other rows.  With c the
// neighbours of a row, A = K(X_c, X_c) + noise I, kappa = K(X_c, x), a = k(x, x) + noise:
//   b = A^-1 kappa,  alpha = A^-1 Y_c,  s = a - kappa^T b,  r = y - kappa^T alpha,  l = -P/2 log 2 pi - P/2 log s - |r|^2 / (2 s)
//   mxf_vecchia_cond        kappa^T alpha and k(x*, x*) - kappa^T b for test rows: the predictor
//   mxf_vecchia_logpdf      the l_i and their sum
//   mxf_vecchia_logpdf_bwd  the gradient of g sum_i l_i in lengthscale, variance, noise and Y; the factor is recomputed
// No reference counterpart.  The covariance of a pair is kmv.h's, the function mxf_gram evaluates, on the scaled difference of the pair.
//
// A group of 32 lanes owns a row of the data set: lane t holds neighbour t (its index, its coordinates in registers) and row t of the tile.
// The tiles are smallmat.h's, double for either dtype: l (A, then its Cholesky factor) and y (the right-hand sides: Y_c in columns
// 0..P-1, kappa in column P; a lane per column in the substitutions).  VECCHIA_ROWS groups share a workgroup, and a workgroup takes further
// rows in a loop.  smallmat_cholesky holds a barrier per column, so every group runs every step with n = k: an empty slot (nbr = -1, at
// any place in the row), a row with fewer than k neighbours and the dead rows of the last trip run on a tile padded with a unit diagonal,
// zero off-diagonal and zero right-hand side, which contributes exactly nothing; stores are guarded, control flow is not.  Coordinates of
// the other neighbours arrive by shuffles within the group, so nothing but the two tiles is in LDS.
//
// With z = L^-1 [Y_c | kappa] (forward substitution): s = a - |z_kappa|^2, r = y - z_Y^T z_kappa; the forward calls stop there.  The
// reverse mode goes on to alpha, b = L^-T z and, with g_s = -P/(2s) + |r|^2/(2s^2), u = alpha r, w = g_s b - u / s:
//   G_a = g_s,  G_kappa = -2 g_s b + u / s,  G_A = b w^T (contracted with the symmetric dA),  dnoise = G_a + b^T w,
//   dl/dy = -r / s,  dl/dY_c = b r^T / s,
// and lengthscale and variance by cov_slope over the (k + 1)^2 pairs of the row, as kmv_bwd_kernel does per pair.
//
// Sums: the value and the parameter gradients are summed per lane and per workgroup in double, then one atomic per workgroup into zeroed
// double scratch that a close kernel narrows once; dY is scattered with atomics into the zeroed buffer.  Last bits can therefore differ
// between calls.  A pivot that is not positive turns that row's factor, term and gradients into NaN (smallmat's rule); nothing traps.
// Precondition (the caller's, stated in mxf_gp.h): nbr entries are -1 or in [0, N) and, for the log-pdf of row i, < i.  An entry outside
// [0, N) is read as -1, so no load leaves X or Y.
#include "common.h"
#include "fused_plan.h"      // VECCHIA_*; vecchia_plan
#include "kmv.h"
#include "smallmat.h"

namespace {

constexpr int VECCHIA_THREADS = 32 * VECCHIA_ROWS;
static_assert(VECCHIA_THREADS % 64 == 0, "whole wavefronts");

struct VecchiaTiles { double l[MVN_MAX * MVN_LD]; double y[MVN_MAX * MVN_LD]; };      // y: up to P + 1 = MVN_LD columns

template <typename T>
struct VecchiaOps {
    int64_t rows, N; int Q, P, k, ard;
    const T* Xt;            // the rows' own points: X itself for the log-pdf
    const T *X, *Y; const int32_t* nbr;
    const T *ls, *var, *noise;
};

template <int QP> struct VecchiaSums { double dl[QP]; double dv, dn, value; };

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}

// scaled squared distance of two points held in registers
template <typename T, int QP>
__device__ __forceinline__ T vecchia_red(const T* a, const T* b, const T* m) {
    T red = 0;
#pragma unroll
    for (int q = 0; q < QP; ++q) { const T d = (a[q] - b[q]) * m[q]; red = fma(d, d, red); }
    return red;
}

// One row of the data set in one group of 32 lanes.  CALL: VECCHIA_COND / VECCHIA_LOGPDF / VECCHIA_BWD.  Every lane of the workgroup runs
// every statement that holds a barrier or a shuffle.
template <typename T, int QP, int KIND, int CALL>
__device__ __forceinline__ void vecchia_row(const VecchiaOps<T>& o, VecchiaTiles& tl, int64_t row, int lane, const T* m, T variance, double noise,
                                            double gscale, T* mean_out, T* var_out, T* terms_out, T* dY, VecchiaSums<QP>& sums) {
    const int k = o.k, P = o.P;
    const bool live = row < o.rows, mine = lane < k;
    double* l = tl.l;
    double* y = tl.y;
    // this lane's neighbour and the row's own point; an empty slot holds zeros
    int64_t c = -1;
    if (live && mine) { c = o.nbr[row * k + lane]; if (c >= o.N) c = -1; }
    const bool valid = c >= 0;
    T xc[QP], xi[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        xc[q] = (valid && q < o.Q) ? o.X[c * o.Q + q] : (T)0;
        xi[q] = (live && q < o.Q) ? o.Xt[row * o.Q + q] : (T)0;
    }
    // row `lane` of A's lower triangle, and of the right-hand sides
    for (int tp = 0; tp < k; ++tp) {
        T z[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q) z[q] = __shfl(xc[q], tp, 32);
        const int other = __shfl((int)valid, tp, 32);          // (every lane takes part: not under the && of the next line)
        const bool both = valid && other != 0;
        const T kv = cov_from<T, KIND>(vecchia_red<T, QP>(xc, z, m), variance);
        if (mine && tp <= lane) l[lane * MVN_LD + tp] = both ? (double)kv + (tp == lane ? noise : 0.0) : (tp == lane ? 1.0 : 0.0);
    }
    const T kap = cov_from<T, KIND>(vecchia_red<T, QP>(xc, xi, m), variance);
    if (mine) {
        for (int p = 0; p < P; ++p) y[lane * MVN_LD + p] = valid ? (double)o.Y[c * P + p] : 0.0;
        y[lane * MVN_LD + P] = valid ? (double)kap : 0.0;
    }
    __syncthreads();
    int bad;
    smallmat_cholesky<32>(l, k, lane, mine, bad);
    // z = L^-1 [Y_c | kappa]: a lane per column
    for (int col = lane; col <= P; col += 32) {
        for (int i = 0; i < k; ++i) {
            double acc = y[i * MVN_LD + col];
            for (int j = 0; j < i; ++j) acc -= l[i * MVN_LD + j] * y[j * MVN_LD + col];
            y[i * MVN_LD + col] = acc / l[i * MVN_LD + i];
        }
    }
    __syncthreads();
    // s and r: every lane forms s; lane p < P forms r_p
    double q2 = 0.0, dot = 0.0;
    for (int i = 0; i < k; ++i) {
        const double zk = y[i * MVN_LD + P];
        q2 += zk * zk;
        if (lane < P) dot += zk * y[i * MVN_LD + lane];
    }
    const double a = CALL == VECCHIA_COND ? (double)variance : (double)cov_from<T, KIND>((T)0, variance) + noise;
    const double s = a - q2;
    if (CALL == VECCHIA_COND) {
        if (live && lane < P) mean_out[row * P + lane] = (T)dot;
        if (live && lane == 0) var_out[row] = (T)s;
        __syncthreads();                                     // the tiles are loaded again on the next trip
        return;
    }
    const double r = (live && lane < P) ? (double)o.Y[row * P + lane] - dot : 0.0;
    const double rr = group_sum(r * r);
    if (CALL == VECCHIA_LOGPDF) {
        const double term = -0.5 * P * 1.8378770664093454836 /* log 2 pi */ - 0.5 * P * log(s) - rr / (2.0 * s);
        if (live && lane == 0) {
            if (terms_out) terms_out[row] = (T)term;
            sums.value += term;
        }
        __syncthreads();
        return;
    }
    // ---- the reverse mode: alpha, b = L^-T z, a lane per column
    for (int col = lane; col <= P; col += 32) {
        for (int i = k - 1; i >= 0; --i) {
            double acc = y[i * MVN_LD + col];
            for (int j = i + 1; j < k; ++j) acc -= l[j * MVN_LD + i] * y[j * MVN_LD + col];
            y[i * MVN_LD + col] = acc / l[i * MVN_LD + i];
        }
    }
    __syncthreads();
    const double gs = live ? -0.5 * P / s + rr / (2.0 * s * s) : 0.0;
    const double b = (mine && live) ? y[lane * MVN_LD + P] : 0.0;
    double u = 0.0;
    for (int p = 0; p < P; ++p) {
        const double rp = __shfl(r, p, 32);
        if (mine) u += y[lane * MVN_LD + p] * rp;
        if (dY && valid) atomic_add(dY + c * P + p, (T)(gscale * b * rp / s));
    }
    if (!live) u = 0.0;
    if (dY && live && lane < P) atomic_add(dY + row * P + lane, (T)(-gscale * r / s));
    const double w = gs * b - u / s, gk = -2.0 * gs * b + u / s;
    sums.dn += b * w + (lane == 0 ? gs : 0.0);
    // the pairs of the row: (c_t, c_t') with G_A = b_t w_t', (c_t, x) with G_kappa, and (x, x) with G_a in lane 0
    for (int tp = 0; tp < k; ++tp) {
        T z[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q) z[q] = __shfl(xc[q], tp, 32);
        const double g = b * __shfl(w, tp, 32);
        T d2[QP], red = 0;
#pragma unroll
        for (int q = 0; q < QP; ++q) { const T d = (xc[q] - z[q]) * m[q]; d2[q] = d * d; red += d2[q]; }
        T f, df;
        cov_slope<T, KIND>(red, f, df);
        sums.dv += g * (double)f;
        const double gw = g * (double)df;
#pragma unroll
        for (int q = 0; q < QP; ++q) sums.dl[q] += gw * (double)d2[q];
    }
    {
        T d2[QP], red = 0;
#pragma unroll
        for (int q = 0; q < QP; ++q) { const T d = (xc[q] - xi[q]) * m[q]; d2[q] = d * d; red += d2[q]; }
        T f, df;
        cov_slope<T, KIND>(red, f, df);
        sums.dv += gk * (double)f;
        const double gw = gk * (double)df;
#pragma unroll
        for (int q = 0; q < QP; ++q) sums.dl[q] += gw * (double)d2[q];
        cov_slope<T, KIND>((T)0, f, df);                     // (x, x): no slope in the lengthscale at distance 0
        if (lane == 0) sums.dv += gs * (double)f;
    }
    __syncthreads();
}

// the scale of coordinate q: c / l_q, 0 for q >= Q
template <typename T, int QP, int KIND>
__device__ __forceinline__ void vecchia_scales(const VecchiaOps<T>& o, T* m) {
#pragma unroll
    for (int q = 0; q < QP; ++q) m[q] = q < o.Q ? coord_scale<T, KIND>() / o.ls[o.ard ? q : 0] : (T)0;
}

// acc: the zeroed doubles of the plan -- [0] the value (LOGPDF); [0, QP) the lengthscale's sums, [QP] the variance's, [QP + 1] the noise's (BWD)
template <typename T, int QP, int KIND, int CALL>
__global__ __launch_bounds__(VECCHIA_THREADS) void vecchia_kernel(VecchiaOps<T> o, const T* __restrict__ g, T* mean_out, T* var_out, T* terms_out,
                                                                  T* dY, double* __restrict__ acc, int want_dl, int want_dv, int want_dn) {
    __shared__ VecchiaTiles tiles[VECCHIA_ROWS];
    const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
    T m[QP];
    vecchia_scales<T, QP, KIND>(o, m);
    const T variance = o.var[0];
    const double noise = (double)o.noise[0];
    const double gscale = CALL == VECCHIA_BWD ? (double)g[0] : 1.0;
    VecchiaSums<QP> sums;
#pragma unroll
    for (int q = 0; q < QP; ++q) sums.dl[q] = 0.0;
    sums.dv = sums.dn = sums.value = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * VECCHIA_ROWS; base < o.rows; base += (int64_t)gridDim.x * VECCHIA_ROWS)
        vecchia_row<T, QP, KIND, CALL>(o, tiles[grp], base + grp, lane, m, variance, noise, gscale, mean_out, var_out, terms_out, dY, sums);
    if (CALL == VECCHIA_LOGPDF) {
        __shared__ double part[16];
        const double t = block_sum(sums.value, part);
        if (threadIdx.x == 0) atomic_add(acc, t);
    }
    if (CALL == VECCHIA_BWD) {
        __shared__ double part[16];
        if (want_dl) {
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                if (q < o.Q) {          // (uniform over the workgroup)
                    const double t = block_sum(sums.dl[q], part);
                    if (threadIdx.x == 0) atomic_add(acc + q, t);
                }
            }
        }
        if (want_dv) { const double t = block_sum(sums.dv, part); if (threadIdx.x == 0) atomic_add(acc + QP, t); }
        if (want_dn) { const double t = block_sum(sums.dn, part); if (threadIdx.x == 0) atomic_add(acc + QP + 1, t); }
    }
}

// value_out[0] = acc[0]
__global__ void vecchia_value_close_kernel(const double* __restrict__ acc, double* __restrict__ value_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) value_out[0] = acc[0];
}

// dls[q] = g (-2 variance / l_q) acc[q] (d red / d l_q = -2 d_q^2 / l_q; summed over q without ARD), dvar = g acc[QP], dnoise = g acc[QP + 1]:
// one thread, one rounding each
template <typename T, int QP>
__global__ void vecchia_bwd_close_kernel(VecchiaOps<T> o, const T* __restrict__ g, const double* __restrict__ acc, T* dls, T* dvar, T* dnoise) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double gs = (double)g[0], variance = (double)o.var[0];
    if (dls) {
        double all = 0.0;
        for (int q = 0; q < o.Q; ++q) {
            const double d = -2.0 * gs * variance / (double)o.ls[o.ard ? q : 0] * acc[q];
            if (o.ard) dls[q] = (T)d;
            all += d;
        }
        if (!o.ard) dls[0] = (T)all;
    }
    if (dvar) dvar[0] = (T)(gs * acc[QP]);
    if (dnoise) dnoise[0] = (T)(gs * acc[QP + 1]);
}

struct VecchiaArgs {
    int kind = MXF_K_RBF, dtype = MXF_F32; int64_t Nt = 0, N = 0; int Q = 0, P = 0, k = 0, ard = 0;
    const void *Xt = nullptr, *X = nullptr, *Y = nullptr; const int32_t* nbr = nullptr; const void *ls = nullptr, *var = nullptr, *noise = nullptr;
    void *mean_out = nullptr, *var_out = nullptr;                                                      // cond
    void* terms_out = nullptr; double* value_out = nullptr;                                            // logpdf
    const void* g = nullptr; void *dls = nullptr, *dvar = nullptr, *dnoise = nullptr, *dY = nullptr;   // bwd
};

// ask the plan (fused_plan.h: vecchia_plan), carve, launch
template <typename T, int QP, int KIND, int CALL>
int vecchia_launch(mxf_handle h, const char* name, const VecchiaArgs& a, const VecchiaPlan& p, hipStream_t st) {
    const VecchiaOps<T> o = {p.rows, a.N, a.Q, a.P, a.k, a.ard, (const T*)(CALL == VECCHIA_COND ? a.Xt : a.X), (const T*)a.X, (const T*)a.Y, a.nbr,
                             (const T*)a.ls, (const T*)a.var, (const T*)a.noise};
    double* acc = nullptr;
    if (p.n_acc) {
        char* ws = (char*)mxf_ws(h, p.bytes);
        if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
        acc = (double*)(ws + p.at_acc);
        MXF_HIP(h, hipMemsetAsync(acc, 0, p.zero_bytes, st));
    }
    if (p.dy_bytes) MXF_HIP(h, hipMemsetAsync(a.dY, 0, p.dy_bytes, st));
    hipLaunchKernelGGL((vecchia_kernel<T, QP, KIND, CALL>), dim3(p.grid), dim3(VECCHIA_THREADS), 0, st, o, (const T*)a.g, (T*)a.mean_out, (T*)a.var_out,
                       (T*)a.terms_out, (T*)a.dY, acc, (int)(a.dls != nullptr), (int)(a.dvar != nullptr), (int)(a.dnoise != nullptr));
    if (CALL == VECCHIA_LOGPDF) hipLaunchKernelGGL(vecchia_value_close_kernel, dim3(1), dim3(64), 0, st, (const double*)acc, a.value_out);
    if (CALL == VECCHIA_BWD)
        hipLaunchKernelGGL((vecchia_bwd_close_kernel<T, QP>), dim3(1), dim3(64), 0, st, o, (const T*)a.g, (const double*)acc, (T*)a.dls, (T*)a.dvar,
                           (T*)a.dnoise);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

template <int CALL>
int run(mxf_handle h, const char* name, const VecchiaArgs& a, void* stream) {
    if (!h) return -1;
    if (a.dtype != MXF_F32 && a.dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, a.dtype);
    if (a.kind != MXF_K_RBF && a.kind != MXF_K_MATERN12 && a.kind != MXF_K_MATERN32 && a.kind != MXF_K_MATERN52)
        MXF_FAIL(h, -2, "%s: stationary kernels only (kind %d)", name, a.kind);
    const VecchiaPlan p = vecchia_plan({.esize = mxf_esize(a.dtype), .call = CALL, .Nt = a.Nt, .N = a.N, .Q = a.Q, .P = a.P, .k = a.k,
                                        .has_Xt = a.Xt != nullptr, .has_X = a.X != nullptr, .has_Y = a.Y != nullptr, .has_nbr = a.nbr != nullptr,
                                        .has_ls = a.ls != nullptr, .has_var = a.var != nullptr, .has_noise = a.noise != nullptr,
                                        .has_mean = a.mean_out != nullptr, .has_vout = a.var_out != nullptr, .has_value = a.value_out != nullptr,
                                        .has_g = a.g != nullptr, .has_dY = a.dY != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    return dispatch<MXF_F32, MXF_F64>(a.dtype, [&](auto dt) {
        return dispatch<4, 8, 16>(p.qp, [&](auto qp) {
            return dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52>(a.kind, [&](auto kind) {
                return vecchia_launch<mxf_elem_t<decltype(dt)::value>, decltype(qp)::value, decltype(kind)::value, CALL>(h, name, a, p,
                                                                                                                         (hipStream_t)stream);
            });
        });
    });
}

}  // namespace

extern "C" int mxf_vecchia_cond(mxf_handle h, int kind, int dtype, int64_t Nt, int64_t N, int Q, int P, int k, int ard, const void* Xt, const void* X,
                                const void* Y, const int32_t* nbr, const void* lengthscale, const void* variance, const void* noise, void* mean_out,
                                void* var_out, void* stream) {
    const VecchiaArgs a = {.kind = kind, .dtype = dtype, .Nt = Nt, .N = N, .Q = Q, .P = P, .k = k, .ard = ard, .Xt = Xt, .X = X, .Y = Y, .nbr = nbr,
                           .ls = lengthscale, .var = variance, .noise = noise, .mean_out = mean_out, .var_out = var_out};
    return run<VECCHIA_COND>(h, "mxf_vecchia_cond", a, stream);
}

extern "C" int mxf_vecchia_logpdf(mxf_handle h, int kind, int dtype, int64_t N, int Q, int P, int k, int ard, const void* X, const void* Y,
                                  const int32_t* nbr, const void* lengthscale, const void* variance, const void* noise, void* terms_out,
                                  double* value_out, void* stream) {
    const VecchiaArgs a = {.kind = kind, .dtype = dtype, .N = N, .Q = Q, .P = P, .k = k, .ard = ard, .X = X, .Y = Y, .nbr = nbr, .ls = lengthscale,
                           .var = variance, .noise = noise, .terms_out = terms_out, .value_out = value_out};
    return run<VECCHIA_LOGPDF>(h, "mxf_vecchia_logpdf", a, stream);
}

extern "C" int mxf_vecchia_logpdf_bwd(mxf_handle h, int kind, int dtype, int64_t N, int Q, int P, int k, int ard, const void* X, const void* Y,
                                      const int32_t* nbr, const void* lengthscale, const void* variance, const void* noise, const void* g, void* dls,
                                      void* dvar, void* dnoise, void* dY, void* stream) {
    const VecchiaArgs a = {.kind = kind, .dtype = dtype, .N = N, .Q = Q, .P = P, .k = k, .ard = ard, .X = X, .Y = Y, .nbr = nbr, .ls = lengthscale,
                           .var = variance, .noise = noise, .g = g, .dls = dls, .dvar = dvar, .dnoise = dnoise, .dY = dY};
    return run<VECCHIA_BWD>(h, "mxf_vecchia_logpdf_bwd", a, stream);
}
