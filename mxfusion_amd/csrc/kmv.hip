// Matrix-free product of a stationary covariance matrix with a block of vectors, and the reverse mode of its bilinear form in the kernel
// parameters (gfx950); the covariance of a pair is kmv.h's, the function mxf_gram evaluates.
//   out[s,n,j] = sum_n2 k(X[s,n,:], X2[s,n2,:]) V[s,n2,j]  (+ diag_add[s] V[s,n,j], square)                         (S, N, J)
//   dls, dvar += the gradient of sum_j w_j A[s,:,j]^T K(X, X2) V[s,:,j] in lengthscale and variance
// No reference counterpart: the reference factorises the N x N matrix.  Conjugate gradients on K + sigma^2 I (Wang et al. 2019) need only this.
//
// Nothing of size N x N2 is stored.  Row-owned, as rff_fwd_kernel of rff.hip: a thread owns a row n with its centred, pre-scaled x in registers
// (Q padded to QP = 4 / 8 / 16); the centred, pre-scaled and padded rows of X2 and a block of JB columns of V -- written once per call by the
// two prep kernels -- are uniform over the wavefront and arrive as scalar loads.  The covariance is evaluated once per pair (n, n2), at unit
// variance, and multiplied into JB accumulators; JB = 4 for J <= 4 and 16 above, and a larger J takes further passes over n2 inside the same
// launch.  A thread sums KMV_CH values of n2 in T, adds that to a double register and writes its own results, times the variance: no atomics.
// n2 is split over grid.y only while the row blocks alone give fewer than KMV_TARGET workgroups; the partial sums then meet in zeroed double
// scratch that one kernel narrows.  Both operands are centred on the first row of X2 before they are scaled, as mxf_gram centres its own.
//
// The reverse mode forms the cotangent of a pair, g = sum_j w_j A[n,j] V[n2,j], in registers (the weights are multiplied into the prepared
// V, KMV_WG columns per prep launch) and sums g f and g f' ((x_q - z_q) c / l_q)^2 per thread, per wavefront in double, and over the
// wavefronts in zeroed double scratch; one thread adds the totals to the caller's buffers (the pattern of psi_close_kernel).
#include "common.h"
#include "fused_plan.h"      // KMV_*: the tile sizes; kmv_plan
#include "kmv.h"
#include "shared_grad.h"   // mxf_narrow_kernel

namespace {

template <typename T>
struct KmvOps {
    int S; int64_t N, N2; int Q, J, ard, square;
    const T* X; int64_t ss_X;
    const T* Z; int64_t ss_Z;       // the second operand: X2, or X itself for a square product
    const T* ls; int64_t ss_ls;
    const T* var; int64_t ss_var;
    const T* da; int64_t ss_da;     // diag_add, or null
    const T* V; int64_t ss_V;
};

struct KmvWeights { double w[KMV_WG]; int use; };

// coordinate q of a row of X or X2 as the kernels subtract them: centred on the first row of the second operand, times c / l_q; 0 for q >= Q
template <typename T, int KIND>
__device__ __forceinline__ T kmv_coord(const KmvOps<T>& o, int64_t s, const T* row, int q) {
    if (q >= o.Q) return (T)0;
    const T m = coord_scale<T, KIND>() / o.ls[s * o.ss_ls + (o.ard ? q : 0)];
    return (row[q] - o.Z[s * o.ss_Z + q]) * m;
}

// zs (S|1, N2, QP): the rows of the second operand; one copy where the samples share X2 and the lengthscale
template <typename T, int QP, int KIND>
__global__ __launch_bounds__(256) void kmv_prep_z_kernel(KmvOps<T> o, int64_t S_z, T* __restrict__ zs) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S_z * o.N2; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / o.N2, n2 = i - s * o.N2;
        const T* row = o.Z + s * o.ss_Z + n2 * o.Q;
#pragma unroll
        for (int q = 0; q < QP; ++q) zs[i * QP + q] = kmv_coord<T, KIND>(o, s, row, q);
    }
}

// vb (S|1, npass, N2, JB): V in blocks of JB columns padded with zeros, passes [pass0, pass0 + np) of them; with wt.use, times the weights of
// those columns (wt.w[0] is the weight of column pass0 JB)
template <typename T, int JB>
__global__ __launch_bounds__(256) void kmv_prep_v_kernel(KmvOps<T> o, int64_t S_V, int npass, int pass0, int np, KmvWeights wt, T* __restrict__ vb) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S_V * np * o.N2; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / (np * o.N2), r = i - s * np * o.N2, pr = r / o.N2, n2 = r - pr * o.N2;
        const T* v = o.V + s * o.ss_V + n2 * o.J;
        T* dst = vb + ((s * npass + pass0 + pr) * o.N2 + n2) * JB;
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            const int64_t jr = pr * JB + j, jj = (int64_t)pass0 * JB + jr;
            T val = jj < o.J ? v[jj] : (T)0;
            if (wt.use) val *= (T)wt.w[jr < KMV_WG ? jr : KMV_WG - 1];
            dst[j] = val;
        }
    }
}

// a thread's own row; a dead thread reads the last row
template <typename T, int QP, int KIND>
__device__ __forceinline__ void kmv_own_row(const KmvOps<T>& o, int64_t s, int64_t n, T* x) {
    const T* row = o.X + s * o.ss_X + n * o.Q;
#pragma unroll
    for (int q = 0; q < QP; ++q) x[q] = kmv_coord<T, KIND>(o, s, row, q);
}

// the n2 of workgroup row blockIdx.y: [c0, c1), chunks of `ch` values (a multiple of KMV_CH)
__device__ __forceinline__ void kmv_range(int64_t N2, int64_t ch, int64_t& c0, int64_t& c1) {
    c0 = (int64_t)blockIdx.y * ch;
    c1 = c0 + ch < N2 ? c0 + ch : N2;
}

// out[s][n][j] = variance sum_n2 f(n, n2) V[n2][j] (+ diag_add V[n][j]).  With grid.y = 1 a thread writes its row's results (out); otherwise
// it adds them to the zeroed doubles acc (S, N, J), narrowed by mxf_narrow_kernel; the diagonal term is workgroup row 0's.
template <typename T, int QP, int JB, int KIND>
__global__ __launch_bounds__(KMV_RB) void kmv_fwd_kernel(KmvOps<T> o, const T* __restrict__ zs_all, int64_t ss_zs, const T* __restrict__ vb_all,
                                                         int64_t ss_vb, int npass, int64_t ch, double* __restrict__ acc, T* __restrict__ out) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * KMV_RB + threadIdx.x;
    const bool live = n < o.N;
    T x[QP];
    kmv_own_row<T, QP, KIND>(o, s, live ? n : o.N - 1, x);
    int64_t c0, c1;
    kmv_range(o.N2, ch, c0, c1);
    const T* zs = zs_all + s * ss_zs;
    const double variance = (double)o.var[s * o.ss_var];
    const bool diag = o.square && o.da != nullptr && blockIdx.y == 0;
    const double dadd = diag ? (double)o.da[s * o.ss_da] : 0.0;
    for (int pass = 0; pass < npass; ++pass) {
        const T* vb = vb_all + s * ss_vb + (int64_t)pass * o.N2 * JB;
        double R[JB];
#pragma unroll
        for (int j = 0; j < JB; ++j) R[j] = 0;
        for (int64_t cb = c0; cb < c1; cb += KMV_CH) {
            const int64_t ce = cb + KMV_CH < c1 ? cb + KMV_CH : c1;
            T r_[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) r_[j] = 0;
            for (int64_t c = cb; c < ce; ++c) {         // z_c and the block of V are uniform over the wavefront: scalar loads
                const T* z = zs + c * QP;
                T red = 0;
#pragma unroll
                for (int q = 0; q < QP; ++q) { const T d = x[q] - z[q]; red = fma(d, d, red); }
                const T f = cov_from<T, KIND>(red, (T)1);
                const T* v = vb + c * JB;
#pragma unroll
                for (int j = 0; j < JB; ++j) r_[j] += v[j] * f;
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) R[j] += (double)r_[j];
        }
        if (live) {
            const int64_t at = (s * o.N + n) * o.J + (int64_t)pass * JB;
            const T* vrow = o.V + s * o.ss_V + n * o.J + (int64_t)pass * JB;         // read only where diag: the product is square, N2 = N
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                if (pass * JB + j < o.J) {
                    double r = variance * R[j];
                    if (diag) r += dadd * (double)vrow[j];
                    if (acc) atomic_add(acc + at + j, r);
                    else out[at + j] = (T)r;
                }
            }
        }
    }
}

// The sums of the reverse mode: dlacc[s][q] += sum_{n,n2} g f' d_q^2 and dvacc[s] += sum_{n,n2} g f, with d_q the scaled difference and
// g = sum_j (w_j V[n2][j]) A[n][j] (the prepared V carries the weights).  Per thread in T over KMV_CH values of n2, then in a double register;
// per wavefront in double; one atomic per wavefront and sum into the zeroed doubles.
template <typename T, int QP, int JB, int KIND>
__global__ __launch_bounds__(KMV_RB) void kmv_bwd_kernel(KmvOps<T> o, const T* __restrict__ zs_all, int64_t ss_zs, const T* __restrict__ vb_all,
                                                         int64_t ss_vb, int npass, int64_t ch, const T* __restrict__ A, int64_t ss_A,
                                                         double* __restrict__ dlacc, double* __restrict__ dvacc) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * KMV_RB + threadIdx.x;
    const bool live = n < o.N;
    T x[QP];
    kmv_own_row<T, QP, KIND>(o, s, live ? n : o.N - 1, x);
    int64_t c0, c1;
    kmv_range(o.N2, ch, c0, c1);
    const T* zs = zs_all + s * ss_zs;
    double DL[QP], DV = 0;
#pragma unroll
    for (int q = 0; q < QP; ++q) DL[q] = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const T* vb = vb_all + s * ss_vb + (int64_t)pass * o.N2 * JB;
        const T* a_row = A + s * ss_A + (live ? n : o.N - 1) * o.J;
        T a[JB];
#pragma unroll
        for (int j = 0; j < JB; ++j) a[j] = (live && pass * JB + j < o.J) ? a_row[pass * JB + j] : (T)0;
        for (int64_t cb = c0; cb < c1; cb += KMV_CH) {
            const int64_t ce = cb + KMV_CH < c1 ? cb + KMV_CH : c1;
            T dl_[QP], dv_ = 0;
#pragma unroll
            for (int q = 0; q < QP; ++q) dl_[q] = 0;
            for (int64_t c = cb; c < ce; ++c) {
                const T *z = zs + c * QP, *v = vb + c * JB;
                T g = 0;
#pragma unroll
                for (int j = 0; j < JB; ++j) g += a[j] * v[j];
                T d[QP], red = 0;
#pragma unroll
                for (int q = 0; q < QP; ++q) { d[q] = x[q] - z[q]; red = fma(d[q], d[q], red); }
                T f, df;
                cov_slope<T, KIND>(red, f, df);
                dv_ += g * f;
                const T gw = g * df;
#pragma unroll
                for (int q = 0; q < QP; ++q) dl_[q] += gw * (d[q] * d[q]);
            }
#pragma unroll
            for (int q = 0; q < QP; ++q) DL[q] += (double)dl_[q];
            DV += (double)dv_;
        }
    }
    const bool lane0 = (threadIdx.x & 63) == 0;
    if (dlacc) {
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            if (q < o.Q) {          // (uniform over the wavefront)
                const double t = wave_sum(DL[q]);
                if (lane0) atomic_add(dlacc + s * QP + q, t);
            }
        }
    }
    if (dvacc) {
        const double t = wave_sum(DV);
        if (lane0) atomic_add(dvacc + s, t);
    }
}

// dls[q] += -2 variance / l_q dlacc[q] (d red / d l_q = -2 d_q^2 / l_q; summed over q without ARD) and dvar += dvacc, over the samples that
// share them: one thread, no atomics
template <typename T, int QP>
__global__ void kmv_close_kernel(KmvOps<T> o, const double* __restrict__ dlacc, const double* __restrict__ dvacc, T* dls, int own_l, T* dvar, int own_v) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int nl = o.ard ? o.Q : 1;
    for (int64_t s = 0; s < o.S; ++s) {
        const double variance = (double)o.var[s * o.ss_var];
        if (dls)
            for (int q = 0; q < o.Q; ++q) {
                T* d = dls + (own_l ? s : 0) * nl + (o.ard ? q : 0);
                *d = (T)((double)*d - 2.0 * variance / (double)o.ls[s * o.ss_ls + (o.ard ? q : 0)] * dlacc[s * QP + q]);
            }
        if (dvar) {
            T* d = dvar + (own_v ? s : 0);
            *d = (T)((double)*d + dvacc[s]);
        }
    }
}

struct KmvArgs {
    int kind = MXF_K_RBF, dtype = MXF_F32, S = 0; int64_t N = 0, N2 = 0; int Q = 0, J = 0;
    const void *X = nullptr, *X2 = nullptr, *ls = nullptr, *var = nullptr, *da = nullptr, *V = nullptr;
    int64_t ss_X = 0, ss_X2 = 0, ss_ls = 0, ss_var = 0, ss_da = 0, ss_V = 0; int ard = 0;
    void* out = nullptr;                                                                                      // forward
    const void* A = nullptr; int64_t ss_A = 0; const double* w = nullptr; void *dls = nullptr, *dvar = nullptr;      // reverse
};

// ask the plan (fused_plan.h: kmv_plan), carve, launch
template <typename T, int QP, int JB, int KIND>
int kmv_launch(mxf_handle h, const char* name, const KmvArgs& a, const KmvPlan& p, bool bwd, hipStream_t st) {
    const KmvOps<T> o = {a.S, a.N, p.N2, a.Q, a.J, a.ard, (int)p.square, (const T*)a.X, a.ss_X, (const T*)(p.square ? a.X : a.X2), p.ss_Z,
                         (const T*)a.ls, a.ss_ls, (const T*)a.var, a.ss_var, (const T*)a.da, a.ss_da, (const T*)a.V, a.ss_V};
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    double* zero = p.n_zero ? (double*)(ws + p.at_zero) : nullptr;
    if (zero) MXF_HIP(h, hipMemsetAsync(zero, 0, p.n_zero * sizeof(double), st));
    T *zs = (T*)(ws + p.at_zs), *vb = (T*)(ws + p.at_vb);
    hipLaunchKernelGGL((kmv_prep_z_kernel<T, QP, KIND>), dim3(grid_for(p.n_prep_z)), dim3(256), 0, st, o, p.S_z, zs);
    for (int pass0 = 0; pass0 < p.npass; pass0 += p.gp) {
        const KmvPrepV pv = kmv_prep_v(p, pass0);
        KmvWeights wt;
        wt.use = bwd;
        for (int k = 0; k < KMV_WG; ++k) wt.w[k] = (bwd && (int64_t)pass0 * JB + k < a.J) ? a.w[(int64_t)pass0 * JB + k] : 0.0;
        hipLaunchKernelGGL((kmv_prep_v_kernel<T, JB>), dim3(grid_for(pv.items)), dim3(256), 0, st, o, p.S_V, p.npass, pass0, pv.np, wt, vb);
    }
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    if (!bwd) {
        hipLaunchKernelGGL((kmv_fwd_kernel<T, QP, JB, KIND>), grid, dim3(KMV_RB), 0, st, o, (const T*)zs, p.ss_zs, (const T*)vb, p.ss_vb, p.npass, p.ch,
                           zero, (T*)a.out);
        if (zero) hipLaunchKernelGGL((mxf_narrow_kernel<T>), dim3(grid_for(p.n_out)), dim3(256), 0, st, p.n_out, (const double*)zero, (T*)a.out);
    } else {
        double *dlacc = zero, *dvacc = (double*)(ws + p.at_dv);
        hipLaunchKernelGGL((kmv_bwd_kernel<T, QP, JB, KIND>), grid, dim3(KMV_RB), 0, st, o, (const T*)zs, p.ss_zs, (const T*)vb, p.ss_vb, p.npass, p.ch,
                           (const T*)a.A, a.ss_A, a.dls ? dlacc : nullptr, a.dvar ? dvacc : nullptr);
        hipLaunchKernelGGL((kmv_close_kernel<T, QP>), dim3(1), dim3(64), 0, st, o, (const double*)dlacc, (const double*)dvacc, (T*)a.dls,
                           (int)(a.ss_ls != 0), (T*)a.dvar, (int)(a.ss_var != 0));
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

int run(mxf_handle h, const char* name, const KmvArgs& a, bool bwd, void* stream) {
    if (!h) return -1;
    if (a.dtype != MXF_F32 && a.dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, a.dtype);
    if (a.kind != MXF_K_RBF && a.kind != MXF_K_MATERN12 && a.kind != MXF_K_MATERN32 && a.kind != MXF_K_MATERN52)
        MXF_FAIL(h, -2, "%s: stationary kernels only (kind %d)", name, a.kind);
    const KmvPlan p = kmv_plan({.esize = mxf_esize(a.dtype), .bwd = bwd, .S = a.S, .N = a.N, .N2 = a.N2, .Q = a.Q, .J = a.J, .ard = a.ard,
                                .ss_X = a.ss_X, .ss_X2 = a.ss_X2, .ss_ls = a.ss_ls, .ss_var = a.ss_var, .ss_da = a.ss_da, .ss_V = a.ss_V, .ss_A = a.ss_A,
                                .has_X = a.X != nullptr, .has_X2 = a.X2 != nullptr, .has_ls = a.ls != nullptr, .has_var = a.var != nullptr,
                                .has_da = a.da != nullptr, .has_V = a.V != nullptr, .has_out = a.out != nullptr, .has_A = a.A != nullptr,
                                .has_w = a.w != nullptr, .has_dls = a.dls != nullptr, .has_dvar = a.dvar != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    return dispatch<MXF_F32, MXF_F64>(a.dtype, [&](auto dt) {
        return dispatch<4, 8, 16>(p.qp, [&](auto qp) {
            return dispatch<KMV_JB_SMALL, KMV_JB>(p.jb, [&](auto jb) {
                return dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52>(a.kind, [&](auto kind) {
                    return kmv_launch<mxf_elem_t<decltype(dt)::value>, decltype(qp)::value, decltype(jb)::value, decltype(kind)::value>(
                        h, name, a, p, bwd, (hipStream_t)stream);
                });
            });
        });
    });
}

}  // namespace

extern "C" int mxf_kmv(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int J, const void* X, int64_t strideS_X, const void* X2,
                       int64_t strideS_X2, const void* lengthscale, int64_t strideS_ls, int ard, const void* variance, int64_t strideS_var,
                       const void* diag_add, int64_t strideS_da, const void* V, int64_t strideS_V, void* out, void* stream) {
    const KmvArgs a = {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .J = J, .X = X, .X2 = X2, .ls = lengthscale, .var = variance,
                       .da = X2 ? nullptr : diag_add, .V = V, .ss_X = strideS_X, .ss_X2 = strideS_X2, .ss_ls = strideS_ls, .ss_var = strideS_var,
                       .ss_da = strideS_da, .ss_V = strideS_V, .ard = ard, .out = out};
    return run(h, "mxf_kmv", a, false, stream);
}

extern "C" int mxf_kmv_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int J, const void* X, int64_t strideS_X,
                           const void* X2, int64_t strideS_X2, const void* lengthscale, int64_t strideS_ls, int ard, const void* variance,
                           int64_t strideS_var, const void* A, int64_t strideS_A, const void* V, int64_t strideS_V, const double* w, void* dls_acc,
                           void* dvar_acc, void* stream) {
    const KmvArgs a = {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .J = J, .X = X, .X2 = X2, .ls = lengthscale, .var = variance,
                       .V = V, .ss_X = strideS_X, .ss_X2 = strideS_X2, .ss_ls = strideS_ls, .ss_var = strideS_var, .ss_V = strideS_V, .ard = ard,
                       .A = A, .ss_A = strideS_A, .w = w, .dls = dls_acc, .dvar = dvar_acc};
    return run(h, "mxf_kmv_bwd", a, true, stream);
}
