// Reverse mode of the matrix-free kernel product in its inputs (gfx950): the gradient of  L = sum_s sum_j w_j A[s,:,j]^T K(X[s], X2[s]) V[s,:,j]
// in X and X2, the dX / dX2 of mxf_gram_bwd for the cotangent dK = sum_j w_j A[:,j] V[:,j]^T, which is never stored.  With kmv.h's scaled
// difference d_q = (x_q - z_q) c / l_q, red = sum_q d_q^2, f' = df / dred (cov_slope) and g_nm = sum_j w_j A[n,j] V[m,j]:
//   dX [n,q] += variance (c / l_q) 2 sum_m g_nm f'(red_nm) d_q(n,m),     dX2[m,q] -= the same sum over n
// No reference counterpart: the reference differentiates through the stored N x N matrix.
//
// Row-owned, as kmv_bwd_kernel: a thread owns a row n with its centred, pre-scaled x[QP] and its factor of g, a[JB], in registers; the
// prepared rows of the other operand and the other, weighted factor (kmv_prep.h's two kernels) are uniform over the wavefront and arrive as
// scalar loads.  Per pair: g (JB multiplies), the QP differences, one cov_slope, QP multiply-adds.  The thread sums g f' d_q over KMV_CH pairs
// in T, adds that to double DX[QP] and at the end writes its own Q results, times 2 variance c / l_q, with ordinary stores: no atomics on the
// result.  Passes for J > JB add, because the sum is linear in g.  The X2 side is the same kernel with the roles exchanged (the difference
// changes sign with them): a thread owns a row m of X2 and of V, X and the weighted A are streamed, both still centred on X2's first row.
// The square product takes one fused pass: the thread holds a_n and v_n, both weighted factors are streamed and g_nm + g_mn multiplies the
// slope, so a pair's covariance is evaluated once.  Only float64 at JB = 16 would spill in that form and runs the two role passes into dX
// instead (kmv_bwd_x_plan.h has the passes).
//
// Doubles in scratch take the result in two cases only: the streamed rows split over grid.y (kmv_plan's rule; zeroed, atomics), and an
// operand shared by S > 1 samples (one plain store per sample).  One closing launch adds them to the caller's buffer, over the samples in
// ascending order.
#include "kmv_bwd_x_plan.h"
#include "kmv_prep.h"

namespace {

// DX[q] = sum over the streamed rows c of (a . vb_c (+ b . ub_c)) f'(red) d_q; out[s|0][n][q] += 2 variance c / l_q DX[q], or the same into
// acc (S, N, Q): added where grid.y > 1, stored otherwise
template <typename T, int QP, int JB, int KIND, bool FUSED>
__global__ __launch_bounds__(KMV_RB) void kmv_bwd_x_kernel(KmvOps<T> o, const T* __restrict__ zs_all, int64_t ss_zs, const T* __restrict__ vb_all,
                                                           int64_t ss_vb, const T* __restrict__ ub_all, int64_t ss_ub, int npass, int64_t ch,
                                                           const T* __restrict__ A, int64_t ss_A, const T* __restrict__ B, int64_t ss_B,
                                                           double* __restrict__ acc, T* out, int own_out) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * KMV_RB + threadIdx.x;
    const bool live = n < o.N;
    const int64_t row = live ? n : o.N - 1;
    T x[QP];
    kmv_own_row<T, QP, KIND>(o, s, row, x);
    int64_t c0, c1;
    kmv_range(o.N2, ch, c0, c1);
    // where the thread's Q results go, per thread and ahead of the loops: the scalar registers are the streamed operands'
    double* const p_acc = acc ? acc + (s * o.N + row) * o.Q : nullptr;
    T* const p_out = out + ((own_out ? s : 0) * o.N + row) * o.Q;
    const T* const a_row = A + s * ss_A + row * o.J;
    const T* const b_row = FUSED ? B + s * ss_B + row * o.J : nullptr;
    const double v2 = 2.0 * (double)o.var[s * o.ss_var];
    const T* const ls = o.ls + s * o.ss_ls;
    const int ls_step = o.ard ? 1 : 0;
    // z_c and the blocks of the factors are uniform over the wavefront: scalar loads, the pointers advanced pair by pair; a pass ends `skip`
    // blocks before the next one's first
    const int64_t cnt = c1 - c0, skip = (o.N2 - cnt) * JB;
    const T* z = zs_all + s * ss_zs + c0 * QP;
    const T* v = vb_all + s * ss_vb + c0 * JB;
    const T* u = FUSED ? ub_all + s * ss_ub + c0 * JB : nullptr;
    double DX[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) DX[q] = 0;
    for (int pass = 0; pass < npass; ++pass, z -= cnt * QP, v += skip) {
        if constexpr (FUSED) { if (pass) u += skip; }
        T a[JB], b[FUSED ? JB : 1];
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            const bool in = live && pass * JB + j < o.J;
            a[j] = in ? a_row[pass * JB + j] : (T)0;
            if constexpr (FUSED) b[j] = in ? b_row[pass * JB + j] : (T)0;
        }
        for (int64_t left = cnt; left > 0; left -= KMV_CH) {
            const int m = left < KMV_CH ? (int)left : KMV_CH;
            T dx_[QP];
#pragma unroll
            for (int q = 0; q < QP; ++q) dx_[q] = 0;
            for (int i = 0; i < m; ++i, z += QP, v += JB) {
                T g = 0;
#pragma unroll
                for (int j = 0; j < JB; ++j) g += a[j] * v[j];
                if constexpr (FUSED) {
#pragma unroll
                    for (int j = 0; j < JB; ++j) g += b[j] * u[j];
                    u += JB;
                }
                T d[QP], red = 0;
#pragma unroll
                for (int q = 0; q < QP; ++q) { d[q] = x[q] - z[q]; red = fma(d[q], d[q], red); }
                T f, df;
                cov_slope<T, KIND>(red, f, df);
                const T gw = g * df;
#pragma unroll
                for (int q = 0; q < QP; ++q) dx_[q] += gw * d[q];
            }
#pragma unroll
            for (int q = 0; q < QP; ++q) DX[q] += (double)dx_[q];
        }
    }
    if (!live) return;
    const bool split = gridDim.y > 1;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        if (q < o.Q) {
            const double r = v2 * (double)(coord_scale<T, KIND>() / ls[q * ls_step]) * DX[q];
            if (p_acc) {
                if (split) atomic_add(p_acc + q, r);
                else p_acc[q] = r;
            } else p_out[q] = (T)((double)p_out[q] + r);
        }
    }
}

__global__ __launch_bounds__(256) void kmv_bwd_x_zero_kernel(int64_t total, double* __restrict__ acc) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) acc[i] = 0;
}

// out[i] += sum_{s < S_sum} acc[s][i], the samples in ascending order, rounded once
template <typename T>
__global__ __launch_bounds__(256) void kmv_bwd_x_close_kernel(int64_t n_out, int64_t S_sum, const double* __restrict__ acc, T* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
        double t = 0;
        for (int64_t s = 0; s < S_sum; ++s) t += acc[s * n_out + i];
        out[i] = (T)((double)out[i] + t);
    }
}

struct KmvBwdXArgs {
    int kind = MXF_K_RBF, dtype = MXF_F32, S = 0; int64_t N = 0, N2 = 0; int Q = 0, J = 0;
    const void *X = nullptr, *X2 = nullptr, *ls = nullptr, *var = nullptr, *A = nullptr, *V = nullptr;
    int64_t ss_X = 0, ss_X2 = 0, ss_ls = 0, ss_var = 0, ss_A = 0, ss_V = 0; int ard = 0;
    const double* w = nullptr; void *dX = nullptr, *dX2 = nullptr;
};

// the blocks of JB weighted columns of o.V (S_V, npass, o.N2, JB) at dst
template <typename T, int JB>
void prep_factor(const KmvOps<T>& o, const KmvPlan& k, int64_t S_V, const double* w, T* dst, hipStream_t st) {
    KmvPlan kv = k;
    kv.S_V = S_V;
    for (int pass0 = 0; pass0 < k.npass; pass0 += k.gp) {
        const KmvPrepV pv = kmv_prep_v(kv, pass0);
        KmvWeights wt;
        wt.use = 1;
        for (int i = 0; i < KMV_WG; ++i) wt.w[i] = (int64_t)pass0 * JB + i < o.J ? w[(int64_t)pass0 * JB + i] : 0.0;
        hipLaunchKernelGGL((kmv_prep_v_kernel<T, JB>), dim3(grid_for(pv.items)), dim3(256), 0, st, o, S_V, k.npass, pass0, pv.np, wt, dst);
    }
}

// one pass: the roles (kmv_bwd_x_plan.h), the prep launches, the kernel, the closing launch
template <typename T, int QP, int JB, int KIND>
void launch_pass(const KmvBwdXArgs& a, const KmvBwdXPass& ps, char* ws, hipStream_t st) {
    const KmvPlan& k = ps.k;
    const T *X = (const T*)a.X, *X2 = (const T*)a.X2, *Am = (const T*)a.A, *Vm = (const T*)a.V;
    const T *own = ps.x2_side ? X2 : X, *str = ps.x2_side ? X : (k.square ? X : X2), *ctr = k.square ? X : X2;
    const int64_t ss_own = ps.x2_side ? a.ss_X2 : a.ss_X, ss_str = ps.x2_side ? a.ss_X : (k.square ? a.ss_X : a.ss_X2);
    const int64_t ss_ctr = k.square ? a.ss_X : a.ss_X2;
    const T *f_own = ps.own_V ? Vm : Am, *f_str = ps.own_V ? Am : Vm;           // the factors of g: the threads' own, and the streamed one
    const int64_t ss_f_own = ps.own_V ? a.ss_V : a.ss_A, ss_f_str = ps.own_V ? a.ss_A : a.ss_V;
    KmvOps<T> o = {a.S, ps.N, k.N2, a.Q, a.J, a.ard, (int)k.square, own, ss_own, str, ss_str, ctr, ss_ctr,
                   (const T*)a.ls, a.ss_ls, (const T*)a.var, a.ss_var, nullptr, 0, f_str, ss_f_str};
    T *zs = (T*)(ws + k.at_zs), *vb = (T*)(ws + k.at_vb), *ub = (T*)(ws + ps.at_ub);
    double* acc = ps.summed ? (double*)(ws + ps.at_acc) : nullptr;
    T* out = (T*)(ps.x2_side ? a.dX2 : a.dX);
    hipLaunchKernelGGL((kmv_prep_z_kernel<T, QP, KIND>), dim3(grid_for(k.n_prep_z)), dim3(256), 0, st, o, k.S_z, zs);
    prep_factor<T, JB>(o, k, k.S_V, a.w, vb, st);
    if (ps.fused) {         // the second streamed factor: the weighted A, beside the weighted V
        KmvOps<T> o2 = o;
        o2.V = Am; o2.ss_V = a.ss_A;
        prep_factor<T, JB>(o2, k, ps.S_U, a.w, ub, st);
    }
    if (ps.zeroed) hipLaunchKernelGGL(kmv_bwd_x_zero_kernel, dim3(grid_for(ps.n_acc)), dim3(256), 0, st, ps.n_acc, acc);
    const dim3 grid(k.grid[0], k.grid[1], k.grid[2]);
    auto run = [&](auto fused) {
        hipLaunchKernelGGL((kmv_bwd_x_kernel<T, QP, JB, KIND, decltype(fused)::value>), grid, dim3(KMV_RB), 0, st, o, (const T*)zs, k.ss_zs,
                           (const T*)vb, k.ss_vb, (const T*)ub, ps.ss_ub, k.npass, k.ch, f_own, ss_f_own, Vm, a.ss_V, acc, out, (int)(ps.S_out > 1));
    };
    if constexpr (kmv_bwd_x_fused(sizeof(T), QP, JB)) {           // the plan asks for no fused pass where the form would spill
        if (ps.fused) run(std::true_type{});
        else run(std::false_type{});
    } else run(std::false_type{});
    if (acc) hipLaunchKernelGGL((kmv_bwd_x_close_kernel<T>), dim3(grid_for(ps.n_out)), dim3(256), 0, st, ps.n_out, ps.S_sum, (const double*)acc, out);
}

}  // namespace

extern "C" int mxf_kmv_bwd_x(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int J, const void* X, int64_t strideS_X,
                             const void* X2, int64_t strideS_X2, const void* lengthscale, int64_t strideS_ls, int ard, const void* variance,
                             int64_t strideS_var, const void* A, int64_t strideS_A, const void* V, int64_t strideS_V, const double* w,
                             void* dX_acc, void* dX2_acc, void* stream) {
    const char* name = "mxf_kmv_bwd_x";
    if (!h) return -1;
    const KmvBwdXArgs a = {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .J = J, .X = X, .X2 = X2, .ls = lengthscale,
                           .var = variance, .A = A, .V = V, .ss_X = strideS_X, .ss_X2 = strideS_X2, .ss_ls = strideS_ls, .ss_var = strideS_var,
                           .ss_A = strideS_A, .ss_V = strideS_V, .ard = ard, .w = w, .dX = dX_acc, .dX2 = dX2_acc};
    if (dtype != MXF_F32 && dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, dtype);
    if (kind != MXF_K_RBF && kind != MXF_K_MATERN12 && kind != MXF_K_MATERN32 && kind != MXF_K_MATERN52)
        MXF_FAIL(h, -2, "%s: stationary kernels only (kind %d)", name, kind);
    const KmvBwdXPlan p = kmv_bwd_x_plan({.esize = mxf_esize(dtype), .S = S, .N = N, .N2 = N2, .Q = Q, .J = J, .ard = ard, .ss_X = strideS_X,
                                          .ss_X2 = strideS_X2, .ss_ls = strideS_ls, .ss_var = strideS_var, .ss_A = strideS_A, .ss_V = strideS_V,
                                          .has_X = X != nullptr, .has_X2 = X2 != nullptr, .has_ls = lengthscale != nullptr,
                                          .has_var = variance != nullptr, .has_A = A != nullptr, .has_V = V != nullptr, .has_w = w != nullptr,
                                          .has_dX = dX_acc != nullptr, .has_dX2 = dX2_acc != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    for (int i = 0; i < p.n; ++i) {
        const KmvBwdXPass& ps = p.pass[i];
        dispatch<MXF_F32, MXF_F64>(dtype, [&](auto dt) {
            return dispatch<4, 8, 16>(ps.k.qp, [&](auto qp) {
                return dispatch<KMV_JB_SMALL, KMV_JB>(ps.k.jb, [&](auto jb) {
                    return dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52>(kind, [&](auto kd) {
                        launch_pass<mxf_elem_t<decltype(dt)::value>, decltype(qp)::value, decltype(jb)::value, decltype(kd)::value>(
                            a, ps, ws, (hipStream_t)stream);
                        return 0;
                    });
                });
            });
        });
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}
