// Random Fourier feature expansion of stationary GP prior draws and its reverse mode in the inputs (gfx950); the element math is rff.h.
//   out[s,n,j] = sum_d cos(X[s,n,:] . Omega[s,d,:] + phase[s,d]) W[s,d,j]                                  (S, N, J)
//   dX[s,n,q] += -sum_d sin(X[s,n,:] . Omega[s,d,:] + phase[s,d]) Omega[s,d,q] sum_j G[s,n,j] W[s,d,j]
// No reference counterpart: the reference draws from the predictive distribution point by point or through an Nt x Nt factor.
//
// The N x D matrix of cosines is never stored.  Row-owned, as psi2_quad_rows_kernel of psi.hip: a thread owns a row n with x in registers (Q
// padded to QP = 4 / 8 / 16); omega_d (padded), phase_d and a block of JB weights W[d, j0 .. j0 + JB) -- written once per call by rff_prep_kernel
// -- are uniform over the wavefront and arrive as scalar loads.  The cosine is evaluated once per (n, d) and multiplied into JB accumulators;
// JB = 4 for J <= 4 and 16 above, and a larger J takes further passes over d inside the same launch.  A thread sums RFF_DCH values of d in T,
// adds that to a double register and writes its own results: no atomics.  Two cases sum across threads, both through doubles (zeroed handle
// scratch, narrowed or folded once; for float64 gradients the caller's buffer itself): d split over grid.y, taken only while the rows alone
// give fewer than RFF_TARGET workgroups, and the gradient of an X that S > 1 samples share.
//
// float32 evaluates the cosine and the sine with the hardware instructions, which take revolutions: rff_prep_kernel divides omega and phase
// by 2 pi (in double, one rounding), the argument is reduced with fract, and the gradient is multiplied by 2 pi once per row.  float64 calls the
// library's cos and sin on radians.
#include "common.h"
#include "fused_plan.h"      // RFF_*: the tile sizes; rff_plan
#include "shared_grad.h"

namespace {
template <typename T> struct RffTrig;
template <> struct RffTrig<float> {
    static constexpr double scale = 0.15915494309189533577;      // 1 / (2 pi): the prepared operands are in revolutions
    static __device__ __forceinline__ float cos(float t) { return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(t)); }
    static __device__ __forceinline__ float sin(float t) { return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(t)); }
};
template <> struct RffTrig<double> {
    static constexpr double scale = 1.0;
    static __device__ __forceinline__ double cos(double t) { return ::cos(t); }
    static __device__ __forceinline__ double sin(double t) { return ::sin(t); }
};
}  // namespace
#define MXF_RFF_COS(T, x) RffTrig<T>::cos(x)
#define MXF_RFF_SIN(T, x) RffTrig<T>::sin(x)
#include "rff.h"

namespace {

template <typename T>
struct RffOps {
    int S; int64_t N, D; int Q, J;
    const T* X; int64_t ss_X;
    const T* Omega; int64_t ss_Om;
    const T* phase; int64_t ss_ph;
    const T* W; int64_t ss_W;
};

// the prepared operands of one call: omega padded to QP and the phase, both times RffTrig<T>::scale, and W in blocks of JB columns padded
// with zeros, one block per pass.  Each keeps its operand's sample axis (S or 1).
template <typename T>
struct RffPrep {
    const T* om; int64_t ss_om;     // (S|1, D, QP)
    const T* ph; int64_t ss_ph;     // (S|1, D)
    const T* wb; int64_t ss_wb;     // (S|1, npass, D, JB)
    int npass;
};

template <typename T, int QP, int JB>
__global__ __launch_bounds__(256) void rff_prep_kernel(RffOps<T> o, int npass, T* __restrict__ om, T* __restrict__ ph, T* __restrict__ wb) {
    const int64_t n_om = (o.ss_Om ? o.S : 1) * o.D, n_ph = (o.ss_ph ? o.S : 1) * o.D, n_w = (o.ss_W ? o.S : 1) * npass * o.D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_om + n_ph + n_w; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n_om) {                     // an owned sample axis is dense: row i of (S D, Q)
#pragma unroll
            for (int q = 0; q < QP; ++q) om[i * QP + q] = q < o.Q ? (T)((double)o.Omega[i * o.Q + q] * RffTrig<T>::scale) : (T)0;
        } else if (i < n_om + n_ph) {
            const int64_t k = i - n_om;
            ph[k] = (T)((double)o.phase[k] * RffTrig<T>::scale);
        } else {
            const int64_t k = i - n_om - n_ph, s = k / (npass * o.D), r = k - s * npass * o.D, pass = r / o.D, d = r - pass * o.D;
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const int64_t jj = pass * JB + j;
                wb[k * JB + j] = jj < o.J ? o.W[(s * o.D + d) * o.J + jj] : (T)0;
            }
        }
    }
}

// a thread's own row, padded with zeros; a dead thread reads the last row
template <typename T, int QP>
__device__ __forceinline__ void rff_own_row(const RffOps<T>& o, int64_t s, int64_t n, T* x) {
    const T* px = o.X + s * o.ss_X + n * o.Q;
#pragma unroll
    for (int q = 0; q < QP; ++q) x[q] = q < o.Q ? px[q] : (T)0;
}

// the d of workgroup row blockIdx.y: [d0, d1), chunks of `ch` values (a multiple of RFF_DCH)
__device__ __forceinline__ void rff_d_range(int64_t D, int64_t ch, int64_t& d0, int64_t& d1) {
    d0 = (int64_t)blockIdx.y * ch;
    d1 = d0 + ch < D ? d0 + ch : D;
}

// out[s][n][j] = sum_d cos(.) W[d][j].  With grid.y = 1 a thread writes its row's results (out); otherwise it adds them to the zeroed
// doubles acc (S, N, J), narrowed by mxf_narrow_kernel.
template <typename T, int QP, int JB>
__global__ __launch_bounds__(RFF_RB) void rff_fwd_kernel(RffOps<T> o, RffPrep<T> p, int64_t ch, double* __restrict__ acc, T* __restrict__ out) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * RFF_RB + threadIdx.x;
    const bool live = n < o.N;
    T x[QP];
    rff_own_row<T, QP>(o, s, live ? n : o.N - 1, x);
    int64_t d0, d1;
    rff_d_range(o.D, ch, d0, d1);
    const T *om = p.om + s * p.ss_om, *ph = p.ph + s * p.ss_ph;
    for (int pass = 0; pass < p.npass; ++pass) {
        const T* wb = p.wb + s * p.ss_wb + (int64_t)pass * o.D * JB;
        double R[JB];
#pragma unroll
        for (int j = 0; j < JB; ++j) R[j] = 0;
        for (int64_t db = d0; db < d1; db += RFF_DCH) {
            const int64_t de = db + RFF_DCH < d1 ? db + RFF_DCH : d1;
            T r_[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) r_[j] = 0;
            for (int64_t d = db; d < de; ++d) {         // omega_d, phase_d and the weights are uniform over the wavefront: scalar loads
                const T c = rff_feature<T, QP>(x, om + d * QP, ph[d]);
                const T* w = wb + d * JB;
#pragma unroll
                for (int j = 0; j < JB; ++j) r_[j] += w[j] * c;
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) R[j] += (double)r_[j];
        }
        if (live) {
            const int64_t at = (s * o.N + n) * o.J + (int64_t)pass * JB;
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                if (pass * JB + j < o.J) {
                    if (acc) atomic_add(acc + at + j, R[j]);
                    else out[at + j] = (T)R[j];
                }
            }
        }
    }
}

// dX[s][n][q] += -sum_d sin(.) omega[d][q] sum_j G[s][n][j] W[d][j]: the thread owns dX[n,:], sums every pass and every d of its range in
// registers and ends with one update per coordinate -- its own read-modify-write of dX (dacc null), or an atomic into the doubles dacc
// shaped like X (d split over grid.y, or X shared by S > 1 samples: own_X = 0 and the samples add into the same row).
template <typename T, int QP, int JB>
__global__ __launch_bounds__(RFF_RB) void rff_bwd_kernel(RffOps<T> o, RffPrep<T> p, int64_t ch, const T* __restrict__ G, double* __restrict__ dacc,
                                                         int own_X, T* __restrict__ dX) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * RFF_RB + threadIdx.x;
    const bool live = n < o.N;
    T x[QP];
    rff_own_row<T, QP>(o, s, live ? n : o.N - 1, x);
    int64_t d0, d1;
    rff_d_range(o.D, ch, d0, d1);
    const T *om = p.om + s * p.ss_om, *ph = p.ph + s * p.ss_ph;
    double DX[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) DX[q] = 0;
    for (int pass = 0; pass < p.npass; ++pass) {
        const T* wb = p.wb + s * p.ss_wb + (int64_t)pass * o.D * JB;
        const T* g_row = G + (s * o.N + (live ? n : o.N - 1)) * o.J;
        T g[JB];
#pragma unroll
        for (int j = 0; j < JB; ++j) g[j] = (live && pass * JB + j < o.J) ? g_row[pass * JB + j] : (T)0;
        for (int64_t db = d0; db < d1; db += RFF_DCH) {
            const int64_t de = db + RFF_DCH < d1 ? db + RFF_DCH : d1;
            T dx_[QP];
#pragma unroll
            for (int q = 0; q < QP; ++q) dx_[q] = 0;
            for (int64_t d = db; d < de; ++d) {
                const T* w = wb + d * JB;
                T gw = 0;
#pragma unroll
                for (int j = 0; j < JB; ++j) gw += g[j] * w[j];
                rff_feature_bwd<T, QP>(x, om + d * QP, ph[d], gw, dx_);
            }
#pragma unroll
            for (int q = 0; q < QP; ++q) DX[q] += (double)dx_[q];
        }
    }
    if (!live) return;
    const int64_t at = ((own_X ? s : 0) * o.N + n) * o.Q;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        if (q < o.Q) {
            const double v = -DX[q] / RffTrig<T>::scale;        // (the prepared omega carries the scale)
            if (dacc) atomic_add(dacc + at + q, v);
            else dX[at + q] = (T)((double)dX[at + q] + v);
        }
    }
}

struct RffArgs {
    int dtype = MXF_F32, S = 0; int64_t N = 0, D = 0; int Q = 0, J = 0;
    const void *X = nullptr, *Omega = nullptr, *phase = nullptr, *W = nullptr; int64_t ss_X = 0, ss_Om = 0, ss_ph = 0, ss_W = 0;
    void* out = nullptr;                                // forward
    const void* G = nullptr; void* dX = nullptr;        // reverse
};

// ask the plan (fused_plan.h: rff_plan), carve, launch
template <typename T, int QP, int JB>
int rff_launch(mxf_handle h, const char* name, const RffArgs& a, const RffPlan& p, bool bwd, hipStream_t st) {
    const RffOps<T> o = {a.S, a.N, a.D, a.Q, a.J, (const T*)a.X, a.ss_X, (const T*)a.Omega, a.ss_Om, (const T*)a.phase, a.ss_ph, (const T*)a.W, a.ss_W};
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    double* acc = p.scratch_sum ? (double*)(ws + p.at_acc) : nullptr;
    if (acc) MXF_HIP(h, hipMemsetAsync(acc, 0, p.zero_bytes, st));
    T *om = (T*)(ws + p.at_om), *ph = (T*)(ws + p.at_ph), *wb = (T*)(ws + p.at_wb);
    hipLaunchKernelGGL((rff_prep_kernel<T, QP, JB>), dim3(grid_for(p.n_prep)), dim3(256), 0, st, o, p.npass, om, ph, wb);
    const RffPrep<T> prep = {om, p.ss_om, ph, p.ss_ph, wb, p.ss_wb, p.npass};
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    if (!bwd) {
        hipLaunchKernelGGL((rff_fwd_kernel<T, QP, JB>), grid, dim3(RFF_RB), 0, st, o, prep, p.ch, acc, (T*)a.out);
        if (acc) hipLaunchKernelGGL((mxf_narrow_kernel<T>), dim3(grid_for(p.n_out)), dim3(256), 0, st, p.n_out, acc, (T*)a.out);
    } else {
        double* dacc = !p.summed ? nullptr : (acc ? acc : (double*)a.dX);
        hipLaunchKernelGGL((rff_bwd_kernel<T, QP, JB>), grid, dim3(RFF_RB), 0, st, o, prep, p.ch, (const T*)a.G, dacc, p.own_X, (T*)a.dX);
        if (acc) {
            const FoldTable f = {acc, {(float*)a.dX, nullptr, nullptr}, {p.n_dx, p.n_dx, p.n_dx}};
            hipLaunchKernelGGL(mxf_fold_kernel, dim3(grid_for(p.n_dx)), dim3(256), 0, st, f);
        }
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

int run(mxf_handle h, const char* name, const RffArgs& a, bool bwd, void* stream) {
    if (!h) return -1;
    if (a.dtype != MXF_F32 && a.dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, a.dtype);
    const RffPlan p = rff_plan({.esize = mxf_esize(a.dtype), .bwd = bwd, .S = a.S, .N = a.N, .D = a.D, .Q = a.Q, .J = a.J,
                                .ss_X = a.ss_X, .ss_Om = a.ss_Om, .ss_ph = a.ss_ph, .ss_W = a.ss_W,
                                .has_X = a.X != nullptr, .has_Om = a.Omega != nullptr, .has_ph = a.phase != nullptr, .has_W = a.W != nullptr,
                                .has_out = a.out != nullptr, .has_G = a.G != nullptr, .has_dX = a.dX != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    return dispatch<MXF_F32, MXF_F64>(a.dtype, [&](auto dt) {
        return dispatch<4, 8, 16>(p.qp, [&](auto qp) {
            return dispatch<RFF_JB_SMALL, RFF_JB>(p.jb, [&](auto jb) {
                return rff_launch<mxf_elem_t<decltype(dt)::value>, decltype(qp)::value, decltype(jb)::value>(h, name, a, p, bwd, (hipStream_t)stream);
            });
        });
    });
}

}  // namespace

extern "C" int mxf_rff_eval(mxf_handle h, int dtype, int S, int64_t N, int64_t D, int Q, int J, const void* X, int64_t strideS_X, const void* Omega,
                            int64_t strideS_Om, const void* phase, int64_t strideS_ph, const void* W, int64_t strideS_W, void* out, void* stream) {
    const RffArgs a = {.dtype = dtype, .S = S, .N = N, .D = D, .Q = Q, .J = J, .X = X, .Omega = Omega, .phase = phase, .W = W,
                       .ss_X = strideS_X, .ss_Om = strideS_Om, .ss_ph = strideS_ph, .ss_W = strideS_W, .out = out};
    return run(h, "mxf_rff_eval", a, false, stream);
}

extern "C" int mxf_rff_eval_bwd(mxf_handle h, int dtype, int S, int64_t N, int64_t D, int Q, int J, const void* X, int64_t strideS_X, const void* Omega,
                                int64_t strideS_Om, const void* phase, int64_t strideS_ph, const void* W, int64_t strideS_W, const void* G, void* dX_acc,
                                void* stream) {
    const RffArgs a = {.dtype = dtype, .S = S, .N = N, .D = D, .Q = Q, .J = J, .X = X, .Omega = Omega, .phase = phase, .W = W,
                       .ss_X = strideS_X, .ss_Om = strideS_Om, .ss_ph = strideS_ph, .ss_W = strideS_W, .G = G, .dX = dX_acc};
    return run(h, "mxf_rff_eval_bwd", a, true, stream);
}
