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

constexpr int RFF_RB = 128;         // rows (threads) per workgroup
constexpr int RFF_DCH = 64;         // values of d summed in T between two additions to the double register
constexpr int RFF_JB = 16;          // weights per feature and pass (one scalar load)
constexpr int RFF_JB_SMALL = 4;     // the same for J <= RFF_JB_SMALL
constexpr int RFF_TARGET = 1024;    // workgroups the split of d aims for

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
// doubles acc (S, N, J), narrowed by rff_narrow_kernel.
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

template <typename T>
__global__ __launch_bounds__(256) void rff_narrow_kernel(int64_t total, const double* __restrict__ acc, T* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) out[i] = (T)acc[i];
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

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t clampi(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

struct RffArgs {
    int dtype, S; int64_t N, D; int Q, J;
    const void *X, *Omega, *phase, *W; int64_t ss_X, ss_Om, ss_ph, ss_W;
    void* out;                      // forward
    const void* G; void* dX;        // reverse
};

struct RffScratch {
    size_t bytes = 0;
    size_t take(size_t b) { const size_t at = bytes; bytes += mxf_align(b); return at; }
};

// the values of d per workgroup row (a multiple of RFF_DCH) and the number of such rows: 1 unless the row blocks alone leave the device empty
static inline void rff_split(int S, int64_t N, int64_t D, int64_t* ch, int* dch) {
    const int64_t want = clampi(cdiv(RFF_TARGET, cdiv(N, RFF_RB) * S), 1, clampi(cdiv(D, RFF_DCH), 1, 65535));
    *ch = cdiv(cdiv(D, want), RFF_DCH) * RFF_DCH;
    *dch = (int)cdiv(D, *ch);
}

template <typename T, int QP, int JB>
int rff_run(mxf_handle h, const char* name, const RffArgs& a, bool bwd, hipStream_t st) {
    const RffOps<T> o = {a.S, a.N, a.D, a.Q, a.J, (const T*)a.X, a.ss_X, (const T*)a.Omega, a.ss_Om, (const T*)a.phase, a.ss_ph, (const T*)a.W, a.ss_W};
    const int npass = (int)cdiv(a.J, JB), own_X = a.ss_X != 0;
    const int64_t S_om = a.ss_Om ? a.S : 1, S_ph = a.ss_ph ? a.S : 1, S_W = a.ss_W ? a.S : 1;
    int64_t ch;
    int dch;
    rff_split(a.S, a.N, a.D, &ch, &dch);
    // what is summed across threads goes through doubles: the forward results under a split of d; the gradient under a split or a shared X
    const int64_t n_out = (int64_t)a.S * a.N * a.J, n_dx = (own_X ? a.S : 1) * a.N * a.Q;
    const bool summed = bwd ? (dch > 1 || (!own_X && a.S > 1)) : dch > 1;
    const bool scratch_sum = summed && !(bwd && sizeof(T) == 8);         // a float64 gradient is summed in the caller's buffer itself
    RffScratch sc;
    const size_t at_om = sc.take((size_t)(S_om * a.D) * QP * sizeof(T)), at_ph = sc.take((size_t)(S_ph * a.D) * sizeof(T));
    const size_t at_wb = sc.take((size_t)(S_W * npass * a.D) * JB * sizeof(T));
    const size_t n_acc = scratch_sum ? (size_t)(bwd ? n_dx : n_out) : 0, at_acc = sc.take(n_acc * sizeof(double));
    char* ws = (char*)mxf_ws(h, sc.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, sc.bytes);
    double* acc = scratch_sum ? (double*)(ws + at_acc) : nullptr;
    if (acc) MXF_HIP(h, hipMemsetAsync(acc, 0, n_acc * sizeof(double), st));
    T *om = (T*)(ws + at_om), *ph = (T*)(ws + at_ph), *wb = (T*)(ws + at_wb);
    hipLaunchKernelGGL((rff_prep_kernel<T, QP, JB>), dim3(grid_for((S_om + S_ph + S_W * npass) * a.D)), dim3(256), 0, st, o, npass, om, ph, wb);
    const RffPrep<T> p = {om, a.ss_Om ? a.D * QP : 0, ph, a.ss_ph ? a.D : 0, wb, a.ss_W ? (int64_t)npass * a.D * JB : 0, npass};
    const dim3 grid((unsigned)cdiv(a.N, RFF_RB), (unsigned)dch, (unsigned)a.S);
    if (!bwd) {
        hipLaunchKernelGGL((rff_fwd_kernel<T, QP, JB>), grid, dim3(RFF_RB), 0, st, o, p, ch, acc, (T*)a.out);
        if (acc) hipLaunchKernelGGL((rff_narrow_kernel<T>), dim3(grid_for(n_out)), dim3(256), 0, st, n_out, acc, (T*)a.out);
    } else {
        double* dacc = !summed ? nullptr : (acc ? acc : (double*)a.dX);
        hipLaunchKernelGGL((rff_bwd_kernel<T, QP, JB>), grid, dim3(RFF_RB), 0, st, o, p, ch, (const T*)a.G, dacc, own_X, (T*)a.dX);
        if (acc) {
            const FoldTable f = {acc, {(float*)a.dX, nullptr, nullptr}, {n_dx, n_dx, n_dx}};
            hipLaunchKernelGGL(mxf_fold_kernel, dim3(grid_for(n_dx)), dim3(256), 0, st, f);
        }
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

int run(mxf_handle h, const char* name, const RffArgs& a, bool bwd, void* stream) {
    if (!h) return -1;
    if (a.dtype != MXF_F32 && a.dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, a.dtype);
    if (a.S < 1 || a.S > 65535 || a.N < 1 || a.D < 1 || a.Q < 1 || a.J < 1) MXF_FAIL(h, -2, "%s: 1 <= S <= 65535 samples, N, D, Q, J >= 1", name);
    if (a.Q > MXF_RFF_MAX_Q) MXF_FAIL(h, -3, "%s: Q = %d above the limit of %d input dimensions", name, a.Q, MXF_RFF_MAX_Q);
    if (a.N > ((int64_t)1 << 31) || a.D > ((int64_t)1 << 24) || a.J > (1 << 16)) MXF_FAIL(h, -2, "%s: N <= 2^31, D <= 2^24, J <= 2^16", name);
    if (!a.X || !a.Omega || !a.phase || !a.W) MXF_FAIL(h, -2, "%s: null X, Omega, phase or W", name);
    if (bwd ? (!a.G || !a.dX) : !a.out) MXF_FAIL(h, -2, "%s: null %s", name, bwd ? "G or dX_acc" : "out");
    if ((a.ss_X != 0 && a.ss_X != a.N * a.Q) || (a.ss_Om != 0 && a.ss_Om != a.D * a.Q) || (a.ss_ph != 0 && a.ss_ph != a.D) ||
        (a.ss_W != 0 && a.ss_W != a.D * a.J))
        MXF_FAIL(h, -2, "%s: a sample stride must be 0 or the elements of one sample (X: N Q; Omega: D Q; phase: D; W: D J)", name);
    const hipStream_t st = (hipStream_t)stream;
    const int qp = a.Q <= 4 ? 4 : (a.Q <= 8 ? 8 : 16);
    const bool small = a.J <= RFF_JB_SMALL;
#define MXF_RFF_JB(T, QP) (small ? rff_run<T, QP, RFF_JB_SMALL>(h, name, a, bwd, st) : rff_run<T, QP, RFF_JB>(h, name, a, bwd, st))
#define MXF_RFF_GO(T) (qp == 4 ? MXF_RFF_JB(T, 4) : qp == 8 ? MXF_RFF_JB(T, 8) : MXF_RFF_JB(T, 16))
    return a.dtype == MXF_F32 ? MXF_RFF_GO(float) : MXF_RFF_GO(double);
#undef MXF_RFF_GO
#undef MXF_RFF_JB
}

}  // namespace

extern "C" int mxf_rff_eval(mxf_handle h, int dtype, int S, int64_t N, int64_t D, int Q, int J, const void* X, int64_t strideS_X, const void* Omega,
                            int64_t strideS_Om, const void* phase, int64_t strideS_ph, const void* W, int64_t strideS_W, void* out, void* stream) {
    RffArgs a = {dtype, S, N, D, Q, J, X, Omega, phase, W, strideS_X, strideS_Om, strideS_ph, strideS_W};
    a.out = out;
    return run(h, "mxf_rff_eval", a, false, stream);
}

extern "C" int mxf_rff_eval_bwd(mxf_handle h, int dtype, int S, int64_t N, int64_t D, int Q, int J, const void* X, int64_t strideS_X, const void* Omega,
                                int64_t strideS_Om, const void* phase, int64_t strideS_ph, const void* W, int64_t strideS_W, const void* G, void* dX_acc,
                                void* stream) {
    RffArgs a = {dtype, S, N, D, Q, J, X, Omega, phase, W, strideS_X, strideS_Om, strideS_ph, strideS_W};
    a.G = G;
    a.dX = dX_acc;
    return run(h, "mxf_rff_eval_bwd", a, true, stream);
}
