// What the row-owned kernels of the matrix-free kernel product share (kmv.hip: the product and its reverse mode in the kernel parameters;
// kmv_bwd_x.hip: its reverse mode in the inputs): the operands, the two kernels that prepare the streamed operands, a thread's own row and
// the range of n2 of a workgroup row.  Internal linkage: each of the two files compiles its own copy.
#pragma once
#include "common.h"
#include "fused_plan.h"      // KMV_*: the tile sizes
#include "kmv.h"

namespace {

template <typename T>
struct KmvOps {
    int S; int64_t N, N2; int Q, J, ard, square;
    const T* X; int64_t ss_X;
    const T* Z; int64_t ss_Z;       // the second operand: X2, or X itself for a square product
    const T* C; int64_t ss_C;       // the centre, the first row of X2 (of X, square): Z, but for the X2 side of the reverse mode in the inputs
    const T* ls; int64_t ss_ls;
    const T* var; int64_t ss_var;
    const T* da; int64_t ss_da;     // diag_add, or null
    const T* V; int64_t ss_V;
};

struct KmvWeights { double w[KMV_WG]; int use; };

// coordinate q of a row of X or X2 as the kernels subtract them: centred on the first row of X2 (o.C), times c / l_q; 0 for q >= Q
template <typename T, int KIND>
__device__ __forceinline__ T kmv_coord(const KmvOps<T>& o, int64_t s, const T* row, int q) {
    if (q >= o.Q) return (T)0;
    const T m = coord_scale<T, KIND>() / o.ls[s * o.ss_ls + (o.ard ? q : 0)];
    return (row[q] - o.C[s * o.ss_C + q]) * m;
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
}  // namespace
