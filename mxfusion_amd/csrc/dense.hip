// A dense neural-network layer that carries the sample axis (gfx950): Y[s,n,:] = act(X[s,n,:] W[s]^T + b[s]) for all S samples in one
// launch, bias and activation fused, and its reverse mode in one launch -- the layer of a network whose weights are random variables
// (S draws of W) or shared parameters (sample stride 0).  Widths 1 <= I, O <= 128.
//   A workgroup of 256 threads owns a tile of TN rows (32 for float, 16 for double) of one sample.
//   Forward: the X tile [TN][I] is staged in LDS once; the weights pass through LDS in chunks of 32 output columns, transposed to
//   [i][column] with a row padded to 33 (conflict-free both for the staging writes, consecutive i, and for the reads, consecutive columns):
//   every element of W[s] and b[s] is fetched once per workgroup.  Thread (tx = column, ty) sums over i for TN / 8 rows in registers.
//   Reverse: G = dY act'(Y) [TN][O] and the X tile are staged; db and dW are sums over the tile's rows of G and of G^T X, one element per
//   thread and trip, added with atomics to a DOUBLE accumulator (shared_grad.h): the sum over the row tiles, and over s where W or b is shared, is formed in double for either
//   dtype.  dX = G W[s] takes W through LDS in chunks of 16 rows; thread (i, half) holds TN / 2 rows.  Where X is shared over the samples
//   a workgroup loops over s itself and sums its dX in double registers: one plain += per element.
// Plain FMAs for both dtypes (the layer is paced by its launch, not by its arithmetic).
//
// Replaces: the per-sample loop of FunctionEvaluation.eval over a Gluon Dense block (components/functions/function_evaluation.py:77-96:
// FullyConnected + Activation per sample, concat) and MXNet autograd through it.
#include "common.h"
#include "shared_grad.h"

namespace {

constexpr int FWD_OC = 32;          // forward: output columns per chunk of W
constexpr int BWD_OC = 16;          // reverse: rows of W per chunk

template <typename T> struct DenseTile { static constexpr int rows = 32; };
template <> struct DenseTile<double> { static constexpr int rows = 16; };

template <typename T>
struct DenseArgs {
    int S;
    int64_t N;
    int I, O, act;
    const T* X; int64_t ldx, ss_x;
    const T* W; int64_t ss_w;
    const T* b; int64_t ss_b;
    int64_t tiles;
};

template <typename T>
__device__ __forceinline__ T dense_act(int act, T z) {
    switch (act) {
        case 1: return tanh(z);
        case 2: return z > (T)0 ? z : (T)0;
        case 3: return (T)1 / ((T)1 + exp(-z));
        default: return z;
    }
}

// act'(z) as a function of y = act(z)
template <typename T>
__device__ __forceinline__ T dense_dact(int act, T y) {
    switch (act) {
        case 1: return (T)1 - y * y;
        case 2: return y > (T)0 ? (T)1 : (T)0;
        case 3: return y * ((T)1 - y);
        default: return (T)1;
    }
}

// rows n0 .. n0 + TN - 1 of X[s] into Xs[TN][I]; rows past N are zero
template <typename T, int TN>
__device__ __forceinline__ void stage_x(const DenseArgs<T>& a, int64_t s, int64_t n0, T* Xs) {
    const T* Xp = a.X + s * a.ss_x;
    for (int idx = threadIdx.x; idx < TN * a.I; idx += 256) {
        const int r = idx / a.I, i = idx - r * a.I;
        Xs[idx] = n0 + r < a.N ? Xp[(n0 + r) * a.ldx + i] : (T)0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dense_fwd_kernel(DenseArgs<T> a, T* __restrict__ Y) {
    constexpr int TN = DenseTile<T>::rows, R = TN / 8;
    __shared__ T Xs[TN * DENSE_MAX];
    __shared__ T Ws[DENSE_MAX * (FWD_OC + 1)];
    const int64_t s = blockIdx.x / a.tiles, n0 = (blockIdx.x % a.tiles) * TN;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    stage_x<T, TN>(a, s, n0, Xs);
    const T* Wp = a.W + s * a.ss_w;
    for (int oc0 = 0; oc0 < a.O; oc0 += FWD_OC) {
        const int ocn = min(FWD_OC, a.O - oc0);
        if (oc0) __syncthreads();
        for (int idx = threadIdx.x; idx < ocn * a.I; idx += 256) {
            const int o = idx / a.I, i = idx - o * a.I;
            Ws[i * (FWD_OC + 1) + o] = Wp[(int64_t)(oc0 + o) * a.I + i];
        }
        __syncthreads();
        const int o = oc0 + tx;
        if (o < a.O) {
            T acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = 0;
            for (int i = 0; i < a.I; ++i) {
                const T w = Ws[i * (FWD_OC + 1) + tx];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fma(Xs[(ty + 8 * r) * a.I + i], w, acc[r]);
            }
            const T bias = a.b ? a.b[s * a.ss_b + o] : (T)0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t n = n0 + ty + 8 * r;
                if (n < a.N) Y[(s * a.N + n) * a.O + o] = dense_act(a.act, acc[r] + bias);
            }
        }
    }
}

// The gradients' indices come from shared_row (shared_grad.h), whose rows are (s, b): dX (S|1, N, I) takes the data row n as b with B = N;
// dW (S|1, O, I) and db (S|1, O) have the sample axis alone, b = 0 of B = 1, and the whole per-sample block as their row.
// by_rows: X is shared over the samples and dX is wanted: the workgroup owns a row tile and loops over s.  sW, sB: double accumulators
// laid out as dW (S|1, O, I) and db (S|1, O).
template <typename T>
__global__ __launch_bounds__(256) void dense_bwd_kernel(DenseArgs<T> a, const T* __restrict__ Y, const T* __restrict__ dY, T* dX, double* sW,
                                                        double* sB, int by_rows) {
    constexpr int TN = DenseTile<T>::rows, RX = TN / 2;
    __shared__ T Gs[TN * DENSE_MAX];
    __shared__ T Xs[TN * DENSE_MAX];
    __shared__ T Ws[BWD_OC * DENSE_MAX];
    const int64_t s0 = by_rows ? 0 : blockIdx.x / a.tiles, n0 = (by_rows ? blockIdx.x : blockIdx.x % a.tiles) * TN;
    const int ns = by_rows ? a.S : 1;
    const int xi = threadIdx.x & 127, half = threadIdx.x >> 7;
    if (sW) stage_x<T, TN>(a, s0, n0, Xs);
    double tot[RX];
#pragma unroll
    for (int r = 0; r < RX; ++r) tot[r] = 0.0;
    for (int64_t s = s0; s < s0 + ns; ++s) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < TN * a.O; idx += 256) {
            const int r = idx / a.O, o = idx - r * a.O;
            T g = 0;
            if (n0 + r < a.N) {
                const int64_t at = (s * a.N + n0 + r) * a.O + o;
                g = dY[at] * dense_dact(a.act, Y[at]);
            }
            Gs[idx] = g;
        }
        __syncthreads();
        if (sB)
            for (int o = threadIdx.x; o < a.O; o += 256) {
                T v = 0;
                for (int r = 0; r < TN; ++r) v += Gs[r * a.O + o];
                atomic_add(sB + shared_row(a.ss_b, true, s, 0, 1, a.O) + o, (double)v);
            }
        if (sW)
            for (int idx = threadIdx.x; idx < a.O * a.I; idx += 256) {
                const int o = idx / a.I, i = idx - o * a.I;
                T v = 0;
                for (int r = 0; r < TN; ++r) v = fma(Gs[r * a.O + o], Xs[r * a.I + i], v);
                atomic_add(sW + shared_row(a.ss_w, true, s, 0, 1, (int64_t)a.O * a.I) + idx, (double)v);
            }
        if (dX) {
            T acc[RX];
#pragma unroll
            for (int r = 0; r < RX; ++r) acc[r] = 0;
            const T* Wp = a.W + s * a.ss_w;
            for (int oc0 = 0; oc0 < a.O; oc0 += BWD_OC) {
                const int ocn = min(BWD_OC, a.O - oc0);
                if (oc0) __syncthreads();
                for (int idx = threadIdx.x; idx < ocn * a.I; idx += 256) Ws[idx] = Wp[(int64_t)oc0 * a.I + idx];
                __syncthreads();
                if (xi < a.I)
                    for (int o = 0; o < ocn; ++o) {
                        const T w = Ws[o * a.I + xi];
#pragma unroll
                        for (int r = 0; r < RX; ++r) acc[r] = fma(Gs[(half + 2 * r) * a.O + oc0 + o], w, acc[r]);
                    }
            }
            if (xi < a.I) {
#pragma unroll
                for (int r = 0; r < RX; ++r) {
                    const int64_t n = n0 + half + 2 * r;
                    if (by_rows) tot[r] += (double)acc[r];
                    else if (n < a.N) dX[shared_row(a.ss_x, true, s, n, a.N, a.I) + xi] += acc[r];
                }
            }
        }
    }
    if (dX && by_rows && xi < a.I) {
#pragma unroll
        for (int r = 0; r < RX; ++r) {
            const int64_t n = n0 + half + 2 * r;
            if (n < a.N) dX[n * a.I + xi] += (T)tot[r];
        }
    }
}

struct DenseCall {
    const char* name;
    int dtype, S; int64_t N; int I, O, act;
    const void* X; int64_t ldx, ss_x;
    const void* W; int64_t ss_w;
    const void* b; int64_t ss_b;
    const void* Y;                  // the output of the forward pass, an operand of the reverse pass
    const void* dY; void *dX, *dW, *db;
};

template <typename T>
int launch(mxf_handle h, const DenseCall& c, const DensePlan& p, bool bwd, hipStream_t st) {
    static_assert(DenseTile<float>::rows == 32 && DenseTile<double>::rows == 16, "dense_tile_rows (pointwise_plan.h) holds the tile heights");
    const DenseArgs<T> a = {.S = c.S, .N = c.N, .I = c.I, .O = c.O, .act = c.act, .X = (const T*)c.X, .ldx = c.ldx, .ss_x = c.ss_x, .W = (const T*)c.W,
                            .ss_w = c.ss_w, .b = (const T*)c.b, .ss_b = c.ss_b, .tiles = p.tiles};
    if (!bwd) {
        hipLaunchKernelGGL(dense_fwd_kernel<T>, dim3(p.grid), dim3(256), 0, st, a, (T*)c.Y);
        return 0;
    }
    SharedSums sums;          // dW and db are sums over the row tiles: in double whenever they are wanted, shared over s or not
    if (int rc = shared_sums_open<T>(h, c.name, {{c.dW, p.n_dw}, {c.db, p.n_db}}, st, &sums)) return rc;
    hipLaunchKernelGGL(dense_bwd_kernel<T>, dim3(p.grid), dim3(256), 0, st, a, (const T*)c.Y, (const T*)c.dY, (T*)c.dX, sums.acc[0], sums.acc[1], p.by_rows ? 1 : 0);
    shared_sums_close(sums, st);
    return 0;
}

int run(mxf_handle h, const DenseCall& c, bool bwd, void* stream) {
    if (!h) return -1;
    const DensePlan p = dense_plan({.dtype = c.dtype, .bwd = bwd, .S = c.S, .N = c.N, .I = c.I, .O = c.O, .act = c.act, .ldx = c.ldx, .ss_x = c.ss_x,
                                    .ss_w = c.ss_w, .ss_b = c.ss_b, .has_X = c.X != nullptr, .has_W = c.W != nullptr, .has_Y = c.Y != nullptr,
                                    .has_dY = c.dY != nullptr, .has_dX = c.dX != nullptr, .has_dW = c.dW != nullptr, .has_db = c.db != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", c.name, p.refusal);
    if (p.empty) return 0;
    return mxf_typed(h, c.name, c.dtype, [&](auto t) { return launch<decltype(t)>(h, c, p, bwd, (hipStream_t)stream); });
}

}  // namespace

extern "C" int mxf_dense_fwd(mxf_handle h, int dtype, int S, int64_t N, int I, int O, int act, const void* X, int64_t ldx, int64_t strideS_x,
                             const void* W, int64_t strideS_w, const void* b, int64_t strideS_b, void* Y, void* stream) {
    const DenseCall c = {.name = "mxf_dense_fwd", .dtype = dtype, .S = S, .N = N, .I = I, .O = O, .act = act, .X = X, .ldx = ldx, .ss_x = strideS_x,
                         .W = W, .ss_w = strideS_w, .b = b, .ss_b = b ? strideS_b : 0, .Y = Y};
    return run(h, c, false, stream);
}

extern "C" int mxf_dense_bwd(mxf_handle h, int dtype, int S, int64_t N, int I, int O, int act, const void* X, int64_t ldx, int64_t strideS_x,
                             const void* W, int64_t strideS_w, int64_t strideS_b, const void* Y, const void* dY, void* dX_acc, void* dW_acc,
                             void* db_acc, void* stream) {
    const DenseCall c = {.name = "mxf_dense_bwd", .dtype = dtype, .S = S, .N = N, .I = I, .O = O, .act = act, .X = X, .ldx = ldx, .ss_x = strideS_x,
                         .W = W, .ss_w = strideS_w, .ss_b = strideS_b, .Y = Y, .dY = dY, .dX = dX_acc, .dW = dW_acc, .db = db_acc};
    return run(h, c, true, stream);
}
