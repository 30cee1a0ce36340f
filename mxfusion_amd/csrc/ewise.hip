// The model operators' arithmetic (gfx950): one broadcast map z = op(x, y) over up to MXF_EW_MAX_RANK merged axes, the sample axis included,
// for all samples in one launch, its reverse mode in one launch, and the reductions sum / mean / prod behind the sample axis.
//   Map.  The output is dense row-major over `extent`; a work item is one 16-byte chunk (4 floats, 2 doubles) of one innermost row, and the
//   256-thread workgroups walk the items in a grid-stride loop.  An item's outer coordinates are peeled off its row number with 32-bit
//   divisions where the item count allows it (a rank-1 call, the fully merged same-shape case, divides nothing).  Each operand's chunk is one
//   16-byte load where its innermost stride is 1 and the chunk is whole and aligned, ONE scalar load where the innermost axis shares it
//   (stride 0), and strided scalar loads otherwise (tails, odd starts, transposed views); the store is chosen the same way.
//   Reverse.  An operand without a shared axis gets plain read-modify-write stores, dense like the output.  The gradient of an operand
//   with a shared axis is its sum over those axes, formed in DOUBLE for either dtype (shared_grad.h).  Before any atomic leaves a workgroup
//   the terms of one destination are pre-reduced three times over: where the innermost axis is shared a thread sums its chunk and a
//   segmented wave shuffle sums the lanes that hold the same destination; a thread keeps the running sum of the destination it last saw
//   across its grid-stride trips and lets go of it only when the destination changes; and a gradient of up to EW_TAB elements is summed
//   in an LDS table of the workgroup, which ends in one atomic per non-zero entry.  A one-element operand under 10^6 terms costs one atomic
//   per workgroup, 512 at the most.
//   exp, log and pow are the device library's accurate functions, never the fast intrinsics.
//
// Replaces: the operators of components/functions/operators/operator_impl.py:27-85 evaluated once per sample in the Python loop of
// FunctionEvaluation.eval (components/functions/function_evaluation.py:72-96), and MXNet autograd through them.
#include "common.h"
#include "shared_grad.h"

namespace {

constexpr int EW_TAB = 1024;                          // LDS sums per operand (doubles)

struct EwArgs : EwAxes {};                            // (pointwise_plan.h: rank, op, extents, operand and gradient strides)

template <typename T>
__device__ __forceinline__ T ew_apply(int op, T x, T y) {
    switch (op) {
        case 0: return x + y;
        case 1: return x - y;
        case 2: return x * y;
        case 3: return x / y;
        case 4: return pow(x, y);
        case 5: return x * x;
        case 6: return exp(x);
        default: return log(x);
    }
}

// dz -> (dx, dy)
template <typename T>
__device__ __forceinline__ void ew_grad(int op, T x, T y, T dz, bool want_y, T* gx, T* gy) {
    *gy = 0;
    switch (op) {
        case 0: *gx = dz; *gy = dz; break;
        case 1: *gx = dz; *gy = -dz; break;
        case 2: *gx = dz * y; *gy = dz * x; break;
        case 3: *gx = dz / y; *gy = -dz * x / (y * y); break;
        case 4: *gx = dz * y * pow(x, y - (T)1); if (want_y) *gy = dz * pow(x, y) * log(x); break;
        case 5: *gx = (T)2 * x * dz; break;
        case 6: *gx = dz * exp(x); break;
        default: *gx = dz / x; break;
    }
}

__device__ __forceinline__ bool ew_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// n <= V elements from p; lanes past n hold 1 (harmless under every op)
template <typename T>
__device__ __forceinline__ void ew_load(const T* p, int64_t stride, int n, T* v) {
    constexpr int V = Vec16<T>::n;
    if (stride == 0) {
        const T s = *p;
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = s;
    } else if (stride == 1 && n == V && ew_aligned(p)) {
        const typename Vec16<T>::type q = *(const typename Vec16<T>::type*)p;
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = q[i];
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = i < n ? p[i * stride] : (T)1;
    }
}

// p[0 .. n) = v (add = false) or += v
template <typename T, bool ADD>
__device__ __forceinline__ void ew_store(T* p, int n, const T* v) {
    constexpr int V = Vec16<T>::n;
    if (n == V && ew_aligned(p)) {
        typename Vec16<T>::type q;
        if (ADD) q = *(typename Vec16<T>::type*)p;
#pragma unroll
        for (int i = 0; i < V; ++i) q[i] = ADD ? q[i] + v[i] : v[i];
        *(typename Vec16<T>::type*)p = q;
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (i < n) p[i] = ADD ? p[i] + v[i] : v[i];
    }
}

// the item's place: row number -> the offsets of the row's first element in x, y and the two gradients; returns nothing for rank 1
template <typename IDX>
__device__ __forceinline__ void ew_place(const EwArgs& a, IDX row, int64_t* ox, int64_t* oy, int64_t* ogx, int64_t* ogy) {
    int64_t x = 0, y = 0, gx = 0, gy = 0;
#pragma unroll
    for (int d = EW_RANK - 2; d >= 0; --d)
        if (d < a.rank - 1) {
            const IDX e = (IDX)a.extent[d], q = row / e, c = row - q * e;
            row = q;
            x += (int64_t)c * a.sx[d];
            y += (int64_t)c * a.sy[d];
            gx += (int64_t)c * a.gx[d];
            gy += (int64_t)c * a.gy[d];
        }
    *ox = x; *oy = y; *ogx = gx; *ogy = gy;
}

template <typename T, typename IDX>
__global__ __launch_bounds__(256) void ewise_fwd_kernel(EwArgs a, const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ z,
                                                        IDX items, IDX chunks) {
    constexpr int V = Vec16<T>::n;
    const int last = a.rank - 1;
    const int64_t inner = a.extent[last];
    for (IDX it = (IDX)blockIdx.x * 256 + threadIdx.x; it < items; it += (IDX)gridDim.x * 256) {
        const IDX row = a.rank > 1 ? it / chunks : 0, c = it - row * chunks;
        const int64_t e0 = (int64_t)c * V;
        const int n = (int)(inner - e0 < V ? inner - e0 : V);
        int64_t ox, oy, ogx, ogy;
        ew_place<IDX>(a, row, &ox, &oy, &ogx, &ogy);
        T vx[V], vy[V], vz[V];
        ew_load(x + ox + e0 * a.sx[last], a.sx[last], n, vx);
        if (y) ew_load(y + oy + e0 * a.sy[last], a.sy[last], n, vy);
#pragma unroll
        for (int i = 0; i < V; ++i) vz[i] = ew_apply(a.op, vx[i], y ? vy[i] : (T)0);
        ew_store<T, false>(z + (int64_t)row * inner + e0, n, vz);
    }
}

// The sum of v over each run of CONSECUTIVE lanes that hold the same key; valid in the run's first lane (*head).  A key may come back later
// in the wave (a shared axis outside a dense one: the destinations repeat with the rows), so lanes are matched by their run -- the lane
// its run starts at -- never by the key itself: a partner `off` lanes on belongs to this lane's run only if every lane between does.
__device__ __forceinline__ double ew_segment_sum(double v, long long key, bool* head) {
    const int lane = threadIdx.x & 63;
    const long long before = __shfl_up(key, 1, 64);
    *head = lane == 0 || before != key;
    const unsigned long long heads = __ballot(*head);                                  // bit l: lane l starts a run; bit 0 is always set
    const int run = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));         // the nearest run start at or below this lane
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ov = __shfl_down(v, off, 64);
        const int orun = __shfl_down(run, off, 64);
        if (lane + off < 64 && orun == run) v += ov;
    }
    return v;
}

// The running sums a thread holds for the destination it last saw (W values from `key` on) of one shared operand's gradient.
template <int V>
struct EwHold {
    long long key = -1;
    double v[V];
};

template <int V>
__device__ __forceinline__ void ew_release(const EwHold<V>& h, int width, double* acc, double* tab) {
    if (h.key < 0) return;
#pragma unroll
    for (int i = 0; i < V; ++i)
        if (i < width && h.v[i] != 0.0) {
            if (tab) lds_add(tab + h.key + i, h.v[i]);
            else atomic_add(acc + h.key + i, h.v[i]);
        }
}

// One item's terms g[0 .. n) for a shared operand.  inner_shared: they all belong to the element at `at`, and so may the neighbouring lanes';
// otherwise to the n elements from `at` on.  Every lane of the wave calls this (valid or not): it shuffles.
template <typename T, int V>
__device__ __forceinline__ void ew_collect(EwHold<V>& h, bool valid, bool inner_shared, long long at, int n, const T* g, double* acc, double* tab) {
    if (inner_shared) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (valid && i < n) s += (double)g[i];
        bool head;
        s = ew_segment_sum(s, valid ? at : -1, &head);
        if (!valid || !head) return;
        if (h.key == at) {
            h.v[0] += s;
            return;
        }
        ew_release<V>(h, 1, acc, tab);
        h.key = at;
        h.v[0] = s;
        return;
    }
    if (!valid) return;
    if (h.key != at) {
        ew_release<V>(h, V, acc, tab);
        h.key = at;
#pragma unroll
        for (int i = 0; i < V; ++i) h.v[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < V; ++i)
        if (i < n) h.v[i] += (double)g[i];
}

struct EwGrad {
    void* dense;         // the operand has no shared axis: its gradient, dense like the output (null: not wanted or shared)
    double* acc;         // it has one: the double accumulator (null: not wanted or not shared)
    int64_t numel;       // elements of the accumulator
    int inner_shared;
};

template <typename T, typename IDX>
__global__ __launch_bounds__(256) void ewise_bwd_kernel(EwArgs a, const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dz,
                                                        EwGrad px, EwGrad py, IDX items, IDX chunks) {
    constexpr int V = Vec16<T>::n;
    __shared__ double tabs[2][EW_TAB];
    double* tx = px.acc && px.numel <= EW_TAB ? tabs[0] : nullptr;
    double* ty = py.acc && py.numel <= EW_TAB ? tabs[1] : nullptr;
    if (tx)
        for (int i = threadIdx.x; i < px.numel; i += 256) tx[i] = 0.0;
    if (ty)
        for (int i = threadIdx.x; i < py.numel; i += 256) ty[i] = 0.0;
    if (tx || ty) __syncthreads();
    const int last = a.rank - 1;
    const int64_t inner = a.extent[last];
    const bool want_y = py.dense || py.acc;
    EwHold<V> hx, hy;
    // the trip count is the workgroup's: every lane takes part in the shuffles of ew_collect
    for (IDX base = (IDX)blockIdx.x * 256; base < items; base += (IDX)gridDim.x * 256) {
        const IDX it = base + threadIdx.x;
        const bool valid = it < items;
        T gx[V], gy[V];
        int n = 0;
        int64_t e0 = 0, zoff = 0, ogx = 0, ogy = 0;
        if (valid) {
            const IDX row = a.rank > 1 ? it / chunks : 0, c = it - row * chunks;
            e0 = (int64_t)c * V;
            n = (int)(inner - e0 < V ? inner - e0 : V);
            zoff = (int64_t)row * inner + e0;
            int64_t ox, oy;
            ew_place<IDX>(a, row, &ox, &oy, &ogx, &ogy);
            T vx[V], vy[V], vd[V];
            ew_load(x + ox + e0 * a.sx[last], a.sx[last], n, vx);
            if (y) ew_load(y + oy + e0 * a.sy[last], a.sy[last], n, vy);
            ew_load(dz + zoff, 1, n, vd);
#pragma unroll
            for (int i = 0; i < V; ++i) ew_grad(a.op, vx[i], y ? vy[i] : (T)0, vd[i], want_y, &gx[i], &gy[i]);
        }
        if (px.dense && valid) ew_store<T, true>((T*)px.dense + zoff, n, gx);
        if (py.dense && valid) ew_store<T, true>((T*)py.dense + zoff, n, gy);
        if (px.acc) ew_collect<T, V>(hx, valid, px.inner_shared, ogx + e0 * a.gx[last], n, gx, px.acc, tx);
        if (py.acc) ew_collect<T, V>(hy, valid, py.inner_shared, ogy + e0 * a.gy[last], n, gy, py.acc, ty);
    }
    if (px.acc) ew_release<V>(hx, px.inner_shared ? 1 : V, px.acc, tx);
    if (py.acc) ew_release<V>(hy, py.inner_shared ? 1 : V, py.acc, ty);
    if (tx || ty) __syncthreads();
    if (tx)
        for (int i = threadIdx.x; i < px.numel; i += 256)
            if (tx[i] != 0.0) atomic_add(px.acc + i, tx[i]);
    if (ty)
        for (int i = threadIdx.x; i < py.numel; i += 256)
            if (ty[i] != 0.0) atomic_add(py.acc + i, ty[i]);
}

// the 32- or 64-bit item counter of the plan's wide_index
template <int WIDE> using ew_index_t = std::conditional_t<WIDE != 0, uint64_t, uint32_t>;

// y, dx, dy: null where the plan has no use for them (a unary op; a gradient that is not wanted)
template <typename T>
int ew_launch_fwd(const EwisePlan& p, const void* x, const void* y, void* z, hipStream_t st) {
    const EwArgs a = {p.a};
    return dispatch<0, 1>(p.wide_index, [&](auto wide) {
        using IDX = ew_index_t<decltype(wide)::value>;
        hipLaunchKernelGGL((ewise_fwd_kernel<T, IDX>), dim3(p.grid), dim3(256), 0, st, a, (const T*)x, (const T*)y, (T*)z, (IDX)p.items, (IDX)p.chunks);
        return 0;
    });
}

template <typename T>
int ew_launch_bwd(mxf_handle h, const EwisePlan& p, const void* x, const void* y, const void* dz, void* dx, void* dy, hipStream_t st) {
    SharedSums sums;
    if (int rc = shared_sums_open<T>(h, "mxf_ewise_bwd", {{p.sum_x ? dx : nullptr, p.numel_gx}, {p.sum_y ? dy : nullptr, p.numel_gy}}, st, &sums)) return rc;
    const EwArgs a = {p.a};
    const EwGrad px = {.dense = p.shared_x ? nullptr : dx, .acc = sums.acc[0], .numel = p.numel_gx, .inner_shared = p.inner_shared_x};
    const EwGrad py = {.dense = p.shared_y ? nullptr : dy, .acc = sums.acc[1], .numel = p.numel_gy, .inner_shared = p.inner_shared_y};
    dispatch<0, 1>(p.wide_index, [&](auto wide) {
        using IDX = ew_index_t<decltype(wide)::value>;
        hipLaunchKernelGGL((ewise_bwd_kernel<T, IDX>), dim3(p.grid), dim3(256), 0, st, a, (const T*)x, (const T*)y, (const T*)dz, px, py, (IDX)p.items, (IDX)p.chunks);
        return 0;
    });
    shared_sums_close(sums, st);
    return 0;
}

// ---- reductions behind the sample axis: x dense (outer, R, inner) -> y dense (outer, inner) -----------------------------------------------

__device__ __forceinline__ double wave_prod(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double red_finish(int kind, double v, int64_t R) { return kind == 1 ? v / (double)R : v; }

// inner == 1.  by_wave: each of the workgroup's four waves owns a row; otherwise the workgroup owns one.
template <typename T>
__global__ __launch_bounds__(256) void reduce_rows_kernel(int kind, int64_t rows, int64_t R, const T* __restrict__ x, T* __restrict__ y, int by_wave) {
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t per = by_wave ? 4 : 1;
    for (int64_t r0 = (int64_t)blockIdx.x * per; r0 < rows; r0 += (int64_t)gridDim.x * per) {
        const int64_t row = by_wave ? r0 + w : r0;
        double v = kind == 2 ? 1.0 : 0.0;
        if (row < rows) {
            const T* p = x + row * R;
            for (int64_t j = by_wave ? lane : threadIdx.x; j < R; j += by_wave ? 64 : 256) v = kind == 2 ? v * (double)p[j] : v + (double)p[j];
        }
        v = kind == 2 ? wave_prod(v) : wave_sum(v);
        if (by_wave) {
            if (lane == 0 && row < rows) y[row] = (T)red_finish(kind, v, R);
        } else {
            if (lane == 0) part[w] = v;
            __syncthreads();
            if (threadIdx.x == 0) {
                const double t = kind == 2 ? part[0] * part[1] * part[2] * part[3] : part[0] + part[1] + part[2] + part[3];
                y[row] = (T)red_finish(kind, t, R);
            }
            __syncthreads();
        }
    }
}

// inner > 1: a thread per output element, lanes along inner, a loop over R
template <typename T>
__global__ __launch_bounds__(256) void reduce_cols_kernel(int kind, int64_t outer, int64_t R, int64_t inner, const T* __restrict__ x, T* __restrict__ y) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < outer * inner; idx += (int64_t)gridDim.x * 256) {
        const int64_t o = idx / inner, i = idx - o * inner;
        const T* p = x + o * R * inner + i;
        double v = kind == 2 ? 1.0 : 0.0;
        for (int64_t j = 0; j < R; ++j) v = kind == 2 ? v * (double)p[j * inner] : v + (double)p[j * inner];
        y[idx] = (T)red_finish(kind, v, R);
    }
}

// sum and mean: dx[o, j, i] += scale dy[o, i]
template <typename T>
__global__ __launch_bounds__(256) void reduce_spread_kernel(int64_t outer, int64_t R, int64_t inner, double scale, const T* __restrict__ dy, T* __restrict__ dx) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < outer * R * inner; idx += (int64_t)gridDim.x * 256) {
        const int64_t o = idx / (R * inner), i = idx % inner;
        dx[idx] += (T)(scale * (double)dy[o * inner + i]);
    }
}

// prod: dx[o, j, i] += dy[o, i] (prod of x[o, k, i] over k < j) (prod over k > j), never a division.  inner > 1: a thread per output element
// walks its column down, leaving the suffix products in `suffix` (double, laid out like x), and up again with the running prefix product.
template <typename T>
__global__ __launch_bounds__(256) void reduce_prod_bwd_kernel(int64_t outer, int64_t R, int64_t inner, const T* __restrict__ x, const T* __restrict__ dy,
                                                              double* __restrict__ suffix, T* __restrict__ dx) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < outer * inner; idx += (int64_t)gridDim.x * 256) {
        const int64_t o = idx / inner, i = idx - o * inner, base = o * R * inner + i;
        double s = 1.0;
        for (int64_t j = R - 1; j >= 0; --j) {
            suffix[base + j * inner] = s;
            s *= (double)x[base + j * inner];
        }
        double pre = (double)dy[idx];
        for (int64_t j = 0; j < R; ++j) {
            dx[base + j * inner] += (T)(pre * suffix[base + j * inner]);
            pre *= (double)x[base + j * inner];
        }
    }
}

// The same for inner == 1 in the forward's two regimes: a wave per row up to RED_WAVE_MAX, the workgroup per row beyond.  Each of the
// group's G threads owns a segment of ceil(R / G) consecutive entries: it walks the segment down, leaving the suffix products WITHIN the
// segment in `suffix`, puts the segment's product into LDS, forms the products of the segments before and behind its own from there, and
// walks the segment up with the running prefix.
template <typename T>
__global__ __launch_bounds__(256) void reduce_prod_bwd_rows_kernel(int64_t rows, int64_t R, const T* __restrict__ x, const T* __restrict__ dy,
                                                                   double* __restrict__ suffix, T* __restrict__ dx, int by_wave) {
    __shared__ double part[256];
    const int G = by_wave ? 64 : 256;
    const int t = by_wave ? (threadIdx.x & 63) : threadIdx.x, g0 = by_wave ? (threadIdx.x & ~63) : 0;
    const int64_t per = by_wave ? 4 : 1, L = (R + G - 1) / G;
    const int64_t lo = t * L < R ? t * L : R, hi = lo + L < R ? lo + L : R;
    for (int64_t r0 = (int64_t)blockIdx.x * per; r0 < rows; r0 += (int64_t)gridDim.x * per) {
        const int64_t row = by_wave ? r0 + (threadIdx.x >> 6) : r0, base = row * R;
        const bool live = row < rows;
        double s = 1.0;
        if (live)
            for (int64_t j = hi - 1; j >= lo; --j) {
                suffix[base + j] = s;
                s *= (double)x[base + j];
            }
        part[threadIdx.x] = s;
        __syncthreads();
        if (live && lo < hi) {
            double pre = (double)dy[row], behind = 1.0;
            for (int u = 0; u < t; ++u) pre *= part[g0 + u];
            for (int u = t + 1; u < G; ++u) behind *= part[g0 + u];
            for (int64_t j = lo; j < hi; ++j) {
                dx[base + j] += (T)(pre * suffix[base + j] * behind);
                pre *= (double)x[base + j];
            }
        }
        __syncthreads();
    }
}

struct RedArgs { int kind; int64_t outer, R, inner; const void *x, *y; void* out; };      // y: dy of the reverse pass; out: y, or dx_acc

template <typename T>
void red_launch_fwd(const RedArgs& a, const ReducePlan& p, hipStream_t st) {
    if (p.rows)
        hipLaunchKernelGGL(reduce_rows_kernel<T>, dim3(p.grid), dim3(256), 0, st, a.kind, a.outer, a.R, (const T*)a.x, (T*)a.out, p.by_wave ? 1 : 0);
    else
        hipLaunchKernelGGL(reduce_cols_kernel<T>, dim3(p.grid), dim3(256), 0, st, a.kind, a.outer, a.R, a.inner, (const T*)a.x, (T*)a.out);
}

template <typename T>
int red_launch_bwd(mxf_handle h, const RedArgs& a, const ReducePlan& p, hipStream_t st) {
    if (p.spread) {
        hipLaunchKernelGGL(reduce_spread_kernel<T>, dim3(p.grid), dim3(256), 0, st, a.outer, a.R, a.inner, a.kind == 1 ? 1.0 / (double)a.R : 1.0, (const T*)a.y, (T*)a.out);
        return 0;
    }
    double* suffix = (double*)mxf_ws(h, (size_t)p.scratch * sizeof(double));
    if (!suffix) MXF_FAIL(h, -4, "mxf_reduce_bwd: out of memory for %lld scratch doubles", (long long)p.scratch);
    if (p.rows)
        hipLaunchKernelGGL(reduce_prod_bwd_rows_kernel<T>, dim3(p.grid), dim3(256), 0, st, a.outer, a.R, (const T*)a.x, (const T*)a.y, suffix, (T*)a.out, p.by_wave ? 1 : 0);
    else
        hipLaunchKernelGGL(reduce_prod_bwd_kernel<T>, dim3(p.grid), dim3(256), 0, st, a.outer, a.R, a.inner, (const T*)a.x, (const T*)a.y, suffix, (T*)a.out);
    return 0;
}

}  // namespace

extern "C" int mxf_ewise_fwd(mxf_handle h, int op, int dtype, int rank, const int64_t* extent, const void* x, const int64_t* stride_x,
                             const void* y, const int64_t* stride_y, void* z, void* stream) {
    if (!h) return -1;
    const EwisePlan p = ewise_plan({.dtype = dtype, .op = op, .rank = rank, .extent = extent, .stride_x = stride_x, .stride_y = stride_y,
                                    .has_x = x != nullptr, .has_y = y != nullptr, .has_z = z != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "mxf_ewise_fwd: %s", p.refusal);
    if (p.empty) return 0;
    return mxf_typed(h, "mxf_ewise_fwd", dtype, [&](auto t) { return ew_launch_fwd<decltype(t)>(p, x, p.binary ? y : nullptr, z, (hipStream_t)stream); });
}

extern "C" int mxf_ewise_bwd(mxf_handle h, int op, int dtype, int rank, const int64_t* extent, const void* x, const int64_t* stride_x,
                             const void* y, const int64_t* stride_y, const void* dz, void* dx_acc, void* dy_acc, void* stream) {
    if (!h) return -1;
    const EwisePlan p = ewise_plan({.dtype = dtype, .op = op, .rank = rank, .bwd = true, .extent = extent, .stride_x = stride_x, .stride_y = stride_y,
                                    .has_x = x != nullptr, .has_y = y != nullptr, .has_z = dz != nullptr, .has_dx = dx_acc != nullptr,
                                    .has_dy = dy_acc != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "mxf_ewise_bwd: %s", p.refusal);
    if (p.empty) return 0;
    return mxf_typed(h, "mxf_ewise_bwd", dtype, [&](auto t) {
        return ew_launch_bwd<decltype(t)>(h, p, x, p.binary ? y : nullptr, dz, dx_acc, p.binary ? dy_acc : nullptr, (hipStream_t)stream);
    });
}

extern "C" int mxf_reduce_fwd(mxf_handle h, int kind, int dtype, int64_t outer, int64_t R, int64_t inner, const void* x, void* y, void* stream) {
    if (!h) return -1;
    const ReducePlan p = reduce_plan({.dtype = dtype, .kind = kind, .outer = outer, .R = R, .inner = inner, .has_x = x != nullptr, .has_y = y != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "mxf_reduce_fwd: %s", p.refusal);
    if (p.empty) return 0;
    const RedArgs a = {.kind = kind, .outer = outer, .R = R, .inner = inner, .x = x, .out = y};
    return mxf_typed(h, "mxf_reduce_fwd", dtype, [&](auto t) { red_launch_fwd<decltype(t)>(a, p, (hipStream_t)stream); });
}

extern "C" int mxf_reduce_bwd(mxf_handle h, int kind, int dtype, int64_t outer, int64_t R, int64_t inner, const void* x, const void* dy,
                              void* dx_acc, void* stream) {
    if (!h) return -1;
    const ReducePlan p = reduce_plan({.dtype = dtype, .kind = kind, .bwd = true, .outer = outer, .R = R, .inner = inner, .has_x = x != nullptr,
                                      .has_y = dy != nullptr, .has_dx = dx_acc != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "mxf_reduce_bwd: %s", p.refusal);
    if (p.empty) return 0;
    const RedArgs a = {.kind = kind, .outer = outer, .R = R, .inner = inner, .x = x, .y = dy, .out = dx_acc};
    return mxf_typed(h, "mxf_reduce_bwd", dtype, [&](auto t) { return red_launch_bwd<decltype(t)>(h, a, p, (hipStream_t)stream); });
}
