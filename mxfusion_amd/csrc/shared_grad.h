// The gradient of an operand that is shared over the sample axis and/or the batch axis of the rows (s, b) of a reverse mode (mvn.hip,
// wishart.hip, simplex.hip, dense.hip).  Such a gradient is dense, shaped like its operand with the shared axes at extent 1, and is the
// sum over those axes: the kernels form it with atomics in a DOUBLE accumulator for either dtype -- a float32 sum of hundreds of rows in
// arrival order would lose digits that the operands have.  For double the accumulator is the caller's buffer itself; for float32 it is
// zeroed handle scratch whose sums one closing launch adds to the caller's buffers with one rounding per element.
#pragma once
#include <initializer_list>

#include "common.h"

// own_s, own_b: the operand has a sample / a batch axis of its own (an extent above 1, a stride other than 0).

// the operand is shared over an axis along which the rows (S, B) differ
__host__ __device__ __forceinline__ bool shared_over(bool own_s, bool own_b, int64_t S, int64_t B) { return (!own_s && S > 1) || (!own_b && B > 1); }

// the index of element 0 of row (s, b) in the operand's gradient (S|1, B|1, row)
__host__ __device__ __forceinline__ int64_t shared_row(bool own_s, bool own_b, int64_t s, int64_t b, int64_t B, int64_t row) {
    return ((own_s ? s : 0) * (own_b ? B : 1) + (own_b ? b : 0)) * row;
}

// the number of elements of that gradient
static inline int64_t shared_numel(bool own_s, bool own_b, int64_t S, int64_t B, int64_t row) { return (own_s ? S : 1) * (own_b ? B : 1) * row; }

constexpr int SHARED_SEGS = 3;

// One gradient that is summed in double: the caller's buffer and its element count (a null buffer or a count of 0: absent).  elsewhere: the
// caller adds the float32 sums to dst itself (mvn_inverse_bwd_kernel does, before its own rounding) and the closing launch leaves them out.
struct SharedSeg {
    void* dst;
    int64_t count;
    bool elsewhere = false;
};

// the sums of the segments lie back to back in src, segment k ending at end[k]; dst[k] null: not this launch's to add (the launch still
// spans such a segment: its threads find no destination and do nothing)
struct FoldTable {
    const double* src;
    float* dst[SHARED_SEGS];
    int64_t end[SHARED_SEGS];
};

struct SharedSums {
    double* acc[SHARED_SEGS];      // the accumulator of each segment, null where it is absent
    FoldTable fold;                // float32: what shared_sums_close adds; src null: nothing
};

// dst[k][i] += src[begin of k + i], each element once
static __global__ __launch_bounds__(256) void mxf_fold_kernel(FoldTable t) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.end[SHARED_SEGS - 1]; i += (int64_t)gridDim.x * blockDim.x) {
        float* dst = t.dst[0];
        int64_t begin = 0;
#pragma unroll
        for (int k = 1; k < SHARED_SEGS; ++k)          // selects, not indexed loads: the table stays in scalar registers
            if (i >= t.end[k - 1]) {
                dst = t.dst[k];
                begin = t.end[k - 1];
            }
        if (dst) dst[i - begin] += (float)t.src[i];
    }
}

// out[i] = acc[i], rounded once: the sums that a split reduction axis left in zeroed doubles (rff.hip, kmv.hip, psi.hip)
template <typename T>
static __global__ __launch_bounds__(256) void mxf_narrow_kernel(int64_t total, const double* __restrict__ acc, T* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) out[i] = (T)acc[i];
}

// The accumulators of up to three segments, in out->acc: the buffers themselves for double; for float32 consecutive pieces of one zeroed
// scratch allocation of the handle (-4 if it cannot be had).  name: the entry point, for the message.
template <typename T>
int shared_sums_open(mxf_handle h, const char* name, std::initializer_list<SharedSeg> segs, hipStream_t st, SharedSums* out) {
    *out = SharedSums();
    int64_t total = 0;
    for (const SharedSeg& g : segs) total += g.dst ? g.count : 0;
    double* ws = nullptr;
    if (sizeof(T) == 4 && total > 0) {
        ws = (double*)mxf_ws(h, (size_t)total * sizeof(double));
        if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %lld scratch doubles", name, (long long)total);
        MXF_HIP(h, hipMemsetAsync(ws, 0, (size_t)total * sizeof(double), st));
    }
    int k = 0;
    int64_t off = 0;
    for (const SharedSeg& g : segs) {
        if (k == SHARED_SEGS) break;
        if (g.dst && g.count > 0) {
            out->acc[k] = ws ? ws + off : (double*)g.dst;
            if (ws && !g.elsewhere) {
                out->fold.src = ws;
                out->fold.dst[k] = (float*)g.dst;
            }
            off += g.count;
        }
        out->fold.end[k++] = off;
    }
    for (; k < SHARED_SEGS; ++k) out->fold.end[k] = off;
    return 0;
}

// after the kernel that summed: the one launch that adds every float32 segment's sums to its buffer
static inline void shared_sums_close(const SharedSums& s, hipStream_t st) {
    if (s.fold.src) hipLaunchKernelGGL(mxf_fold_kernel, dim3(grid_for(s.fold.end[SHARED_SEGS - 1])), dim3(256), 0, st, s.fold);
}
