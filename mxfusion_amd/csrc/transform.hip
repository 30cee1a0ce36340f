// Variable transformations of several parameters in one launch (gfx950): the flat buffer holds one segment per parameter, segment k is
// mapped by its own kind -- softplus plus an offset, or the logistic map onto (lower, upper).  The segment table (kind, start, size,
// parameters) travels BY VALUE in the kernel arguments, TR_SEG segments per launch, so a call makes no host-to-device copy and captures into
// a hipGraph like every other call of the step.  blockIdx.y is the segment and blockIdx.x walks it in a grid-stride loop: no prefix search
// per element, and the workgroups past a short segment's end return at once.  A model has a handful of constrained parameters of a few
// elements each: launch-bound, one launch each way where there was one per parameter.
//
// Replaces: Softplus.transform with an offset (components/variables/var_trans.py:53-91) and Logistic.transform (var_trans.py:105-147) as
// ObjectiveBlock.__call__ applies them before every compute, and MXNet autograd through them.
#include <cfloat>
#include <cmath>

#include "common.h"

namespace {

constexpr int TR_SEG = MXF_TR_MAX_SEG;

struct TrTable {
    int kind[TR_SEG];
    int64_t start[TR_SEG], size[TR_SEG];
    double p0[TR_SEG], p1[TR_SEG];
    double lo[TR_SEG], hi[TR_SEG];      // LOGISTIC: the bounds rounded inwards to the working dtype (exact in it)
};

template <typename T> struct TrLimits;
template <> struct TrLimits<float> { static constexpr float tiny = FLT_MIN; };
template <> struct TrLimits<double> { static constexpr double tiny = DBL_MIN; };

// e = exp(-|x|), 0 where it would be subnormal: beyond that point sigmoid(x) is 0 or 1 and its slope 0, exactly
template <typename T> __device__ __forceinline__ T tr_e(T x) {
    const T e = exp(-fabs(x));
    return e < TrLimits<T>::tiny ? (T)0 : e;
}
template <typename T> __device__ __forceinline__ T tr_sigmoid(T x, T e) { return x >= (T)0 ? (T)1 / ((T)1 + e) : e / ((T)1 + e); }

template <typename T>
__global__ __launch_bounds__(256) void transform_fwd_kernel(TrTable t, const T* __restrict__ x, T* __restrict__ y) {
    const int k = blockIdx.y;
    const int64_t n = t.size[k];
    const T* xs = x + t.start[k];
    T* ys = y + t.start[k];
    const T p0 = (T)t.p0[k], p1 = (T)t.p1[k], lo = (T)t.lo[k], hi = (T)t.hi[k];
    const bool logistic = t.kind[k] == MXF_TR_LOGISTIC;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T v = xs[i];
        if (logistic) {
            const T e = tr_e<T>(v), r = p0 + p1 * tr_sigmoid<T>(v, e);
            ys[i] = e == (T)0 ? (v >= (T)0 ? hi : lo)                       // saturated: the bound itself
                              : (r < lo ? lo : (r > hi ? hi : r));          // (comparisons: a NaN stays a NaN)
        } else
            ys[i] = fmax(v, (T)0) + log1p(exp(-fabs(v))) + p0;              // softplus_f of elementwise.hip, then the offset
    }
}

template <typename T>
__global__ __launch_bounds__(256) void transform_bwd_kernel(TrTable t, const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx) {
    const int k = blockIdx.y;
    const int64_t n = t.size[k];
    const T* xs = x + t.start[k];
    const T* gs = dy + t.start[k];
    T* ds = dx + t.start[k];
    const T p1 = (T)t.p1[k];
    const bool logistic = t.kind[k] == MXF_TR_LOGISTIC;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const T v = xs[i], e = tr_e<T>(v), q = (T)1 + e;
        const T slope = logistic ? p1 * (e / (q * q)) : tr_sigmoid<T>(v, e);
        ds[i] += gs[i] * slope;
    }
}

// the smallest value of the working dtype that is >= v / the largest that is <= v
static double tr_round_up(double v, int dtype) {
    if (dtype != MXF_F32) return v;
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return (double)f;
}
static double tr_round_down(double v, int dtype) {
    if (dtype != MXF_F32) return v;
    float f = (float)v;
    if ((double)f > v) f = nextafterf(f, -INFINITY);
    return (double)f;
}

int run(mxf_handle h, const char* name, int dtype, int nseg, const int* kinds, const int64_t* sizes, const double* p0, const double* p1,
        const void* x, const void* dy, void* out, bool bwd, hipStream_t st) {
    if (!h) return -1;
    if (nseg <= 0) return 0;
    if (dtype != MXF_F32 && dtype != MXF_F64) return mxf_bad_dtype(h, name, dtype);
    if (!kinds || !sizes || !p0 || !p1) MXF_FAIL(h, -2, "%s: null segment table", name);
    int64_t total = 0;
    for (int k = 0; k < nseg; ++k) {              // every segment is checked before anything is launched
        if (kinds[k] != MXF_TR_SOFTPLUS && kinds[k] != MXF_TR_LOGISTIC) MXF_FAIL(h, -2, "%s: unknown transformation kind %d (segment %d)", name, kinds[k], k);
        if (sizes[k] < 0) MXF_FAIL(h, -2, "%s: negative size (segment %d)", name, k);
        if (!std::isfinite(p0[k])) MXF_FAIL(h, -2, "%s: p0 is not finite (segment %d)", name, k);
        if (kinds[k] == MXF_TR_LOGISTIC) {
            if (!std::isfinite(p1[k]) || !(p1[k] > 0)) MXF_FAIL(h, -2, "%s: the lower bound is not below the upper bound (segment %d)", name, k);
            if (!(tr_round_up(p0[k], dtype) <= tr_round_down(p0[k] + p1[k], dtype)))
                MXF_FAIL(h, -2, "%s: no value of the working dtype lies between the bounds (segment %d)", name, k);
        }
        total += sizes[k];
    }
    if (total == 0) return 0;
    if (!x || !out || (bwd && !dy)) MXF_FAIL(h, -2, "%s: null buffer", name);
    int64_t start = 0;
    for (int k = 0; k < nseg;) {
        TrTable t = {};
        int m = 0;
        int64_t longest = 0;
        for (; k < nseg && m < TR_SEG; ++k) {
            if (sizes[k] > 0) {
                t.kind[m] = kinds[k]; t.start[m] = start; t.size[m] = sizes[k];
                t.p0[m] = p0[k]; t.p1[m] = p1[k];
                if (kinds[k] == MXF_TR_LOGISTIC) { t.lo[m] = tr_round_up(p0[k], dtype); t.hi[m] = tr_round_down(p0[k] + p1[k], dtype); }
                if (sizes[k] > longest) longest = sizes[k];
                ++m;
            }
            start += sizes[k];
        }
        if (m == 0) continue;
        const dim3 grid(grid_for(longest), (unsigned)m), block(256);
        const int rc = mxf_typed(h, name, dtype, [&](auto e) {
            using T = decltype(e);
            if (bwd) hipLaunchKernelGGL((transform_bwd_kernel<T>), grid, block, 0, st, t, (const T*)x, (const T*)dy, (T*)out);
            else hipLaunchKernelGGL((transform_fwd_kernel<T>), grid, block, 0, st, t, (const T*)x, (T*)out);
        });
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

extern "C" int mxf_transform_fwd(mxf_handle h, int dtype, int nseg, const int* kinds, const int64_t* sizes, const double* p0, const double* p1,
                                 const void* x, void* y, void* stream) {
    return run(h, "mxf_transform_fwd", dtype, nseg, kinds, sizes, p0, p1, x, nullptr, y, false, (hipStream_t)stream);
}

extern "C" int mxf_transform_bwd(mxf_handle h, int dtype, int nseg, const int* kinds, const int64_t* sizes, const double* p0, const double* p1,
                                 const void* x, const void* dy, void* dx_acc, void* stream) {
    return run(h, "mxf_transform_bwd", dtype, nseg, kinds, sizes, p0, p1, x, dy, dx_acc, true, (hipStream_t)stream);
}
