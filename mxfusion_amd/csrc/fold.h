// The closing step of the float32 reverse modes that sum a shared operand's gradient in double (mvn.hip, wishart.hip, simplex.hip, dense.hip): the
// sums, formed with atomics in zeroed handle scratch, are added to the caller's float32 buffer with one rounding per element.
#pragma once
#include "common.h"

// dst[i] += src[i]
static __global__ __launch_bounds__(256) void mxf_fold_kernel(int64_t n, const double* __restrict__ src, float* __restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] += (float)src[i];
}

// the same for two destinations whose sums lie back to back in src: dst1[i] += src[i] (i < n1), dst2[i] += src[n1 + i] (i < n2)
static __global__ __launch_bounds__(256) void mxf_fold2_kernel(int64_t n1, const double* __restrict__ src, float* __restrict__ dst1, int64_t n2,
                                                               float* __restrict__ dst2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n1) dst1[i] += (float)src[i];
        else dst2[i - n1] += (float)src[i];
    }
}
