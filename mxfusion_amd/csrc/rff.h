// Per-element math of the random Fourier feature expansion (rff.hip): a stationary GP prior draw evaluated at a point x,
//   f(x)[j]  = sum_d cos(x . omega_d + b_d) W[d,j]
//   df/dx_q  = -sum_d sin(x . omega_d + b_d) omega_dq sum_j G[j] W[d,j]          (G: the cotangent of f(x))
// The argument of the cosine is in whatever unit the prepared operands are in: radians here, and revolutions (omega and b divided by 2 pi by
// rff_prep_kernel, the gradient multiplied by 2 pi once at the end) for the float32 kernels of rff.hip, whose MXF_RFF_COS / MXF_RFF_SIN are the
// hardware's.  float and double, host and device: tests/host/rff_check.cpp prints these without a GPU.  QP is Q padded with zeros.
#pragma once
#include <math.h>

#ifndef MXF_HD
#if defined(__HIPCC__)
#define MXF_HD __host__ __device__
#else
#define MXF_HD
#endif
#endif
#ifndef MXF_RFF_COS            // cos and sin of a prepared argument; rff.hip substitutes the device forms
#define MXF_RFF_COS(T, x) cos(x)
#define MXF_RFF_SIN(T, x) sin(x)
#endif

// x . omega + b
template <typename T, int QP>
MXF_HD inline T rff_arg(const T* x, const T* omega, T b) {
    T r = b;
#pragma unroll
    for (int q = 0; q < QP; ++q) r += x[q] * omega[q];
    return r;
}

// one feature: cos(x . omega + b)
template <typename T, int QP>
MXF_HD inline T rff_feature(const T* x, const T* omega, T b) { return MXF_RFF_COS(T, (rff_arg<T, QP>(x, omega, b))); }

// one feature's part of the gradient: dx[q] += sin(x . omega + b) gw omega[q], gw = sum_j G[j] W[d,j]; the caller negates (and rescales) the sum
template <typename T, int QP>
MXF_HD inline void rff_feature_bwd(const T* x, const T* omega, T b, T gw, T* dx) {
    const T a = MXF_RFF_SIN(T, (rff_arg<T, QP>(x, omega, b))) * gw;
#pragma unroll
    for (int q = 0; q < QP; ++q) dx[q] += a * omega[q];
}
