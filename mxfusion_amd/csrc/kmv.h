// The stationary covariance functions as functions of the reduced quantity of a pair, shared by the Gram build (gram.hip) and the matrix-free
// kernel product (kmv.hip): a pair's covariance is the same function of the operands in both.  Device only (the exponentials and the square
// root are common.h's device forms), so there is no host check of this header.
//   red = sum_q ((x_q - z_q) c / l_q)^2,  c = coord_scale()      (the scaled r^2; c = 1 for the Matern kinds, whose red is r^2 itself)
//   k   = variance f(red)                                         cov_from
//   f, f' = df / dred                                             cov_slope (the reverse mode in lengthscale and variance)
#pragma once
#include "common.h"

// coordinate pre-scale so that the RBF epilogue is a bare exp2:  exp(-r2/2) = 2^-(c^2 r2), c^2 = log2(e)/2
template <typename T, int KIND> __device__ __forceinline__ T coord_scale() {
    return KIND == MXF_K_RBF ? (T)0.84932180028801904272 /* sqrt(0.5*log2(e)) */ : (T)1;
}

// value of the covariance from the reduced quantity (scaled r2, or the dot product for LINEAR)
template <typename T, int KIND> __device__ __forceinline__ T cov_from(T red, T variance) {
    if (KIND == MXF_K_RBF) return variance * fast_exp2_neg<T>(red);
    if (KIND == MXF_K_MATERN12) { T r = t_sqrt<T>(red < (T)1e-14 ? (T)1e-14 : red); return variance * t_exp<T>(-r); }
    if (KIND == MXF_K_MATERN32) {
        T r = (T)1.7320508075688772 * t_sqrt<T>(red < (T)1e-14 ? (T)1e-14 : red);
        return variance * ((T)1 + r) * t_exp<T>(-r);
    }
    if (KIND == MXF_K_MATERN52) {   // matern.py:85-87: clipped r in the linear/exp terms, UN-clipped r2 in 5/3 r2
        T r = (T)2.23606797749979 * t_sqrt<T>(red < (T)1e-14 ? (T)1e-14 : red);
        return variance * ((T)1 + r + (T)(5.0 / 3.0) * red) * t_exp<T>(-r);
    }
    return red;   // LINEAR: the dot product itself
}

// f = cov_from(red, 1) and its slope df / dred, the stationary kinds only.  The clip of r carries no slope (cov_and_slope of gram_bwd.hip: the
// same rule), so a clipped pair gives 0, and for MATERN52 the slope of its un-clipped 5/3 red term alone.
template <typename T, int KIND> __device__ __forceinline__ void cov_slope(T red, T& f, T& df) {
    if (KIND == MXF_K_RBF) { f = fast_exp2_neg<T>(red); df = (T)-0.69314718055994530942 * f; return; }
    const bool clipped = red < (T)1e-14;
    const T r = t_sqrt<T>(clipped ? (T)1e-14 : red);
    if (KIND == MXF_K_MATERN12) { f = t_exp<T>(-r); df = clipped ? (T)0 : -f / ((T)2 * r); return; }
    if (KIND == MXF_K_MATERN32) {
        const T s3 = (T)1.7320508075688772, e = t_exp<T>(-s3 * r);
        f = ((T)1 + s3 * r) * e; df = clipped ? (T)0 : (T)-1.5 * e; return;
    }
    const T s5 = (T)2.23606797749979, e = t_exp<T>(-s5 * r);
    f = ((T)1 + s5 * r + (T)(5.0 / 3.0) * red) * e;
    df = clipped ? (T)(5.0 / 3.0) * e : (T)(-5.0 / 6.0) * ((T)1 + s5 * r) * e;
}
