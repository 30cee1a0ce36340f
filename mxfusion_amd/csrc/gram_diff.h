// Per-pair math of the difference-form covariances (gram_diff.hip): Periodic, RationalQuadratic and SpectralMixture as functions of the
// per-dimension differences tau_d = x_d - x'_d, each a sum over components (one for Periodic and RQ, A for SpectralMixture) of
//   amp * k(tau),   amp = variance | variance | w_a
//   Periodic  k = exp(-sum_d hl_d sin^2(pi u_d)),  u_d = tau_d / p_d reduced to [-1/2, 1/2],  hl_d = 1 / (2 l_d^2)
//   RQ        k = exp(-alpha log1p(x)),            x = sum_d tau_d^2 / l_d^2 / (2 alpha)
//   SM        k = exp(-sum_d c_d tau_d^2) prod_d cos(2 pi u_d),  c_d = 2 pi^2 s_d^2,  u_d = tau_d mu_d reduced to [-1/2, 1/2]
// gd_prepare turns a component's raw operands into the constants above once per workgroup; gd_value is k; gd_grad is k with its slopes in
// tau_d and the un-scaled per-pair terms of the two parameter gradients, which the caller sums with the cotangent as weight and scales once
// at the end (gd_finish).  A phase is reduced BEFORE the sine or cosine (u = x - rint(x): odd in x, so k(tau) == k(-tau) bit for bit), so the
// float32 error of a trigonometric factor is |tau / p| eps and no more.  The SpectralMixture slopes use leave-one-out products: no division
// by a cosine.  float and double, host and device: tests/host/gram_diff_check.cpp prints these without a GPU.  QT is Q padded (gd_prepare
// fills the padding with constants that leave k alone).
#pragma once
#include <math.h>

#include "../../include/mxf_gp.h"      // MXF_KD_*, the limits

#ifndef MXF_HD
#if defined(__HIPCC__)
#define MXF_HD __host__ __device__
#else
#define MXF_HD
#endif
#endif

#ifndef MXF_GD_FNS      // sin / cos of an angle in revolutions, |u| <= 1/2, and e^x for x <= 0; gram_diff.hip substitutes the device forms
template <typename T> MXF_HD inline T gd_sin_rev(T u) { return sin((T)6.283185307179586477 * u); }
template <typename T> MXF_HD inline T gd_cos_rev(T u) { return cos((T)6.283185307179586477 * u); }
template <typename T> MXF_HD inline T gd_exp_nonpos(T x) { return exp(x); }
template <typename T> MXF_HD inline T gd_log1p(T x) { return log1p(x); }
#endif

// a phase in revolutions reduced to [-1/2, 1/2]
template <typename T> MXF_HD inline T gd_reduce(T x) { return x - rint(x); }

// constants of one component: amp and three rows of QT
template <typename T, int QT> struct GdComp { T amp; T a1[QT], a2[QT], a3[QT]; };

// p0 (the component's amplitude), p1 / p2 (its Q, or 1 when !ard, values; RQ: p2 is alpha)
template <typename T, int KIND, int QT>
MXF_HD inline void gd_prepare(int Q, int ard, T p0, const T* p1, const T* p2, GdComp<T, QT>& c) {
    const T pi = (T)3.141592653589793238;
    c.amp = p0;
    for (int q = 0; q < QT; ++q) {
        const bool in = q < Q;
        const int j = ard ? q : 0;
        if (KIND == MXF_KD_PERIODIC) {       // a1 = 1 / p, a2 = 1 / (2 l^2), a3 = pi a1 a2
            c.a1[q] = in ? (T)1 / p2[j] : (T)0;
            c.a2[q] = in ? (T)0.5 / (p1[j] * p1[j]) : (T)0;
            c.a3[q] = pi * c.a1[q] * c.a2[q];
        } else if (KIND == MXF_KD_RQ) {      // a1 = 1 / l^2, a2 = alpha, a3 = 1 / (2 alpha)
            c.a1[q] = in ? (T)1 / (p1[j] * p1[j]) : (T)0;
            c.a2[q] = p2[0];
            c.a3[q] = (T)0.5 / p2[0];
        } else {                             // a1 = mu, a2 = 2 pi^2 s^2
            c.a1[q] = in ? p1[q] : (T)0;
            c.a2[q] = in ? (T)2 * pi * pi * p2[q] * p2[q] : (T)0;
            c.a3[q] = 0;
        }
    }
}

template <typename T, int KIND, int QT>
MXF_HD inline T gd_value(const T* tau, const GdComp<T, QT>& c) {
    if (KIND == MXF_KD_PERIODIC) {
        T e = 0;
#pragma unroll
        for (int q = 0; q < QT; ++q) { const T s = gd_sin_rev<T>((T)0.5 * gd_reduce<T>(tau[q] * c.a1[q])); e = fma(c.a2[q] * s, s, e); }
        return gd_exp_nonpos<T>(-e);
    }
    if (KIND == MXF_KD_RQ) {
        T r2 = 0;
#pragma unroll
        for (int q = 0; q < QT; ++q) r2 = fma(tau[q] * c.a1[q], tau[q], r2);
        return gd_exp_nonpos<T>(-c.a2[0] * gd_log1p<T>(r2 * c.a3[0]));
    }
    T e = 0, P = 1;
#pragma unroll
    for (int q = 0; q < QT; ++q) { e = fma(tau[q] * c.a2[q], tau[q], e); P *= gd_cos_rev<T>(gd_reduce<T>(tau[q] * c.a1[q])); }
    return gd_exp_nonpos<T>(-e) * P;
}

// x / (1 + x) - log1p(x) for x >= 0 with y = x / (1 + x): -(y^2 / 2 + y^3 / 3 + ...), summed as a series where the two terms would cancel
template <typename T>
MXF_HD inline T gd_rq_dalpha(T x, T y, T L) {
    const T small = sizeof(T) == 4 ? (T)0.0625 : (T)0.0009765625;
    if (y >= small) return y - L;
    return -y * y * ((T)0.5 + y * ((T)(1.0 / 3.0) + y * ((T)0.25 + y * ((T)0.2 + y * ((T)(1.0 / 6.0) + y * (T)(1.0 / 7.0))))));
}

// k, dk / dtau_q, and the pair's terms t1 / t2 of the two parameter sums (gd_finish says what each is scaled by)
template <typename T, int KIND, int QT>
MXF_HD inline T gd_grad(const T* tau, const GdComp<T, QT>& c, T* dtau, T* t1, T* t2) {
    if (KIND == MXF_KD_PERIODIC) {
        T e = 0, s2[QT], S[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            const T u = gd_reduce<T>(tau[q] * c.a1[q]), s = gd_sin_rev<T>((T)0.5 * u);
            S[q] = gd_sin_rev<T>(u);                  // sin(2 pi u) = d sin^2(pi u) / d(pi u)
            s2[q] = c.a2[q] * s * s;
            e += s2[q];
        }
        const T k = gd_exp_nonpos<T>(-e);
#pragma unroll
        for (int q = 0; q < QT; ++q) { dtau[q] = -k * c.a3[q] * S[q]; t1[q] = k * s2[q]; t2[q] = -dtau[q] * tau[q]; }
        return k;
    }
    if (KIND == MXF_KD_RQ) {
        T r2 = 0;
#pragma unroll
        for (int q = 0; q < QT; ++q) r2 = fma(tau[q] * c.a1[q], tau[q], r2);
        const T x = r2 * c.a3[0], L = gd_log1p<T>(x), k = gd_exp_nonpos<T>(-c.a2[0] * L), kb = k / ((T)1 + x);
#pragma unroll
        for (int q = 0; q < QT; ++q) { dtau[q] = -kb * tau[q] * c.a1[q]; t1[q] = -dtau[q] * tau[q]; t2[q] = 0; }
        t2[0] = k * gd_rq_dalpha<T>(x, x / ((T)1 + x), L);
        return k;
    }
    const T twopi = (T)6.283185307179586477;
    T e = 0, C[QT], S[QT], pre[QT];      // pre[q] = prod_{j < q} C[j]
    T P = 1;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        const T u = gd_reduce<T>(tau[q] * c.a1[q]);
        e = fma(tau[q] * c.a2[q], tau[q], e);
        C[q] = gd_cos_rev<T>(u); S[q] = gd_sin_rev<T>(u);
        pre[q] = P; P *= C[q];
    }
    const T ex = gd_exp_nonpos<T>(-e), k = ex * P;
    T suf = 1;                           // prod_{j > q} C[j]
#pragma unroll
    for (int q = QT - 1; q >= 0; --q) {
        const T dP = -twopi * S[q] * pre[q] * suf * ex;      // d(ex P) / d(tau_q mu_q)
        suf *= C[q];
        t1[q] = dP * tau[q];
        t2[q] = -k * tau[q] * tau[q];
        dtau[q] = fma(dP, c.a1[q], (T)-2 * k * c.a2[q] * tau[q]);
    }
    return k;
}

// the gradient of the raw operand from the cotangent-weighted sum of its pairs' terms: which = 1 / 2 for p1 / p2, v1 / v2 the raw values
template <typename T, int KIND>
MXF_HD inline T gd_finish(int which, T amp, T v1, T v2, T sum) {
    if (KIND == MXF_KD_PERIODIC) return which == 1 ? amp * (T)2 / v1 * sum : amp / v2 * sum;      // dl: k sin^2 / l^3; dp: -dk/dtau tau / p
    if (KIND == MXF_KD_RQ) return which == 1 ? amp / v1 * sum : amp * sum;                         // dl: k tau^2 / (l^3 (1 + x))
    const T pi = (T)3.141592653589793238;
    return which == 1 ? amp * sum : amp * (T)4 * pi * pi * v2 * sum;                               // dmu; ds: -4 pi^2 tau^2 s k
}
