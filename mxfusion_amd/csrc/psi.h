// Per-element math of the RBF psi statistics (psi.hip): the expected kernel under q(x_n) = N(mu_n, diag(s_n)), k = 1 for Psi1, k = 2 for Psi2.
//   Psi1[m,n]     = var   c1_n exp(-1/2 sum_q a1_nq (mu_nq - z_mq)^2)                            a1 = 1 / (s + l^2),   c1 = prod_q sqrt(l^2 a1)
//   psi2n[n,m,m'] = var^2 c2_n exp(-D[m,m']) exp(-sum_q a2_nq (mu_nq - (z_mq + z_m'q) / 2)^2)    a2 = 1 / (2 s + l^2), c2 = prod_q sqrt(l^2 a2)
//   D[m,m']       = sum_q (z_mq - z_m'q)^2 / (4 l_q^2)
// sqrt(l^2 a) = (1 + k s / l^2)^-1/2 is 1 at s = 0 with no 0 / 0, and every derivative below is a product of a, the offset and s / l^2: nothing
// is divided by s.  A far row underflows in exp to a clean 0 that multiplies finite factors.
// float and double, host and device: tests/host/psi_check.cpp prints these without a GPU.  QP is Q padded with zeros (mu = z = a = 0).
//
// The reverse mode sums, over the terms t of one row n with weight w_t = cotangent * term,
//   V = sum w_t,   M_q = sum w_t a_q e_tq,   U_q = sum w_t (a_q e_tq)^2            e = the offset mu - z (k = 1) or mu - zbar (k = 2)
// and the row's gradients follow from them (psi_dmu, psi_ds, psi_dl2_row): three accumulators per coordinate instead of five.
#pragma once
#include <math.h>

#ifndef MXF_HD
#if defined(__HIPCC__)
#define MXF_HD __host__ __device__
#else
#define MXF_HD
#endif
#endif
#ifndef MXF_PSI_EXP            // e^x for x <= 0; psi.hip substitutes the bare device forms of common.h
#define MXF_PSI_EXP(T, x) exp(x)
#endif

// row constants of one coordinate: a = 1 / (k s + l2) and the factor sqrt(l2 a) of c
template <typename T>
MXF_HD inline void psi_row_q(int k, T s, T l2, T& a, T& cq) {
    a = (T)1 / ((T)k * s + l2);
    cq = sqrt(l2 * a);
}

// c exp(-1/2 sum_q a_q (mu_q - z_q)^2): Psi1 without the variance.  ae[q] = a_q (mu_q - z_q) for the reverse mode.
template <typename T, int QP>
MXF_HD inline T psi1_term(const T* mu, const T* a, T c, const T* z, T* ae) {
    T r = 0;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        const T d = mu[q] - z[q];
        ae[q] = a[q] * d;
        r += ae[q] * d;
    }
    return c * MXF_PSI_EXP(T, (T)-0.5 * r);
}

// c exp(-sum_q a_q (mu_q - zbar_q)^2), zbar = (z_m + z_m') / 2: psi2n without var^2 exp(-D).  ae[q] = a_q (mu_q - zbar_q).
template <typename T, int QP>
MXF_HD inline T psi2_term(const T* mu, const T* a, T c, const T* zbar, T* ae) {
    T r = 0;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        const T e = mu[q] - zbar[q];
        ae[q] = a[q] * e;
        r += ae[q] * e;
    }
    return c * MXF_PSI_EXP(T, -r);
}

// D[m,m'] of one coordinate and its weight in the reverse mode
template <typename T>
MXF_HD inline T psi2_dist_q(T zm, T zm2, T l2) { const T d = zm - zm2; return d * d / ((T)4 * l2); }

// a row's gradients from its sums (k = 1, 2)
template <typename T>
MXF_HD inline T psi_dmu(int k, T Mq) { return -(T)k * Mq; }
template <typename T>
MXF_HD inline T psi_ds(int k, T a, T Uq, T V) { return (T)0.5 * (T)k * ((T)k * Uq - a * V); }
template <typename T>      // d / d(l^2), the row's part; Psi2's D[m,m'] adds psi2_dl2_pair
MXF_HD inline T psi_dl2_row(int k, T a, T s, T l2, T Uq, T V) { return (T)0.5 * (T)k * (Uq + a * (s / l2) * V); }

// a pair's gradients of Psi2 from its sums over the rows, P = sum_n w psi2n and A_q = sum_n w psi2n a_q e_q:
// d/dz_m = A_q - P (z_m - z_m') / (2 l2),  d/dz_m' = A_q + P (z_m - z_m') / (2 l2),  d/d(l^2) += P (z_m - z_m')^2 / (4 l2^2)
template <typename T>
MXF_HD inline T psi2_dz_pair(T Aq, T P, T zm, T zm2, T l2, int side) {
    const T t = P * (zm - zm2) / ((T)2 * l2);
    return side == 0 ? Aq - t : Aq + t;
}
template <typename T>
MXF_HD inline T psi2_dl2_pair(T P, T zm, T zm2, T l2) { const T d = (zm - zm2) / l2; return (T)0.25 * P * d * d; }
