// Link functions of the non-Gaussian SVGP likelihoods (likelihood.hip): g(f) = log p(y | f), g'(f), g''(f) and mu(f) = E[y | f] of
//   MXF_LIK_BERNOULLI_LOGIT   g = log sigmoid((2y - 1) f)          mu = sigmoid(f)
//   MXF_LIK_BERNOULLI_PROBIT  g = log Phi((2y - 1) f)              mu = Phi(f)
//   MXF_LIK_POISSON_EXP       g = y f - exp(f) - lgamma(y + 1)     mu = exp(f)
// float and double, callable from host and device code -- the host side exists so that tests/host/lik_check.cpp can hold them to SciPy
// without a GPU.  No tables in memory, no inline assembly.  Every value is finite and accurate over |f| <= 40 in both precisions:
//
// log sigmoid(z) = min(z, 0) - log1p(exp(-|z|)) and its derivatives from the one e = exp(-|z|): no 1 - sigmoid cancellation.
//
// log Phi(z), lambda(z) = phi(z) / Phi(z) and lambda' = -lambda (z + lambda):
//   z >= 0        Phi = 1 - q with q = erfc(z / sqrt 2) / 2, log Phi = log1p(-q); lambda and z + lambda are sums of positive terms.
//   -5 <= z < 0   log(erfc(-z / sqrt 2) / 2) directly; R = Phi / phi is the Mills ratio, lambda = 1 / R and lambda - t = lambda (1 - t R) with
//                 t = -z: at t = 5 the subtraction 1 - t R = 0.036 costs a factor 28 on R's 4e-15.
//   z < -5        erfc underflows (float32: z = -13, float64: z = -38) and 1 - t R cancels without bound, so the Mills ratio comes from its
//                 continued fraction  R = 1 / (t + C),  C = 1 / (t + 2 / (t + 3 / (t + ...))):  lambda = t + C, lambda - t = C and
//                 log Phi = -t^2 / 2 - log(2 pi) / 2 - log(t + C) are sums of positive terms.  Evaluated bottom-up to depth 10 + 450 / t^2 (28 at
//                 t = 5, 10 at t = 40), two levels more than the depth at which it is within 2e-15 of the exact ratio.
//   The z < 0 forms run in double for either T: in float32 the rounding of z / sqrt 2 alone moves erfc by z^2 2^-25, 2e-6 at z = -8, which
//   the ratio phi / Phi and 1 - t R amplify further.  z >= 0 stays in T.
//
// The Poisson terms y f, exp(f) and lgamma(y + 1) are each far larger than their sum near its maximum (y = 50, f = 4: 200 - 54.6 - 148.5),
// so they are formed in double for either T, as unidist.h does for its lgamma differences; lgamma(y + 1) once per set().
#pragma once
#include "special.h"

#define MXF_LIK_KIND_LOGIT 0       // the numbers of MXF_LIK_* (include/mxf_gp.h), for translation units that do not see that header
#define MXF_LIK_KIND_PROBIT 1
#define MXF_LIK_KIND_POISSON 2

#ifndef MXF_LIK_MAX_NODES
#define MXF_LIK_MAX_NODES 64       // as include/mxf_gp.h
#endif

// A Gauss-Hermite rule as the quadrature kernels take it, in their arguments: x_k = sqrt(2) node_k and w_k = weight_k / sqrt(pi), rounded to T
// once, zeros from nq up to MXF_LIK_MAX_NODES
template <typename T>
struct MxfQuadNodes { T x[MXF_LIK_MAX_NODES], w[MXF_LIK_MAX_NODES]; int nq; };

template <typename T>
inline MxfQuadNodes<T> mxf_quad_nodes(int nq, const double* nodes, const double* weights) {
    MxfQuadNodes<T> q;
    q.nq = nq;
    for (int k = 0; k < MXF_LIK_MAX_NODES; ++k) {
        q.x[k] = k < nq ? (T)(1.41421356237309504880 * nodes[k]) : (T)0;
        q.w[k] = k < nq ? (T)(0.56418958354775628695 * weights[k]) : (T)0;
    }
    return q;
}

// log sigmoid(z) and its first two derivatives in z
template <typename T>
MXF_HD inline void mxf_log_sigmoid(T z, T& l, T& d1, T& d2) {
    const T e = exp(-fabs(z)), r = (T)1 / ((T)1 + e);
    l = (z < (T)0 ? z : (T)0) - log1p(e);
    d1 = z < (T)0 ? r : e * r;              // sigmoid(-z)
    d2 = -e * r * r;                        // -sigmoid(z) sigmoid(-z)
}

template <typename T>
MXF_HD inline T mxf_sigmoid(T z) {
    const T e = exp(-fabs(z)), r = (T)1 / ((T)1 + e);
    return z < (T)0 ? e * r : r;
}

// z < 0: log Phi(z), lambda(z) and c = lambda(z) + z > 0, in double
MXF_HD inline void mxf_probit_left(double z, double& l, double& lam, double& c) {
    const double t = -z;
    if (t <= 5.0) {
        const double Phi = 0.5 * erfc(t * 0.70710678118654752440), phi = 0.39894228040143267794 * exp(-0.5 * t * t);
        l = log(Phi);
        lam = phi / Phi;
        c = lam * (1.0 - t * (Phi / phi));
    } else {
        const int n = 10 + (int)(450.0 / (t * t));
        c = 0.0;
        for (int k = n; k >= 1; --k) c = (double)k / (t + c);
        lam = t + c;
        l = -0.5 * t * t - 0.91893853320467274178 - log(lam);
    }
}

// log Phi(z) and its first two derivatives in z
template <typename T>
MXF_HD inline void mxf_log_ndtr(T z, T& l, T& d1, T& d2) {
    if (z < (T)0) {
        double ld, lam, c;
        mxf_probit_left((double)z, ld, lam, c);
        l = (T)ld; d1 = (T)lam; d2 = (T)(-lam * c);
    } else {
        const T q = (T)0.5 * erfc(z * (T)0.70710678118654752440), lam = (T)0.39894228040143267794 * exp((T)-0.5 * z * z) / ((T)1 - q);
        l = log1p(-q);
        d1 = lam;
        d2 = -lam * (z + lam);
    }
}

template <typename T>
MXF_HD inline T mxf_ndtr(T z) { return (T)0.5 * erfc(-z * (T)0.70710678118654752440); }

// Robust-max, the multi-class likelihood of robustmax.hip: one row of C latent values f_c ~ N(m_c, v) and a label y,
//   p = P(f_y is the largest) ~ sum_k w_k P_k,   P_k = prod_{c != y} Phi(z_kc),   z_kc = d_c + x_k,   d_c = (m_y - m_c) / sqrt(v_eff)
// with v_eff = max(v, MXF_ROBUSTMAX_V_FLOOR), x_k the nodes times sqrt 2 and w_k the weights over sqrt pi.  The derivatives are those of the
// sum itself: with lambda = phi / Phi and G_c = sum_k w_k P_k lambda(z_kc),
//   dp/dm_c = -G_c / sqrt(v_eff) (c != y),   dp/dm_y = sum_{c != y} G_c / sqrt(v_eff),   dp/dv = -sum_c G_c d_c / (2 v_eff)   (0 below the floor).
// P_k = exp(sum_c log Phi(z_kc)) from mxf_log_ndtr, never a product of Phi; a node whose P_k underflows to 0 adds nothing to any sum, so
// 0 * lambda is never formed.  With |m_y - m_c| <= 1e3 every intermediate is finite in float32: at the floor |z| <= 1e9, lambda <= 1e9 + 1 and
// log Phi >= -5e17 per class, -1.6e19 over 31 classes; P_k > 0 needs sum log Phi > -104, so |z| < 15 wherever a term is added, and
// G_c d_c / v_eff <= 15 * 1e9 * 1e12.  CP is C padded to a compile-time size so that the row lives in registers; a padded class enters no product.
#define MXF_ROBUSTMAX_V_FLOOR 1e-12

// one node: P_k of the row d at the node x; lam[c] = lambda(z_kc) of the classes in the product, 0 for y and for the padding
template <typename T, int CP>
MXF_HD inline T mxf_robustmax_node(int C, int y, const T* d, T x, T* lam) {
    T sl = 0;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        lam[c] = 0;
        if (c < C && c != y) {
            T l, d1, d2;
            mxf_log_ndtr<T>(d[c] + x, l, d1, d2);
            sl += l;
            lam[c] = d1;
        }
    }
    return exp(sl);
}

// one row: returns p; with GRAD, dpm[c] = dp/dm_c (CP entries, 0 in the padding) and dpv = dp/dv.  q holds x[], w[] and nq (scaled as above).
template <typename T, int CP, bool GRAD, typename Q>
MXF_HD inline T mxf_robustmax_row(int C, int y, const T* m, T v, const Q& q, T* dpm, T& dpv) {
    const bool floored = !(v >= (T)MXF_ROBUSTMAX_V_FLOOR);
    const T ve = floored ? (T)MXF_ROBUSTMAX_V_FLOOR : v, rs = (T)1 / sqrt(ve);
    T my = 0, d[CP], G[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) my = c == y ? m[c] : my;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        d[c] = c < C ? (my - m[c]) * rs : (T)0;
        G[c] = 0;
    }
    T p = 0;
    for (int k = 0; k < q.nq; ++k) {
        T lam[CP];
        const T P = mxf_robustmax_node<T, CP>(C, y, d, q.x[k], lam);
        if (P > (T)0) {
            const T wP = q.w[k] * P;
            p += wP;
            if (GRAD) {
#pragma unroll
                for (int c = 0; c < CP; ++c) G[c] += wP * lam[c];
            }
        }
    }
    if (GRAD) {
        T sy = 0, sv = 0;
#pragma unroll
        for (int c = 0; c < CP; ++c) {       // (G is 0 at y and in the padding)
            sy += G[c];
            sv += G[c] * d[c];
        }
#pragma unroll
        for (int c = 0; c < CP; ++c) dpm[c] = rs * (c == y ? sy : -G[c]);
        dpv = floored ? (T)0 : (T)-0.5 * sv / ve;
    }
    return p;
}

// One observation y: set() holds what does not depend on f, eval() gives g = log p(y | f), g' and g''.
template <typename T, int KIND>
struct MxfLik {
    T y;        // POISSON: the count; Bernoulli kinds: the sign 2y - 1
    double c;   // POISSON: lgamma(y + 1)

    MXF_HD inline void set(T y_) {
        if constexpr (KIND == MXF_LIK_KIND_POISSON) { y = y_; c = mxf_lgamma((double)y_ + 1.0); }
        else { y = (T)2 * y_ - (T)1; c = 0.0; }
    }

    MXF_HD inline void eval(T f, T& g, T& g1, T& g2) const {
        if constexpr (KIND == MXF_LIK_KIND_LOGIT) {
            mxf_log_sigmoid<T>(y * f, g, g1, g2);
            g1 *= y;
        } else if constexpr (KIND == MXF_LIK_KIND_PROBIT) {
            mxf_log_ndtr<T>(y * f, g, g1, g2);
            g1 *= y;
        } else {
            const double e = exp((double)f);
            g = (T)((double)y * (double)f - e - c);
            g1 = (T)((double)y - e);
            g2 = (T)(-e);
        }
    }

    MXF_HD static inline T mu(T f) {
        if constexpr (KIND == MXF_LIK_KIND_LOGIT) return mxf_sigmoid<T>(f);
        else if constexpr (KIND == MXF_LIK_KIND_PROBIT) return mxf_ndtr<T>(f);
        else return exp(f);
    }
};
