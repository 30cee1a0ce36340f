// Prints the per-pair math of mxfusion_amd/csrc/gram_diff.h in both precisions for every line read from standard input:
//   kind Q A ard  tau[Q]  p0[A]  p1[n1]  p2[n2]        (A = 1 unless kind is MXF_KD_SM; n1, n2 as the operands of mxf_gram_diff: Q or 1; A Q)
//     ->  K  dK/dtau[Q]  dK/dp0[A]  dK/dp1[n1]  dK/dp2[n2]      first in double (%.17g), then in float (%.9g)
// assembled from gd_prepare, gd_grad and gd_finish exactly as the kernels of gram_diff.hip assemble them (cotangent 1; gd_value is printed
// last, once per precision, and must equal K).  tests/test_gram_diff_host.py compiles this with the system C++ compiler and compares the
// columns with the float64 restatement (tests/_gram_diff_ref.py).  What runs here are the header's default transcendentals (libm, radians); the
// float32 forms the kernels substitute (gram_diff.hip: the hardware sine and cosine in revolutions, exp2 of a pre-scaled argument) exist on the
// device only and are covered by tests/test_gpu_gram_diff.py alone.
#include <stdio.h>

#include <vector>

#include "gram_diff.h"

template <typename T, int KIND, int QT>
static void pair(int Q, int A, int ard, const double* in, const char* fmt) {
    std::vector<T> v;
    const int n1 = KIND == MXF_KD_SM ? A * Q : (ard ? Q : 1), n2 = KIND == MXF_KD_SM ? A * Q : (KIND == MXF_KD_RQ ? 1 : n1);
    for (int i = 0; i < Q + A + n1 + n2; ++i) v.push_back((T)in[i]);
    const T *tau_in = v.data(), *p0 = tau_in + Q, *p1 = p0 + A, *p2 = p1 + n1;
    T tau[QT], K = 0, Kv = 0, dtau[QT];
    std::vector<T> d0(A), d1(n1, (T)0), d2(n2, (T)0);
    for (int q = 0; q < QT; ++q) { tau[q] = q < Q ? tau_in[q] : (T)0; dtau[q] = 0; }
    for (int c = 0; c < A; ++c) {
        GdComp<T, QT> cc;
        const int off = KIND == MXF_KD_SM ? c * Q : 0;
        gd_prepare<T, KIND, QT>(Q, KIND == MXF_KD_SM ? 1 : ard, p0[c], p1 + off, p2 + off, cc);
        T dt[QT], t1[QT], t2[QT];
        const T k = gd_grad<T, KIND, QT>(tau, cc, dt, t1, t2);
        K = fma(cc.amp, k, K);
        Kv = fma(cc.amp, gd_value<T, KIND, QT>(tau, cc), Kv);
        d0[c] = k;
        const bool ard1 = KIND == MXF_KD_SM || ard, ard2 = KIND == MXF_KD_SM || (KIND == MXF_KD_PERIODIC && ard);
        for (int q = 0; q < Q; ++q) {
            dtau[q] += cc.amp * dt[q];
            d1[off + (ard1 ? q : 0)] += gd_finish<T, KIND>(1, cc.amp, p1[off + (ard1 ? q : 0)], (T)1, t1[q]);
            if (KIND != MXF_KD_RQ || q == 0) d2[off + (ard2 ? q : 0)] += gd_finish<T, KIND>(2, cc.amp, (T)1, p2[off + (ard2 ? q : 0)], t2[q]);
        }
    }
    printf(fmt, (double)K);
    for (int q = 0; q < Q; ++q) printf(fmt, (double)dtau[q]);
    for (T x : d0) printf(fmt, (double)x);
    for (T x : d1) printf(fmt, (double)x);
    for (T x : d2) printf(fmt, (double)x);
    printf(fmt, (double)Kv);
}

template <typename T>
static int any(int kind, int Q, int A, int ard, const double* in, const char* fmt) {
    if (kind == MXF_KD_PERIODIC) pair<T, MXF_KD_PERIODIC, MXF_GD_MAX_Q>(Q, 1, ard, in, fmt);
    else if (kind == MXF_KD_RQ) pair<T, MXF_KD_RQ, MXF_GD_MAX_Q>(Q, 1, ard, in, fmt);
    else if (kind == MXF_KD_SM) pair<T, MXF_KD_SM, MXF_GD_SM_MAX_Q>(Q, A, ard, in, fmt);
    else return 1;
    return 0;
}

int main() {
    int kind, Q, A, ard;
    while (scanf("%d %d %d %d", &kind, &Q, &A, &ard) == 4) {
        const bool sm = kind == MXF_KD_SM;
        if (Q < 1 || Q > (sm ? MXF_GD_SM_MAX_Q : MXF_GD_MAX_Q) || A < 1 || A > (sm ? MXF_GD_SM_MAX_A : 1)) return 1;
        const int n1 = sm ? A * Q : (ard ? Q : 1), n2 = sm ? A * Q : (kind == MXF_KD_RQ ? 1 : n1), n = Q + A + n1 + n2;
        std::vector<double> in((size_t)n);
        for (int i = 0; i < n; ++i) if (scanf("%lf", &in[(size_t)i]) != 1) return 1;
        if (any<double>(kind, Q, A, ard, in.data(), "%.17g ") || any<float>(kind, Q, A, ard, in.data(), "%.9g ")) return 1;
        printf("\n");
    }
    return 0;
}
