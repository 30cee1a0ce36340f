// Prints the element functions of mxfusion_amd/csrc/psi.h at Q = 1 in both precisions for every "mu s z z2 l var" line read from standard input:
// the Psi1 term var * psi1_term at (mu, s, z) and the psi2n term var^2 exp(-D) psi2_term at (mu, s, z, z2), each followed by its partial
// derivatives in mu, s, z (Psi2: z and z2), l and var, assembled from the sums V, M, U of one term exactly as the kernels assemble them:
//   P1 dmu ds dz dl dvar   P2 dmu ds dz dz2 dl dvar      first in double (%.17g), then in float (%.9g)
// tests/test_psi_host.py compiles this with the system C++ compiler and compares the columns with the float64 restatement (tests/_psi_ref.py).
#include <stdio.h>

#include "psi.h"

template <typename T>
static void row(T mu, T s, T z, T z2, T l, T var, T* out) {
    const T l2 = l * l;
    T a, c, ae;
    psi_row_q<T>(1, s, l2, a, c);
    T t = psi1_term<T, 1>(&mu, &a, c, &z, &ae);             // the weight of the term is 1: V = t, M = t ae, U = t ae^2
    out[0] = var * t;
    out[1] = var * psi_dmu<T>(1, t * ae);
    out[2] = var * psi_ds<T>(1, a, t * ae * ae, t);
    out[3] = var * t * ae;
    out[4] = (T)2 * l * var * psi_dl2_row<T>(1, a, s, l2, t * ae * ae, t);
    out[5] = t;
    psi_row_q<T>(2, s, l2, a, c);
    const T zbar = (T)0.5 * (z + z2), w = var * var * exp(-psi2_dist_q<T>(z, z2, l2));
    t = w * psi2_term<T, 1>(&mu, &a, c, &zbar, &ae);
    out[6] = t;
    out[7] = psi_dmu<T>(2, t * ae);
    out[8] = psi_ds<T>(2, a, t * ae * ae, t);
    out[9] = psi2_dz_pair<T>(t * ae, t, z, z2, l2, 0);
    out[10] = psi2_dz_pair<T>(t * ae, t, z, z2, l2, 1);
    out[11] = (T)2 * l * (psi_dl2_row<T>(2, a, s, l2, t * ae * ae, t) + psi2_dl2_pair<T>(t, z, z2, l2));
    out[12] = (T)2 * t / var;
}

int main() {
    double v[6];
    while (scanf("%lf %lf %lf %lf %lf %lf", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
        double d[13];
        float f[13];
        row<double>(v[0], v[1], v[2], v[3], v[4], v[5], d);
        row<float>((float)v[0], (float)v[1], (float)v[2], (float)v[3], (float)v[4], (float)v[5], f);
        for (int i = 0; i < 13; ++i) printf("%.17g ", d[i]);
        for (int i = 0; i < 13; ++i) printf("%.9g ", (double)f[i]);
        printf("\n");
    }
    return 0;
}
