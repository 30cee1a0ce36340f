// Prints the element functions of mxfusion_amd/csrc/rff.h at Q = 2 in both precisions for every "x0 x1 om0 om1 b gw" line read from standard
// input: the feature cos(x . omega + b) and the two sums rff_feature_bwd adds to, sin(x . omega + b) gw omega_q, which the kernel negates:
//   c s0 s1      first in double (%.17g), then in float (%.9g)
// tests/test_pathwise_host.py compiles this with the system C++ compiler and compares the columns with the float64 restatement.
#include <stdio.h>

#include "rff.h"

template <typename T>
static void row(const double* v, T* out) {
    const T x[2] = {(T)v[0], (T)v[1]}, om[2] = {(T)v[2], (T)v[3]};
    out[0] = rff_feature<T, 2>(x, om, (T)v[4]);
    out[1] = out[2] = 0;
    rff_feature_bwd<T, 2>(x, om, (T)v[4], (T)v[5], out + 1);
}

int main() {
    double v[6];
    while (scanf("%lf %lf %lf %lf %lf %lf", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6) {
        double d[3];
        float f[3];
        row<double>(v, d);
        row<float>(v, f);
        for (int i = 0; i < 3; ++i) printf("%.17g ", d[i]);
        for (int i = 0; i < 3; ++i) printf("%.9g ", (double)f[i]);
        printf("\n");
    }
    return 0;
}
