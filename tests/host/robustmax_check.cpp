// Prints the one-row robust-max functions of mxfusion_amd/csrc/likelihood.h at C = 3 (padded to 4, as the kernel holds it) in both precisions.
// Standard input: the number of nodes nq, then nq Gauss-Hermite nodes and nq weights (numpy's hermgauss as it comes; scaled here to
// sqrt(2) x and w / sqrt(pi) and rounded to T once, as the launcher does), then one "y v m0 m1 m2" line per point.  Per point:
//   p dm0 dm1 dm2 dv      first in double (%.17g), then in float (%.9g)
// tests/test_robustmax_host.py compiles this with the system C++ compiler and compares the columns with autograd on the float64
// restatement (tests/_robustmax_ref.py).
#include <stdio.h>

#include "likelihood.h"

#define MAX_NODES 64

template <typename T>
struct Nodes { T x[MAX_NODES], w[MAX_NODES]; int nq; };

template <typename T>
static void row(const Nodes<T>& q, int y, T v, const double* m, T* out) {
    T mr[4] = {(T)m[0], (T)m[1], (T)m[2], (T)0}, g[4], gv = 0;
    out[0] = mxf_robustmax_row<T, 4, true>(3, y, mr, v, q, g, gv);
    for (int c = 0; c < 3; ++c) out[1 + c] = g[c];
    out[4] = gv;
}

int main() {
    int nq;
    double x[MAX_NODES], w[MAX_NODES];
    if (scanf("%d", &nq) != 1 || nq < 1 || nq > MAX_NODES) return 1;
    for (int k = 0; k < nq; ++k) if (scanf("%lf", &x[k]) != 1) return 1;
    for (int k = 0; k < nq; ++k) if (scanf("%lf", &w[k]) != 1) return 1;
    Nodes<double> qd;
    Nodes<float> qf;
    qd.nq = qf.nq = nq;
    for (int k = 0; k < nq; ++k) {
        qd.x[k] = 1.41421356237309504880 * x[k];
        qd.w[k] = 0.56418958354775628695 * w[k];
        qf.x[k] = (float)qd.x[k];
        qf.w[k] = (float)qd.w[k];
    }
    int y;
    double v, m[3];
    while (scanf("%d %lf %lf %lf %lf", &y, &v, &m[0], &m[1], &m[2]) == 5) {
        double d[5];
        float f[5];
        row<double>(qd, y, v, m, d);
        row<float>(qf, y, (float)v, m, f);
        for (int i = 0; i < 5; ++i) printf("%.17g ", d[i]);
        for (int i = 0; i < 5; ++i) printf("%.9g ", (double)f[i]);
        printf("\n");
    }
    return 0;
}
