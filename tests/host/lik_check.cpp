// Prints the link functions of mxfusion_amd/csrc/likelihood.h in both precisions for every "kind y f" line read from standard input:
//   kind y f  g<double> g'<double> g''<double> mu<double>  (float)f  g<float> g'<float> g''<float> mu<float>
// tests/test_likelihood_host.py compiles this with the system C++ compiler and compares the columns with SciPy.
#include <stdio.h>

#include "likelihood.h"

template <typename T, int KIND>
static void row(double y, T f, T out[4]) {
    MxfLik<T, KIND> l;
    l.set((T)y);
    l.eval(f, out[0], out[1], out[2]);
    out[3] = MxfLik<T, KIND>::mu(f);
}

template <typename T>
static void by_kind(int kind, double y, T f, T out[4]) {
    if (kind == MXF_LIK_KIND_LOGIT) row<T, MXF_LIK_KIND_LOGIT>(y, f, out);
    else if (kind == MXF_LIK_KIND_PROBIT) row<T, MXF_LIK_KIND_PROBIT>(y, f, out);
    else row<T, MXF_LIK_KIND_POISSON>(y, f, out);
}

int main() {
    int kind;
    double y, f;
    while (scanf("%d %lf %lf", &kind, &y, &f) == 3) {
        double d[4];
        float s[4];
        const float ff = (float)f;
        by_kind<double>(kind, y, f, d);
        by_kind<float>(kind, y, ff, s);
        printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %.9g %.9g %.9g %.9g %.9g\n", kind, y, f, d[0], d[1], d[2], d[3], (double)ff, (double)s[0],
               (double)s[1], (double)s[2], (double)s[3]);
    }
    return 0;
}
