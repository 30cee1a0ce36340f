// Prints mxf_lmvgamma and mxf_mvdigamma (mxfusion_amd/csrc/special.h) in both precisions for every pair "n a" (a > (n - 1) / 2) read from
// standard input, one per line:
//   n  a  lmvgamma<double>  mvdigamma<double>  (float)a  lmvgamma<float>  mvdigamma<float>
// tests/test_wishart_host.py compiles this with the system C++ compiler and compares the columns with SciPy.
#include <stdio.h>

#include "special.h"

int main() {
    int n;
    double a;
    while (scanf("%d %lf", &n, &a) == 2) {
        const float af = (float)a;
        printf("%d %.17g %.17g %.17g %.9g %.9g %.9g\n", n, a, mxf_lmvgamma<double>(a, n), mxf_mvdigamma<double>(a, n), (double)af,
               (double)mxf_lmvgamma<float>(af, n), (double)mxf_mvdigamma<float>(af, n));
    }
    return 0;
}
