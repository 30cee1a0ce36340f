// Prints mxf_lgamma and mxf_digamma (mxfusion_amd/csrc/special.h) in both precisions for every x > 0 read from standard input, one per line:
//   x  lgamma<double>  digamma<double>  (float)x  lgamma<float>  digamma<float>
// tests/test_univariate_host.py compiles this with the system C++ compiler and compares the columns with SciPy.
#include <stdio.h>

#include "special.h"

int main() {
    double x;
    while (scanf("%lf", &x) == 1) {
        const float xf = (float)x;
        printf("%.17g %.17g %.17g %.9g %.9g %.9g\n", x, mxf_lgamma(x), mxf_digamma<double>(x), (double)xf, (double)mxf_lgamma(xf),
               (double)mxf_digamma<float>(xf));
    }
    return 0;
}
