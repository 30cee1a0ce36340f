// Special functions of the univariate log-densities (univariate.hip) and of the Wishart density (wishart.hip): log-gamma and digamma for
// x > 0 and their multivariate forms, float and double, callable from host and device code -- the host side exists so that
// tests/host/special_check.cpp and tests/host/mvgamma_check.cpp can hold them to SciPy without a GPU.
// No tables in memory, no inline assembly.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MXF_HD __host__ __device__
#else
#define MXF_HD
#endif

// log Gamma(x), x > 0: the math library's (device: the device library's) own
MXF_HD inline float mxf_lgamma(float x) { return lgammaf(x); }
MXF_HD inline double mxf_lgamma(double x) { return lgamma(x); }

// psi(x) = d/dx log Gamma(x), x > 0.  psi(x) = psi(x + 1) - 1/x lifts the argument to x >= 6; there the asymptotic series
//   psi(x) ~ log x - 1/(2x) - sum_k B_2k / (2k x^2k)
// through B_20 is cut off below 854513/(3036 x^22) <= 2.2e-15 (4e-16 at x = 6.46, where the lift of psi's zero at 1.4616 lands: the value
// there is all cancellation, so the cut has to be small absolutely, not relative to psi(6) = 1.706).  The reciprocals of the lift are summed smallest first
// (the largest, 1/x, last), so for small x, where psi ~ -1/x, the sum carries one rounding of its dominant term.
template <typename T>
MXF_HD inline T mxf_digamma(T x) {
    int k = 0;
    while (k < 6 && x + (T)k < (T)6) ++k;
    const T y = x + (T)k;
    T lift = 0;
    for (int j = k - 1; j >= 0; --j) lift += (T)1 / (x + (T)j);
    const T r = (T)1 / y, r2 = r * r;
    T p = (T)(-174611.0 / 6600.0);          // B_20 / 20
    p = (T)(43867.0 / 14364.0) + r2 * p;    // B_18 / 18
    p = (T)(-3617.0 / 8160.0) + r2 * p;     // B_16 / 16
    p = (T)(1.0 / 12.0) + r2 * p;           // B_14 / 14
    p = (T)(-691.0 / 32760.0) + r2 * p;     // B_12 / 12
    p = (T)(1.0 / 132.0) + r2 * p;          // B_10 / 10
    p = (T)(-1.0 / 240.0) + r2 * p;         // B_8 / 8
    p = (T)(1.0 / 252.0) + r2 * p;          // B_6 / 6
    p = (T)(-1.0 / 120.0) + r2 * p;         // B_4 / 4
    p = (T)(1.0 / 12.0) + r2 * p;           // B_2 / 2
    return (log(y) - (T)0.5 * r - r2 * p) - lift;
}

// log Gamma_n(a) = n (n - 1) / 4 log pi + sum_{k=1..n} lgamma(a + (1 - k) / 2), a > (n - 1) / 2: the multivariate gamma function of the
// Wishart density (util/special.py:21-132 of the reference forms it element by element).  The terms run from lgamma(a) ~ a log a down to
// lgamma of the margin a - (n - 1) / 2, which is large again near zero: terms and sum are double for either T, and T sees one rounding,
// as univariate.hip does for its lgamma differences.
template <typename T>
MXF_HD inline T mxf_lmvgamma(T a, int n) {
    double s = 0.25 * n * (n - 1) * 1.1447298858494001741 /* log pi */;
    for (int k = 0; k < n; ++k) s += mxf_lgamma((double)a - 0.5 * k);
    return (T)s;
}

// d/da log Gamma_n(a) = sum_{k=1..n} psi(a + (1 - k) / 2): psi changes sign at 1.4616, so the sum cancels; double as above.
template <typename T>
MXF_HD inline T mxf_mvdigamma(T a, int n) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += mxf_digamma<double>((double)a - 0.5 * k);
    return (T)s;
}
