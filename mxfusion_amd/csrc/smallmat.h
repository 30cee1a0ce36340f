// Matrices of order n <= 32 in LDS, a lane per row or column: the tile layout, the Cholesky step and the triangular substitutions that
// mvn.hip and wishart.hip share.  Tiles are double for either dtype: a float32 result is rounded once, when it is stored.
// No inline assembly; every loop is bounded by n.
#pragma once
#include "common.h"

constexpr int MVN_MAX = 32;             // largest order: a lane per row (or column) of a matrix
constexpr int MVN_LD = MVN_MAX + 1;     // LDS row stride: lanes walking down a column fall into different banks

// the tiles of one matrix
struct MvnTiles { double l[MVN_MAX * MVN_LD]; double x[MVN_MAX * MVN_LD]; };

// x = l^-1 (both lower, in LDS) by forward substitution; lane c owns column c of x and touches no other, so no barrier is needed inside.
// Rows above the diagonal come out as exact zeros.  Lanes >= n stay out.
__device__ __forceinline__ void mvn_invert_lower(const double* l, double* x, int n, int lane) {
    if (lane >= n) return;
    for (int i = 0; i < n; ++i) {
        double acc = i == lane ? 1.0 : 0.0;
        for (int k = 0; k < i; ++k) acc -= l[i * MVN_LD + k] * x[k * MVN_LD + lane];
        x[i * MVN_LD + lane] = acc / l[i * MVN_LD + i];
    }
}

// y <- l^-1 y in place (both lower, in LDS), the same substitution with y's own column as right-hand side: lane c < n owns column c, whose
// rows above the diagonal are zeros and are skipped.  Returns the column's sum of squares.
__device__ __forceinline__ double smallmat_solve_lower(const double* l, double* y, int n, int c) {
    double q = 0.0;
    for (int i = c; i < n; ++i) {
        double acc = y[i * MVN_LD + c];
        for (int k = c; k < i; ++k) acc -= l[i * MVN_LD + k] * y[k * MVN_LD + c];
        acc /= l[i * MVN_LD + i];
        y[i * MVN_LD + c] = acc;
        q += acc * acc;
    }
    return q;
}

// The lower triangle in tile l -> its Cholesky factor, in place; returns sum_j log L_jj.  Left-looking, a column per step: lane i of a
// group of W lanes (64: the wavefront; 32: a half-wave with a tile of its own) forms A_ij - sum_k L_ik L_jk, lane j's value is the pivot;
// sums, pivots and the log-determinant are double.  A pivot that is not positive sets bad = j + 1 once and turns the rest of the factor and
// the log-determinant into NaN; nothing traps.  `mine`: this lane holds a row (i < n of a live matrix).  Holds a barrier per column, so
// every wave of the workgroup calls it with the same n; the factor is complete for every lane on return.
template <int W>
__device__ __forceinline__ double smallmat_cholesky(double* l, int n, int i, bool mine, int& bad) {
    double ld = 0.0;
    bad = 0;
    for (int j = 0; j < n; ++j) {
        double s = 0.0;
        if (mine && i >= j) {
            s = l[i * MVN_LD + j];
            for (int k = 0; k < j; ++k) s -= l[i * MVN_LD + k] * l[j * MVN_LD + k];
        }
        const double piv = __shfl(s, j, W);
        if (!(piv > 0.0) && !bad) bad = j + 1;
        const double d = bad ? (double)NAN : sqrt(piv);
        ld += log(d);
        if (mine && i >= j) l[i * MVN_LD + j] = i == j ? d : s / d;
        __syncthreads();
    }
    return ld;
}
