// Multivariate normal log-density for thousands of small matrices (gfx950): order n <= 32, covariance or precision form.
//   mxf_mvn_factor      one wavefront per DISTINCT matrix factorises it in LDS and leaves L^-1 (precision form: L) and sum log L_ii
//   mxf_mvn_logpdf      one half-wave per row (s, b): lane i holds component i, the matrix-vector product runs on shuffles
//   mxf_mvn_logpdf_bwd  the same rows with the cotangent, + one wavefront per distinct matrix for the separable -1/2 (sum w) K^-1 term;
//                       sums over shared axes are formed in double for either dtype
// All three are launch-bound at the sizes of a prior or of a variational posterior (a few microseconds of arithmetic per launch).
//
// Replaces: MultivariateNormal.log_pdf_impl (components/distributions/normal.py:157-178), MultivariateNormalMeanPrecision.log_pdf_impl
// (normal.py:369-394) and MXNet autograd through linalg.potrf / linalg.trsm / linalg.sumlogdiag on (S, B, n, n) operands.
#include "common.h"
#include "shared_grad.h"
#include "smallmat.h"

namespace {

constexpr int MVN_WAVES = 4;            // wavefronts (matrices) per workgroup of the per-matrix kernels
constexpr int MVN_ROWS = 8;             // half-waves (rows) per workgroup of the per-row kernels

// Matrix m = sa * B_A + ba of A (S_A, B_A, n, n) -> F[m] (n x n, dense) and logdet[m].  Left-looking Cholesky, a column per step
// (smallmat_cholesky): sums, pivots and the log-determinant are double for either T.  A pivot that is not positive sets info[m] = j + 1
// once and turns the rest of the matrix and its log-determinant into NaN; nothing traps, every loop is bounded by n.
// Every wave of a workgroup takes the same number of trips (the barriers are reached by all four); a wave without a matrix loads and
// stores nothing.
template <typename T>
__global__ __launch_bounds__(256) void mvn_factor_kernel(int form, int64_t M, int64_t B_A, int n, const T* __restrict__ A, int64_t lda,
                                                         int64_t ss_A, int64_t sb_A, T* __restrict__ F, T* __restrict__ logdet,
                                                         int* __restrict__ info) {
    __shared__ MvnTiles tiles[MVN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* l = tiles[wave].l;
    double* x = tiles[wave].x;
    for (int64_t base = (int64_t)blockIdx.x * MVN_WAVES; base < M; base += (int64_t)gridDim.x * MVN_WAVES) {
        const int64_t m = base + wave;
        const bool live = m < M, mine = live && lane < n;
        if (mine) {
            const T* a = A + (m / B_A) * ss_A + (m % B_A) * sb_A;
            for (int i = 0; i < n; ++i) l[i * MVN_LD + lane] = lane <= i ? (double)a[(int64_t)i * lda + lane] : 0.0;
        }
        __syncthreads();
        int bad;
        const double ld = smallmat_cholesky<64>(l, n, lane, mine, bad);
        if (form == 0) mvn_invert_lower(l, x, n, mine ? lane : n);
        if (mine) {
            const double* src = form == 0 ? x : l;          // x: this lane's own column; l: complete since the last barrier
            T* f = F + m * n * n;
            for (int i = 0; i < n; ++i) f[i * n + lane] = lane <= i ? (T)src[i * MVN_LD + lane] : (T)0;
        }
        if (live && lane == 0) {
            logdet[m] = (T)ld;
            if (bad) info[m] = bad;
        }
        __syncthreads();                               // the tiles are loaded again on the next trip
    }
}

template <typename T>
struct MvnRows {
    int form, S;
    int64_t B;
    int n;
    const T* x; int64_t ss_x;
    const T* mean; int64_t ss_m, sb_m;
    const T* F; const T* logdet;
    int S_A; int64_t B_A;
    T scale;
};

// y_i = sum_k F[i][k] v_k, or (transposed) sum_k F[k][i] v_k, over a half-wave: lane i holds v_i and gets y_i.  F's upper triangle holds
// zeros, so the sums run over all k.  All 32 lanes take part in the shuffles; only lanes `on` (i < n of a live row) load.
template <typename T>
__device__ __forceinline__ T mvn_matvec(const T* __restrict__ F, bool transposed, T v, int n, int i, bool on) {
    T acc = 0;
    for (int k = 0; k < n; ++k) {
        const T vk = __shfl(v, k, 32);
        if (on) acc += (transposed ? F[k * n + i] : F[i * n + k]) * vk;
    }
    return acc;
}

// the row (s, b) of a half-wave: its matrix, and d_i = x_i - mean_i in lane i
template <typename T>
struct MvnRow {
    bool live, on;
    int64_t s, b, m;
    T d;
    __device__ __forceinline__ MvnRow(const MvnRows<T>& a, int64_t r, int64_t rows, int i) {
        live = r < rows;
        on = live && i < a.n;
        s = live ? r / a.B : 0;
        b = live ? r % a.B : 0;
        m = (a.S_A == 1 ? 0 : s) * a.B_A + (a.B_A == 1 ? 0 : b);
        d = on ? a.x[s * a.ss_x + b * a.n + i] - a.mean[s * a.ss_m + b * a.sb_m + i] : (T)0;
    }
};

// out[s,b] = scale * (-1/2 |z|^2 -+ logdet - c),  z = L^-1 d (covariance form) or L^T d (precision form),  c = n/2 log 2 pi
template <typename T>
__global__ __launch_bounds__(256) void mvn_logpdf_kernel(MvnRows<T> a, T c, T* __restrict__ out) {
    const int i = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const int64_t rows = (int64_t)a.S * a.B;
    for (int64_t base = (int64_t)blockIdx.x * MVN_ROWS; base < rows; base += (int64_t)gridDim.x * MVN_ROWS) {
        const MvnRow<T> row(a, base + sub, rows, i);
        const T z = mvn_matvec(a.F + row.m * a.n * a.n, a.form == 1, row.d, a.n, i, row.on);
        T q = z * z;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 32);
        if (row.live && i == 0) {
            const T ld = a.logdet[row.m];
            out[base + sub] = a.scale * ((T)-0.5 * q + (a.form == 1 ? ld : -ld) - c);
        }
    }
}

// With w = scale * cot[s,b] and alpha = K^-1 d:  dx -= w alpha,  dmean += w alpha,  dA += 1/2 w alpha alpha^T (covariance form) or
// -1/2 w d d^T (precision form).  A gradient whose operand is broadcast over an axis is summed over it with atomics into a DOUBLE
// accumulator (sx, sm, sA: shared_grad.h); the others are plain read-modify-writes of elements this half-wave alone owns.  The term in
// K^-1 is mvn_inverse_bwd_kernel's.
template <typename T>
__global__ __launch_bounds__(256) void mvn_logpdf_bwd_kernel(MvnRows<T> a, const T* __restrict__ cot, T* dx, T* dmean, T* dA, double* sx,
                                                             double* sm, double* sA) {
    const int i = threadIdx.x & 31, sub = threadIdx.x >> 5, n = a.n;
    const int64_t rows = (int64_t)a.S * a.B;
    const bool x_shared = shared_over(a.ss_x, true, a.S, a.B), m_shared = shared_over(a.ss_m, a.sb_m, a.S, a.B);
    const bool A_shared = shared_over(a.S_A != 1, a.B_A != 1, a.S, a.B);
    // dmean's row index, shared_row(ss_m, sb_m, s, b, B, n), is linear in (s, b): its two steps, taken once (in the loop it costs the
    // double kernel two scalar registers and a wave of occupancy)
    const int64_t ds_m = shared_row(a.ss_m, a.sb_m, 1, 0, a.B, n), db_m = shared_row(a.ss_m, a.sb_m, 0, 1, a.B, n);
    for (int64_t base = (int64_t)blockIdx.x * MVN_ROWS; base < rows; base += (int64_t)gridDim.x * MVN_ROWS) {
        const MvnRow<T> row(a, base + sub, rows, i);
        const T* Fm = a.F + row.m * n * n;
        const T w = row.live ? a.scale * cot[base + sub] : (T)0;
        const T z = mvn_matvec(Fm, a.form == 1, row.d, n, i, row.on);
        const T alpha = mvn_matvec(Fm, a.form == 0, z, n, i, row.on);       // L^-T z, or L z
        if (row.on && dx) {
            const int64_t e = shared_row(a.ss_x, true, row.s, row.b, a.B, n) + i;
            if (x_shared) atomic_add(sx + e, (double)(-w * alpha)); else dx[e] -= w * alpha;
        }
        if (row.on && dmean) {
            const int64_t e = row.s * ds_m + row.b * db_m + i;
            if (m_shared) atomic_add(sm + e, (double)(w * alpha)); else dmean[e] += w * alpha;
        }
        if (dA) {
            const T u = a.form == 0 ? alpha : row.d, hw = a.form == 0 ? (T)0.5 * w : (T)-0.5 * w;
            const int64_t g = row.m * n * n;
            for (int j = 0; j < n; ++j) {
                const T uj = __shfl(u, j, 32);
                if (row.on) {                                                // row j of a symmetric matrix: consecutive lanes, consecutive addresses
                    if (A_shared) atomic_add(sA + g + j * n + i, (double)(hw * u * uj)); else dA[g + j * n + i] += hw * u * uj;
                }
            }
        }
    }
}

// dA[m] -+= 1/2 W_m K_m^-1 with W_m = scale * (sum of cot over the rows that use matrix m), once per distinct matrix: a wavefront per
// matrix as in mvn_factor_kernel.  K^-1 = X^T X with X = L^-1: F itself (covariance form) or inverted here from F = L (precision form).
// fold (float32 with shared matrices): the per-row terms that mvn_logpdf_bwd_kernel summed in double, added here before the one rounding.
template <typename T>
__global__ __launch_bounds__(256) void mvn_inverse_bwd_kernel(int form, int S, int64_t B, int n, const T* __restrict__ F, int S_A,
                                                              int64_t B_A, const T* __restrict__ cot, double scale, T* dA,
                                                              const double* fold) {
    __shared__ MvnTiles tiles[MVN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* l = tiles[wave].l;
    double* x = tiles[wave].x;
    const int64_t M = (int64_t)S_A * B_A;
    for (int64_t base = (int64_t)blockIdx.x * MVN_WAVES; base < M; base += (int64_t)gridDim.x * MVN_WAVES) {
        const int64_t m = base + wave;
        const bool live = m < M, mine = live && lane < n;
        double W = 0;
        if (live) {
            const int64_t s0 = S_A == 1 ? 0 : m / B_A, ns = S_A == 1 ? S : 1, b0 = B_A == 1 ? 0 : m % B_A, nb = B_A == 1 ? B : 1;
            for (int64_t t = lane; t < ns * nb; t += 64) W += (double)cot[(s0 + t / nb) * B + b0 + t % nb];
        }
        W = wave_sum(W) * scale;
        if (mine) {
            const T* f = F + m * n * n;
            double* dst = form == 0 ? x : l;
            for (int i = 0; i < n; ++i) dst[i * MVN_LD + lane] = (double)f[i * n + lane];
        }
        __syncthreads();
        if (form == 1) mvn_invert_lower(l, x, n, mine ? lane : n);
        __syncthreads();                               // lane i reads the columns of the other lanes below
        if (mine) {
            const int64_t g = m * n * n;
            const double hw = form == 0 ? -0.5 * W : 0.5 * W;
            for (int j = 0; j < n; ++j) {
                double acc = 0;
                for (int k = 0; k < n; ++k) acc += x[k * MVN_LD + lane] * x[k * MVN_LD + j];
                acc *= hw;
                if (fold) acc += fold[g + j * n + lane];
                dA[g + j * n + lane] += (T)acc;
            }
        }
        __syncthreads();
    }
}

int check_common(mxf_handle h, const char* name, int dtype, int form, int n) {
    if (dtype != MXF_F32 && dtype != MXF_F64) return mxf_bad_dtype(h, name, dtype);
    if (form != 0 && form != 1) MXF_FAIL(h, -2, "%s: form is 0 (covariance) or 1 (precision), got %d", name, form);
    if (n < 1 || n > MVN_MAX) MXF_FAIL(h, -3, "%s: order n = %d is outside 1..%d (larger matrices take mxf_potrf / mxf_trsm)", name, n, MVN_MAX);
    return 0;
}

struct MvnCall {
    int dtype, form, S; int64_t B; int n;
    const void* x; int64_t ss_x;
    const void* mean; int64_t ss_m, sb_m;
    const void *F, *logdet; int S_A; int64_t B_A;
    double scale;
};

int check_rows(mxf_handle h, const char* name, const MvnCall& c) {
    if (int rc = check_common(h, name, c.dtype, c.form, c.n)) return rc;
    if (!c.x || !c.mean || !c.F) MXF_FAIL(h, -2, "%s: null operand", name);
    if ((c.S_A != 1 && c.S_A != c.S) || (c.B_A != 1 && c.B_A != c.B))
        MXF_FAIL(h, -2, "%s: the matrices have 1 or S samples and 1 or B batch entries, got (%d, %lld)", name, c.S_A, (long long)c.B_A);
    if (c.ss_x < 0 || c.ss_m < 0 || c.sb_m < 0) MXF_FAIL(h, -2, "%s: negative stride", name);
    return 0;
}

template <typename T>
MvnRows<T> rows_of(const MvnCall& c) {
    return {.form = c.form, .S = c.S, .B = c.B, .n = c.n, .x = (const T*)c.x, .ss_x = c.ss_x, .mean = (const T*)c.mean, .ss_m = c.ss_m, .sb_m = c.sb_m,
            .F = (const T*)c.F, .logdet = (const T*)c.logdet, .S_A = c.S_A, .B_A = c.B_A, .scale = (T)c.scale};
}

template <typename T>
void launch_logpdf(const MvnCall& c, void* out, hipStream_t st) {
    const int64_t rows = (int64_t)c.S * c.B;
    hipLaunchKernelGGL((mvn_logpdf_kernel<T>), dim3(grid_for(rows * 32)), dim3(256), 0, st, rows_of<T>(c), (T)(0.5 * c.n * 1.8378770664093454836 /* log 2 pi */), (T*)out);
}

// dx, dmean and dA where their operand is shared over an axis are summed in double (shared_grad.h); mvn_inverse_bwd_kernel adds dA's float32
// sums itself, before its own rounding.
template <typename T>
int launch_bwd(mxf_handle h, const MvnCall& c, const void* cot, void* dx, void* dmean, void* dA, hipStream_t st) {
    const int64_t rows = (int64_t)c.S * c.B, n = c.n;
    const bool own_sA = c.S_A != 1, own_bA = c.B_A != 1;
    SharedSums sums;
    if (int rc = shared_sums_open<T>(h, "mxf_mvn_logpdf_bwd",
                                     {{dx, shared_over(c.ss_x, true, c.S, c.B) ? shared_numel(c.ss_x, true, c.S, c.B, n) : 0},
                                      {dmean, shared_over(c.ss_m, c.sb_m, c.S, c.B) ? shared_numel(c.ss_m, c.sb_m, c.S, c.B, n) : 0},
                                      {dA, shared_over(own_sA, own_bA, c.S, c.B) ? shared_numel(own_sA, own_bA, c.S, c.B, n * n) : 0, true}},
                                     st, &sums))
        return rc;
    hipLaunchKernelGGL((mvn_logpdf_bwd_kernel<T>), dim3(grid_for(rows * 32)), dim3(256), 0, st, rows_of<T>(c), (const T*)cot, (T*)dx,
                       (T*)dmean, (T*)dA, sums.acc[0], sums.acc[1], sums.acc[2]);
    if (dA)
        hipLaunchKernelGGL((mvn_inverse_bwd_kernel<T>), dim3(grid_for((int64_t)c.S_A * c.B_A * 64)), dim3(256), 0, st, c.form, c.S, c.B, c.n,
                           (const T*)c.F, c.S_A, c.B_A, (const T*)cot, c.scale, (T*)dA, sizeof(T) == 4 ? (const double*)sums.acc[2] : nullptr);
    shared_sums_close(sums, st);
    return 0;
}

}  // namespace

extern "C" int mxf_mvn_factor(mxf_handle h, int dtype, int form, int S_A, int64_t B_A, int n, const void* A, int64_t lda, int64_t strideS_A,
                              int64_t strideB_A, void* F, void* logdet, int* info, void* stream) {
    if (!h) return -1;
    if (int rc = check_common(h, "mxf_mvn_factor", dtype, form, n)) return rc;
    if (S_A <= 0 || B_A <= 0) return 0;
    if (!A || !F || !logdet || !info) MXF_FAIL(h, -2, "mxf_mvn_factor: null operand");
    if (lda < n || strideS_A < 0 || strideB_A < 0) MXF_FAIL(h, -2, "mxf_mvn_factor: lda %lld < n = %d, or a negative stride", (long long)lda, n);
    const int64_t M = (int64_t)S_A * B_A;
    return mxf_typed(h, "mxf_mvn_factor", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((mvn_factor_kernel<T>), dim3(grid_for(M * 64)), dim3(256), 0, (hipStream_t)stream, form, M, B_A, n, (const T*)A, lda, strideS_A,
                           strideB_A, (T*)F, (T*)logdet, info);
    });
}

extern "C" int mxf_mvn_logpdf(mxf_handle h, int dtype, int form, int S, int64_t B, int n, const void* x, int64_t strideS_x, const void* mean,
                              int64_t strideS_mean, int64_t strideB_mean, const void* F, const void* logdet, int S_A, int64_t B_A,
                              double scale, void* out, void* stream) {
    if (!h) return -1;
    const MvnCall c = {.dtype = dtype, .form = form, .S = S, .B = B, .n = n, .x = x, .ss_x = strideS_x, .mean = mean, .ss_m = strideS_mean,
                       .sb_m = strideB_mean, .F = F, .logdet = logdet, .S_A = S_A, .B_A = B_A, .scale = scale};
    if (int rc = check_common(h, "mxf_mvn_logpdf", dtype, form, n)) return rc;
    if (S <= 0 || B <= 0) return 0;
    if (int rc = check_rows(h, "mxf_mvn_logpdf", c)) return rc;
    if (!out || !logdet) MXF_FAIL(h, -2, "mxf_mvn_logpdf: null out or logdet");
    return mxf_typed(h, "mxf_mvn_logpdf", dtype, [&](auto t) { launch_logpdf<decltype(t)>(c, out, (hipStream_t)stream); });
}

extern "C" int mxf_mvn_logpdf_bwd(mxf_handle h, int dtype, int form, int S, int64_t B, int n, const void* x, int64_t strideS_x,
                                  const void* mean, int64_t strideS_mean, int64_t strideB_mean, const void* F, int S_A, int64_t B_A,
                                  const void* cot, double scale, void* dx_acc, void* dmean_acc, void* dA_acc, void* stream) {
    if (!h) return -1;
    const MvnCall c = {.dtype = dtype, .form = form, .S = S, .B = B, .n = n, .x = x, .ss_x = strideS_x, .mean = mean, .ss_m = strideS_mean,
                       .sb_m = strideB_mean, .F = F, .S_A = S_A, .B_A = B_A, .scale = scale};
    if (int rc = check_common(h, "mxf_mvn_logpdf_bwd", dtype, form, n)) return rc;
    if (S <= 0 || B <= 0) return 0;
    if (int rc = check_rows(h, "mxf_mvn_logpdf_bwd", c)) return rc;
    if (!cot) MXF_FAIL(h, -2, "mxf_mvn_logpdf_bwd: null cotangent");
    if (!dx_acc && !dmean_acc && !dA_acc) return 0;
    return mxf_typed(h, "mxf_mvn_logpdf_bwd", dtype, [&](auto t) { return launch_bwd<decltype(t)>(h, c, cot, dx_acc, dmean_acc, dA_acc, (hipStream_t)stream); });
}
