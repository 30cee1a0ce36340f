// Wishart log-density for thousands of small matrices (gfx950): order n <= 32, X (S|1, B, n, n) under V (S|1, B|1, n, n) and nu (S|1, B|1).
//   mxf_wishart_logpdf      one wavefront per row (s, b): its half-waves factorise X[s,b] and V side by side in LDS (lanes 0..31 and
//                           32..63, a tile each), lanes 0..n-1 form Y = L_V^-1 L_X a column each, tr(V^-1 X) = |Y|_F^2
//   mxf_wishart_logpdf_bwd  the same rows with the cotangent: both factors again (a few thousand FMAs), both inverses side by side,
//                           Z = L_V^-T Y, and X^-1, V^-1 and Z Z^T = V^-1 X V^-1 a row per lane; sums over shared axes are formed in
//                           double for either dtype
// The tiles are double for either dtype: a float32 operand is widened when it is loaded and a float32 result is rounded once.
// One wavefront per workgroup: four tiles are 33 KB of LDS, and a barrier is the wave's own.  Both calls are launch-bound at the sizes of
// a prior.
//
// Replaces: Wishart.log_pdf_impl (components/distributions/wishart.py:62-96) over the per-element loops of util/special.py:21-132
// (log_determinant, solve, trace, log_multivariate_gamma) and MXNet autograd through them.
#include "common.h"
#include "shared_grad.h"
#include "smallmat.h"
#include "special.h"

namespace {

constexpr int WISH_TILE = MVN_MAX * MVN_LD;
constexpr double WISH_LOG_2 = 0.69314718055994530942, WISH_LOG_PI = 1.1447298858494001741;

template <typename T>
struct WishRows {
    int S;
    int64_t B;
    int n;
    const T* X; int64_t ldx, ss_X;
    const T* dof; int64_t ss_d, sb_d;
    const T* V; int64_t ldv, ss_V, sb_V;
    int S_V; int64_t B_V;
    double scale;
};

// the row (s, b) of a wavefront after the factor step
struct WishRow {
    int64_t s, b;
    double nu, ldX, ldV;      // sum log diag of the two factors: half their log-determinants
    int fail;                 // the info word: 0, j + 1 (V), n + j + 1 (X), 2 n + 1 (nu <= n - 1); the first that applies
};

// Lower triangles of X[s,b] -> tx and of its V -> tv, then both Cholesky factors in place: lanes 0..31 hold X, lanes 32..63 hold V,
// lane c of a half the column c on the way in and the row c in the factor step.
template <typename T>
__device__ __forceinline__ WishRow wish_factor(const WishRows<T>& a, int64_t row, double* tx, double* tv, int lane) {
    const int half = lane >> 5, c = lane & 31, n = a.n;
    WishRow r;
    r.s = row / a.B;
    r.b = row % a.B;
    const bool mine = c < n;
    double* t = half ? tv : tx;
    if (mine) {
        const T* src = half ? a.V + (a.S_V == 1 ? 0 : r.s) * a.ss_V + (a.B_V == 1 ? 0 : r.b) * a.sb_V : a.X + r.s * a.ss_X + r.b * n * a.ldx;
        const int64_t ld = half ? a.ldv : a.ldx;
        for (int i = 0; i < n; ++i) t[i * MVN_LD + c] = c <= i ? (double)src[i * ld + c] : 0.0;
    }
    __syncthreads();
    int bad;
    const double ld = smallmat_cholesky<32>(t, n, c, mine, bad);
    r.ldX = __shfl(ld, 0, 64);
    r.ldV = __shfl(ld, 32, 64);
    const int badX = __shfl(bad, 0, 64), badV = __shfl(bad, 32, 64);
    r.nu = (double)a.dof[r.s * a.ss_d + r.b * a.sb_d];
    r.fail = badV ? badV : badX ? n + badX : !(r.nu > (double)(n - 1)) ? 2 * n + 1 : 0;
    return r;
}

// out[s,b] = scale * (1/2 [(nu - n - 1) log|X| - tr(V^-1 X) - nu n log 2 - nu log|V|] - log Gamma_n(nu / 2)); a failed row is NaN.
// log Gamma_n is mxf_lmvgamma's sum (special.h) with a term per lane.
template <typename T>
__global__ __launch_bounds__(64) void wishart_logpdf_kernel(WishRows<T> a, T* __restrict__ out, int* __restrict__ info) {
    __shared__ double tiles[2 * WISH_TILE];
    double *tx = tiles, *tv = tiles + WISH_TILE;
    const int lane = threadIdx.x, n = a.n;
    const int64_t rows = (int64_t)a.S * a.B;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const WishRow r = wish_factor(a, row, tx, tv, lane);
        const double q = wave_sum(lane < n ? smallmat_solve_lower(tv, tx, n, lane) : 0.0);
        const double lg = wave_sum(lane < n ? mxf_lgamma(0.5 * (r.nu - lane)) : 0.0) + 0.25 * n * (n - 1) * WISH_LOG_PI;
        if (lane == 0) {
            const double v = 0.5 * (2.0 * (r.nu - n - 1) * r.ldX - q - r.nu * n * WISH_LOG_2 - 2.0 * r.nu * r.ldV) - lg;
            out[row] = r.fail ? (T)NAN : (T)(a.scale * v);
            if (r.fail) info[row] = r.fail;
        }
        __syncthreads();                               // the tiles are loaded again on the next trip
    }
}

// A gradient whose operand is broadcast over an axis is summed over it with atomics into a DOUBLE accumulator (shared_grad.h); the others
// are read-modify-writes of elements this wavefront alone owns.
template <typename T>
__device__ __forceinline__ void wish_add(bool shared, T* dst, double* sum, int64_t e, double v) {
    if (shared) atomic_add(sum + e, v); else dst[e] += (T)v;
}

// With w = scale * cot[s,b] (NaN for a failed row):
//   dX += w [1/2 (nu - n - 1) X^-1 - 1/2 V^-1],   dV += w [1/2 V^-1 X V^-1 - 1/2 nu V^-1],
//   dnu += w [1/2 (log|X| - n log 2 - log|V|) - 1/2 sum_k psi((nu + 1 - k) / 2)]
// X^-1 = Wx^T Wx and V^-1 = Wv^T Wv from the inverted factors, V^-1 X V^-1 = Z Z^T with Z = Wv^T Y.  Tiles: tx holds L_X, then Y, then Z;
// tv L_V; ix Wx; iv Wv.  In the closing loop lane c of half h forms the rows j = h, h + 2, ... of column c of the three symmetric
// matrices (consecutive lanes, consecutive addresses).
template <typename T>
__global__ __launch_bounds__(64) void wishart_logpdf_bwd_kernel(WishRows<T> a, const T* __restrict__ cot, T* dX, T* ddof, T* dV, double* sX,
                                                                double* sd, double* sV) {
    __shared__ double tiles[4 * WISH_TILE];
    double *tx = tiles, *tv = tiles + WISH_TILE, *ix = tiles + 2 * WISH_TILE, *iv = tiles + 3 * WISH_TILE;
    const int lane = threadIdx.x, half = lane >> 5, c = lane & 31, n = a.n;
    const int64_t rows = (int64_t)a.S * a.B;
    const bool X_shared = shared_over(a.ss_X, true, a.S, a.B), d_shared = shared_over(a.ss_d, a.sb_d, a.S, a.B);
    const bool V_shared = shared_over(a.S_V != 1, a.B_V != 1, a.S, a.B);
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const WishRow r = wish_factor(a, row, tx, tv, lane);
        const double w = r.fail ? (double)NAN : a.scale * (double)cot[row];
        if (ddof) {
            const double psi = wave_sum(lane < n ? mxf_digamma<double>(0.5 * (r.nu - lane)) : 0.0);     // mxf_mvdigamma's sum, a term per lane
            if (lane == 0) {
                wish_add(d_shared, ddof, sd, shared_row(a.ss_d, a.sb_d, r.s, r.b, a.B, 1), w * (r.ldX - 0.5 * n * WISH_LOG_2 - r.ldV - 0.5 * psi));
            }
        }
        if (dX || dV) {
            if (half || dX) mvn_invert_lower(half ? tv : tx, half ? iv : ix, n, c);
            __syncthreads();                           // Wv is read across columns below
            if (dV && lane < n) {                      // column c of Y in place of L_X's, then of Z in place of Y's: Z_ic needs Y_kc for k >= i only
                smallmat_solve_lower(tv, tx, n, c);
                for (int i = 0; i < n; ++i) {
                    double acc = 0.0;
                    for (int k = i > c ? i : c; k < n; ++k) acc += iv[k * MVN_LD + i] * tx[k * MVN_LD + c];
                    tx[i * MVN_LD + c] = acc;
                }
            }
            __syncthreads();
            if (c < n) {
                const int64_t gX = shared_row(a.ss_X, true, r.s, r.b, a.B, n * n), gV = shared_row(a.S_V != 1, a.B_V != 1, r.s, r.b, a.B, n * n);
                for (int j = half; j < n; j += 2) {
                    double vinv = 0.0, xinv = 0.0, sand = 0.0;
                    for (int k = j > c ? j : c; k < n; ++k) vinv += iv[k * MVN_LD + j] * iv[k * MVN_LD + c];
                    if (dX) {
                        for (int k = j > c ? j : c; k < n; ++k) xinv += ix[k * MVN_LD + j] * ix[k * MVN_LD + c];
                        wish_add(X_shared, dX, sX, gX + j * n + c, w * (0.5 * (r.nu - n - 1) * xinv - 0.5 * vinv));
                    }
                    if (dV) {
                        for (int k = 0; k < n; ++k) sand += tx[j * MVN_LD + k] * tx[c * MVN_LD + k];
                        wish_add(V_shared, dV, sV, gV + j * n + c, w * (0.5 * sand - 0.5 * r.nu * vinv));
                    }
                }
            }
        }
        __syncthreads();                               // the tiles are loaded again on the next trip
    }
}

struct WishCall {
    int dtype, S; int64_t B; int n;
    const void* X; int64_t ldx, ss_X;
    const void* dof; int64_t ss_d, sb_d;
    const void* V; int64_t ldv, ss_V, sb_V; int S_V; int64_t B_V;
    double scale;
};

int check_common(mxf_handle h, const char* name, int dtype, int n) {
    if (dtype != MXF_F32 && dtype != MXF_F64) return mxf_bad_dtype(h, name, dtype);
    if (n < 1 || n > MVN_MAX) MXF_FAIL(h, -3, "%s: order n = %d is outside 1..%d (larger matrices take mxf_potrf / mxf_trsm)", name, n, MVN_MAX);
    return 0;
}

int check_rows(mxf_handle h, const char* name, const WishCall& c) {
    if (!c.X || !c.dof || !c.V) MXF_FAIL(h, -2, "%s: null operand", name);
    if ((c.S_V != 1 && c.S_V != c.S) || (c.B_V != 1 && c.B_V != c.B))
        MXF_FAIL(h, -2, "%s: the scale matrices have 1 or S samples and 1 or B batch entries, got (%d, %lld)", name, c.S_V, (long long)c.B_V);
    if (c.ldx < c.n || c.ldv < c.n) MXF_FAIL(h, -2, "%s: ldx %lld or ldv %lld < n = %d", name, (long long)c.ldx, (long long)c.ldv, c.n);
    if (c.ss_X < 0 || c.ss_d < 0 || c.sb_d < 0 || c.ss_V < 0 || c.sb_V < 0) MXF_FAIL(h, -2, "%s: negative stride", name);
    return 0;
}

template <typename T>
WishRows<T> rows_of(const WishCall& c) {
    return {.S = c.S, .B = c.B, .n = c.n, .X = (const T*)c.X, .ldx = c.ldx, .ss_X = c.ss_X, .dof = (const T*)c.dof, .ss_d = c.ss_d, .sb_d = c.sb_d,
            .V = (const T*)c.V, .ldv = c.ldv, .ss_V = c.ss_V, .sb_V = c.sb_V, .S_V = c.S_V, .B_V = c.B_V, .scale = c.scale};
}

// a workgroup (one wavefront) per row, grid-stride above 4096 rows
unsigned grid_of(const WishCall& c) {
    const int64_t rows = (int64_t)c.S * c.B;
    return (unsigned)(rows < 4096 ? rows : 4096);
}

// dX, ddof and dV where their operand is shared over an axis are summed in double (shared_grad.h)
template <typename T>
int launch_bwd(mxf_handle h, const WishCall& c, const void* cot, void* dX, void* ddof, void* dV, hipStream_t st) {
    const int64_t nn = (int64_t)c.n * c.n;
    const bool own_sV = c.S_V != 1, own_bV = c.B_V != 1;
    SharedSums sums;
    if (int rc = shared_sums_open<T>(h, "mxf_wishart_logpdf_bwd",
                                     {{dX, shared_over(c.ss_X, true, c.S, c.B) ? shared_numel(c.ss_X, true, c.S, c.B, nn) : 0},
                                      {ddof, shared_over(c.ss_d, c.sb_d, c.S, c.B) ? shared_numel(c.ss_d, c.sb_d, c.S, c.B, 1) : 0},
                                      {dV, shared_over(own_sV, own_bV, c.S, c.B) ? shared_numel(own_sV, own_bV, c.S, c.B, nn) : 0}},
                                     st, &sums))
        return rc;
    hipLaunchKernelGGL((wishart_logpdf_bwd_kernel<T>), dim3(grid_of(c)), dim3(64), 0, st, rows_of<T>(c), (const T*)cot, (T*)dX, (T*)ddof,
                       (T*)dV, sums.acc[0], sums.acc[1], sums.acc[2]);
    shared_sums_close(sums, st);
    return 0;
}

}  // namespace

extern "C" int mxf_wishart_logpdf(mxf_handle h, int dtype, int S, int64_t B, int n, const void* X, int64_t ldx, int64_t strideS_X,
                                  const void* dof, int64_t strideS_dof, int64_t strideB_dof, const void* V, int64_t ldv, int64_t strideS_V,
                                  int64_t strideB_V, int S_V, int64_t B_V, double scale, void* out, int* info, void* stream) {
    if (!h) return -1;
    const WishCall c = {.dtype = dtype, .S = S, .B = B, .n = n, .X = X, .ldx = ldx, .ss_X = strideS_X, .dof = dof, .ss_d = strideS_dof, .sb_d = strideB_dof,
                        .V = V, .ldv = ldv, .ss_V = strideS_V, .sb_V = strideB_V, .S_V = S_V, .B_V = B_V, .scale = scale};
    if (int rc = check_common(h, "mxf_wishart_logpdf", dtype, n)) return rc;
    if (S <= 0 || B <= 0) return 0;
    if (int rc = check_rows(h, "mxf_wishart_logpdf", c)) return rc;
    if (!out || !info) MXF_FAIL(h, -2, "mxf_wishart_logpdf: null out or info");
    return mxf_typed(h, "mxf_wishart_logpdf", dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((wishart_logpdf_kernel<T>), dim3(grid_of(c)), dim3(64), 0, (hipStream_t)stream, rows_of<T>(c), (T*)out, info);
    });
}

extern "C" int mxf_wishart_logpdf_bwd(mxf_handle h, int dtype, int S, int64_t B, int n, const void* X, int64_t ldx, int64_t strideS_X,
                                      const void* dof, int64_t strideS_dof, int64_t strideB_dof, const void* V, int64_t ldv,
                                      int64_t strideS_V, int64_t strideB_V, int S_V, int64_t B_V, const void* cot, double scale, void* dX_acc,
                                      void* ddof_acc, void* dV_acc, void* stream) {
    if (!h) return -1;
    const WishCall c = {.dtype = dtype, .S = S, .B = B, .n = n, .X = X, .ldx = ldx, .ss_X = strideS_X, .dof = dof, .ss_d = strideS_dof, .sb_d = strideB_dof,
                        .V = V, .ldv = ldv, .ss_V = strideS_V, .sb_V = strideB_V, .S_V = S_V, .B_V = B_V, .scale = scale};
    if (int rc = check_common(h, "mxf_wishart_logpdf_bwd", dtype, n)) return rc;
    if (S <= 0 || B <= 0) return 0;
    if (int rc = check_rows(h, "mxf_wishart_logpdf_bwd", c)) return rc;
    if (!cot) MXF_FAIL(h, -2, "mxf_wishart_logpdf_bwd: null cotangent");
    if (!dX_acc && !ddof_acc && !dV_acc) return 0;
    return mxf_typed(h, "mxf_wishart_logpdf_bwd", dtype, [&](auto t) { return launch_bwd<decltype(t)>(h, c, cot, dX_acc, ddof_acc, dV_acc, (hipStream_t)stream); });
}
