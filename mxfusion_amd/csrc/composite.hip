// Fused composites: one C-ABI call = one reference `compute` body (value + reverse mode), gfx950.
//
//   mxf_gp_logpdf   <- GPRegressionLogPdf.compute        (modules/gp_modules/gp_regression.py:42-76)
//   mxf_svgp_logpdf <- SVGPRegressionLogPdf.compute      (modules/gp_modules/svgp_regression.py:43-109)
//
// The reference gets gradients from MXNet autograd through potrf/trsm; here the reverse mode is closed
// form (matrix-calculus identities with K^-1 from the Cholesky factor), so every O(n^3) piece is an MFMA
// GEMM and no reverse-mode Cholesky is needed.
//
// SVGP is evaluated in the streaming sufficient-statistics form.  With Ki = Kuu^-1,
// H0 = Ki - Ki Su Ki,  w = Ki mu,  k_n = Kuf[:, n],  beta = 1/noise:
//     l_s   = -B P/2 (log 2pi + log noise) - P beta B var/2 - beta/2 sum_n |y_n - w^T k_n|^2
//             + P beta/2 sum_n k_n^T H0 k_n
//     logL_s = scaling * l_s + negKL,
//     negKL = P/2 (M + logdet Su - logdet Kuu - tr(Ki Su)) - 1/2 tr(mu^T Ki mu)
// All samples' columns are laid side by side (Kuf_all : M x (S*B)), so the data term is TWO big MFMA
// GEMMs ( [H0; w^T] * Kuf_all and Kuf_all * Kuf_all^T ) instead of S batched trsm/gemm2 pairs, and the
// (M x M) factorisation work is done ONCE (not S times: runtime_variable.py:96-99 broadcast) in float64.
#include "common.h"
#include "internal.h"

namespace {

constexpr double LOG2PI = 1.8378770664093453;

// ------------------------------------------------------------------------------------ small kernels
template <typename TI, typename TO>
__global__ void convert_kernel(int64_t rows, int64_t cols, const TI* __restrict__ src, int64_t lds_, TO* __restrict__ dst, int64_t ldd) {
    const int64_t n = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols, c = i % cols;
        dst[r * ldd + c] = (TO)src[r * lds_ + c];
    }
}
// float64 -> float32 copy of a contiguous array AND the bit pattern of max |dst| (out: cleared by the caller; non-negative floats order like
// unsigned integers) in one launch -- the M x M operands of the split products went through a convert and a max|x| launch on the chain's critical path
__global__ __launch_bounds__(256) void convert_max_kernel(int64_t n, const double* __restrict__ src, float* __restrict__ dst, unsigned* __restrict__ out) {
    __shared__ unsigned wm[4];
    unsigned m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = (float)src[i];
        dst[i] = v;
        const unsigned b = __builtin_bit_cast(unsigned, v) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = wm[w] > m ? wm[w] : m;
        atomicMax(out, m);
    }
}
// dst[c][r] = src[r][c]
template <typename TI, typename TO>
__global__ void transpose_convert_kernel(int64_t rows, int64_t cols, const TI* __restrict__ src, int64_t lds_, TO* __restrict__ dst, int64_t ldd) {
    const int64_t n = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols, c = i % cols;
        dst[c * ldd + r] = (TO)src[r * lds_ + c];
    }
}
// dst = a*x + b*y (elementwise, contiguous)
template <typename T>
__global__ void axpby_kernel(int64_t n, T a, const T* __restrict__ x, T b, const T* __restrict__ y, T* __restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = a * x[i] + (y ? b * y[i] : (T)0);
}
// the gradient outputs of the SVGP training call's tail in ONE launch: dst_k (+)= (T)(src_k + src2_k), k < cnt  (six dependent 5-us launches
// at the end of the caller's stream otherwise)
struct FinishArgs { const double* src[6]; const double* src2[6]; void* dst[6]; int64_t n[6]; int acc[6]; int cnt; };
template <typename T>
__global__ void svgp_finish_kernel(FinishArgs a) {
    const int k = blockIdx.y;
    if (k >= a.cnt) return;
    T* __restrict__ d = (T*)a.dst[k];
    const double* __restrict__ s1 = a.src[k];
    const double* __restrict__ s2 = a.src2[k];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n[k]; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = s1[i] + (s2 ? s2[i] : 0.0);
        d[i] = (a.acc[k] ? d[i] : (T)0) + (T)v;
    }
}
// dst(TO) (+)= a * (TO)src(TI)
template <typename TI, typename TO>
__global__ void add_convert_kernel(int64_t n, TO a, const TI* __restrict__ src, TO* __restrict__ dst, int accumulate) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = (accumulate ? dst[i] : (TO)0) + a * (TO)src[i];
}
template <typename T>
__global__ void diag_embed_kernel(int64_t n, const T* __restrict__ d, T* __restrict__ A) {   // A = diag(d)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * n; i += (int64_t)gridDim.x * blockDim.x)
        A[i] = (i / n == i % n) ? d[i / n] : (T)0;
}
template <typename TI, typename TO>
__global__ void diag_extract_kernel(int64_t n, const TI* __restrict__ A, int64_t lda, TO* __restrict__ d) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = (TO)A[i * lda + i];
}
// out (+)= scale * sum_i x[i]*y[i]
template <typename T>
__global__ __launch_bounds__(256) void dot_kernel(int64_t n, const T* __restrict__ x, const T* __restrict__ y, double scale, double* __restrict__ out) {
    __shared__ double red[16];
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += (double)x[i] * (double)y[i];
    s = block_sum<double>(s, red);
    if (threadIdx.x == 0) atomic_add(out, s * scale);
}
// out += sum_ij A[i][j] * B[j][i]   (n x n, float64; tr(A B))
__global__ __launch_bounds__(256) void dot_t_kernel(int64_t n, const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ out) {
    __shared__ double red[16];
    double s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * n; i += (int64_t)gridDim.x * blockDim.x) s += A[i] * B[(i % n) * n + i / n];
    s = block_sum<double>(s, red);
    if (threadIdx.x == 0) atomic_add(out, s);
}
// copy lower triangle to upper (tiled transpose through LDS)
template <typename T>
__global__ __launch_bounds__(256) void symmetrize_kernel(T* __restrict__ A, int64_t n, int64_t lda, int64_t sA) {
    __shared__ T tile[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;   // tile (by, bx) of the LOWER part, bx <= by
    if (bx > by) return;
    T* a = A + (int64_t)blockIdx.z * sA;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = (int64_t)by * 32 + r, col = (int64_t)bx * 32 + tx;
        tile[r][tx] = (row < n && col < n) ? a[row * lda + col] : (T)0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = (int64_t)bx * 32 + r, col = (int64_t)by * 32 + tx;   // transposed position
        if (row < n && col < n && col > row) a[row * lda + col] = tile[tx][r];
    }
}
// The same with a rank-P term folded in (r06, exact GP):  A <- sym(lower(A)) + c v v^T,  v (n x P) -- the reverse mode's 1/2 alpha alpha^T
// without a pass of its own over the n x n matrix
template <typename T>
__global__ __launch_bounds__(256) void symmetrize_rankp_kernel(T* __restrict__ A, int64_t n, int64_t lda, const T* __restrict__ v, int P, T c, int mirror = 1) {
    __shared__ T tile[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;
    if (bx > by) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = (int64_t)by * 32 + r, col = (int64_t)bx * 32 + tx;
        T x = 0;
        if (row < n && col < n && col <= row) {
            T d = 0;
            for (int p = 0; p < P; ++p) d = fma(v[row * P + p], v[col * P + p], d);
            x = fma(c, d, A[row * lda + col]);
            A[row * lda + col] = x;
        }
        tile[r][tx] = x;
    }
    if (!mirror) return;         // (block-uniform: the reverse pass reads the lower triangle only)
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t row = (int64_t)bx * 32 + r, col = (int64_t)by * 32 + tx;
        if (row < n && col < n && col > row) A[row * lda + col] = tile[tx][r];
    }
}
// Skinny products with the lower-triangular L^-1 (r06, exact GP; P <= 8 right-hand sides): the general small-product kernel took 0.20 / 0.18 ms
// for these two at n = 8192 -- they read n^2 / 2 doubles, 0.07 ms at the rate a streaming read reaches.
//   trmv_lower_kernel:    y = A x      one wave per row, the lanes along it
//   trmv_lower_t_kernel:  y += A^T x   one thread per column over a chunk of 128 rows, chunks summed with atomics (y zeroed by the caller)
template <typename T>
__global__ __launch_bounds__(256) void trmv_lower_kernel(int64_t n, int P, const T* __restrict__ A, int64_t lda, const T* __restrict__ x, int64_t ldx, T* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    T acc[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) acc[p] = 0;
    const T* a = A + r * lda;
#pragma unroll 4
    for (int64_t c = lane; c <= r; c += 64) {
        const T v = a[c];
#pragma unroll
        for (int p = 0; p < 8; ++p) if (p < P) acc[p] = fma(v, x[c * ldx + p], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        if (p < P) { const T t = wave_sum(acc[p]); if (lane == 0) y[r * P + p] = t; }
    }
}
// y = A x for a full (n x n) matrix, one wave per row (r06: w = Ki mu of the SVGP chain -- the small-product kernel with its split-K pre-scale took 0.2 ms
// of the few-sample step's critical path for an 8 MB read)
template <typename T>
__global__ __launch_bounds__(256) void gemv_rows_kernel(int64_t n, int P, const T* __restrict__ A, int64_t lda, const T* __restrict__ x, int64_t ldx, T* __restrict__ y,
                                                        T c = 0, const T* __restrict__ z = nullptr /* y = A x + c z */) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    T acc[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) acc[p] = 0;
    const T* a = A + r * lda;
#pragma unroll 4
    for (int64_t c = lane; c < n; c += 64) {
        const T v = a[c];
#pragma unroll
        for (int p = 0; p < 8; ++p) if (p < P) acc[p] = fma(v, x[c * ldx + p], acc[p]);
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        if (p < P) { const T t = wave_sum(acc[p]); if (lane == 0) y[r * P + p] = z ? t + c * z[r * P + p] : t; }
    }
}
// y (n x P) = A (n x K, row-major, long rows) x (K x P): one workgroup per row (r06: R = Kuf Eb of the generic path, 512 x 131 072 -- the general product took
// 0.18 ms for a 268 MB read); float64 accumulation of the workgroup's partial sums
template <typename T>
__global__ __launch_bounds__(256) void rowdot_kernel(int64_t K, int P, const T* __restrict__ A, int64_t lda, const T* __restrict__ x, T* __restrict__ y) {
    __shared__ double red[16];
    const T* a = A + (int64_t)blockIdx.x * lda;
    T acc[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) acc[p] = 0;
#pragma unroll 4
    for (int64_t c = threadIdx.x; c < K; c += 256) {
        const T v = a[c];
#pragma unroll
        for (int p = 0; p < 8; ++p) if (p < P) acc[p] = fma(v, x[c * P + p], acc[p]);
    }
    for (int p = 0; p < P; ++p) {
        const double t = block_sum<double>((double)acc[p], red);
        if (threadIdx.x == 0) y[(int64_t)blockIdx.x * P + p] = (T)t;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void trmv_lower_t_kernel(int64_t n, int P, const T* __restrict__ A, int64_t lda, const T* __restrict__ x, T* __restrict__ y) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x, r0 = (int64_t)blockIdx.y * 128;
    const int64_t r1 = r0 + 128 < n ? r0 + 128 : n;
    if (r1 <= (int64_t)blockIdx.x * 256) return;                 // the chunk lies above the diagonal
    __shared__ T xs[128 * 8];
    for (int e = threadIdx.x; e < (int)(r1 - r0) * P; e += 256) xs[e] = x[r0 * P + e];
    __syncthreads();
    if (c >= n) return;
    T acc[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) acc[p] = 0;
    const int64_t rs = c > r0 ? c : r0;
#pragma unroll 4
    for (int64_t r = rs; r < r1; ++r) {
        const T v = A[r * lda + c];
#pragma unroll
        for (int p = 0; p < 8; ++p) if (p < P) acc[p] = fma(v, xs[(r - r0) * P + p], acc[p]);
    }
    if (rs < r1) {
#pragma unroll
        for (int p = 0; p < 8; ++p) if (p < P) atomic_add(y + c * P + p, acc[p]);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void sumsq_kernel(int64_t n, const T* __restrict__ x, int64_t sx, double* __restrict__ out) {
    __shared__ double red[16];
    const T* p = x + (int64_t)blockIdx.x * sx;
    double s = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)p[i] * (double)p[i];
    s = block_sum<double>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}
template <typename T>
__global__ __launch_bounds__(256) void trace_kernel(int64_t n, const T* __restrict__ A, int64_t lda, int64_t sA, T* __restrict__ out) {
    __shared__ double red[16];
    const T* a = A + (int64_t)blockIdx.x * sA;
    double s = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)a[i * lda + i];
    s = block_sum<double>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (T)s;
}
template <typename T>
__global__ void gp_finalize_kernel(int S, int64_t N, int P, const T* __restrict__ sld, const double* __restrict__ ss, T* __restrict__ logL) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) logL[s] = (T)(-(double)P * (double)sld[s] - 0.5 * (ss[s] + (double)N * P * LOG2PI));
}
// Y (S|1,n) -> dst (S,n), optionally negated
template <typename T>
__global__ void bcast_copy_kernel(int S, int64_t n, const T* __restrict__ src, int64_t ssrc, T* __restrict__ dst, T scale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)S * n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = scale * src[(i / n) * ssrc + (i % n)];
}

// dot_kernel ends with ONE atomic per workgroup on one word: 4096 of them serialise to ~0.16 ms (seen on the critical chain in front of the T
// product, r03 timeline); 64 workgroups with a grid-stride loop take ~5 us
inline unsigned dotgrid(int64_t n) { int64_t b = (n + 255) / 256; if (b < 1) b = 1; if (b > 64) b = 64; return (unsigned)b; }
inline unsigned gridn(int64_t n) { int64_t b = (n + 255) / 256; if (b < 1) b = 1; if (b > 4096) b = 4096; return (unsigned)b; }

// A composite's scratch layout is ONE list of take() calls (`layout`), run once to count the bytes and once to carve them, so the two
// cannot disagree.  false (need = the bytes asked for) when the scratch cannot be allocated.
template <typename F>
bool carve_scratch(mxf_ctx* h, F&& layout, size_t& need) {
    Carver count(nullptr);
    layout(count);
    need = count.off;
    void* ws = mxf_ws(h, need);
    if (!ws) return false;
    Carver cv(ws);
    layout(cv);
    return true;
}
// dst = (TO)src, n contiguous elements
template <typename TI, typename TO>
void copy_convert(int64_t n, const TI* src, TO* dst, hipStream_t s) {
    hipLaunchKernelGGL((convert_kernel<TI, TO>), dim3(gridn(n)), dim3(256), 0, s, (int64_t)1, n, src, n, dst, n);
}
// f(float) or f(double) for a float32 / float64 call: the typed body behind each C entry point
template <typename F>
int by_dtype(mxf_ctx* h, const char* fn, int dtype, F&& f) {
    if (dtype == MXF_F32) return f(0.f);
    if (dtype == MXF_F64) return f(0.0);
    MXF_FAIL(h, -2, "%s: bad dtype %d", fn, dtype);
}
// The sparse models' two Grams, hyper-parameters shared by the samples.  Kuu = k(Z, Z) + jitter I (M x M) in float64:
inline int kuu_f64(mxf_ctx* h, hipStream_t st, int kind, int64_t M, int Q, const double* Zd, const double* lsd, int ard, const double* vard, double jitter,
                   double* Kuu) {
    return mxf_gram_internal(h, st, {.kind = kind, .dtype = MXF_F64, .N = M, .Q = Q, .X = Zd, .ls = lsd, .ard = ard, .var = vard, .jitter = jitter,
                                     .K = {Kuu, M, M * M}});
}
// ... and K = k(A, B) (n x n2, dense rows)
inline int cross_gram(mxf_ctx* h, hipStream_t st, int kind, int dtype, int Q, int64_t n, const void* A, int64_t n2, const void* B, const void* ls, int ard,
                      const void* var, void* K) {
    return mxf_gram_internal(h, st, {.kind = kind, .dtype = dtype, .N = n, .N2 = n2, .Q = Q, .X = A, .X2 = B, .ls = ls, .ard = ard, .var = var, .K = {K, n2}});
}
// The sparse models' float64 M x M factorisations, one dense matrix each: L = chol(A) in place; L^-1; sum_i log L[i][i].
// bare (the SVGP core): the strict upper triangle stays as it was (trtri / sumlogdiag read the lower one only) and the caller has zeroed info
inline int potrf_f64(mxf_ctx* h, hipStream_t st, int64_t M, double* A, int* info, bool bare = false) {
    return mxf_potrf_internal(h, st, {.dtype = MXF_F64, .n = M, .A = {A, M, M * M}, .info = info, .zero_upper = !bare, .zero_info = !bare});
}
inline int trtri_f64(mxf_ctx* h, hipStream_t st, int64_t M, const double* L, double* Linv) {
    return mxf_trtri_internal(h, st, {.dtype = MXF_F64, .n = M, .L = {L, M, M * M}, .Linv = {Linv, M, M * M}});
}
inline int sumlogdiag_f64(mxf_ctx* h, hipStream_t st, int64_t M, const double* L, double* out) {
    return mxf_sumlogdiag_internal(h, st, {.dtype = MXF_F64, .n = M, .L = {L, M, M * M}, .out = out});
}

// ================================================================================================ exact GP
template <typename T>
int gp_logpdf_typed(mxf_ctx* h, int kind, int dtype, int S, int64_t N, int Q, int P, const T* X, int64_t sX, const T* Y, int64_t sY,
                    const T* noise, int64_t snoise, const T* ls, int ard, int64_t sls, const T* var, int64_t svar, double jitter,
                    T* logL, T* L, T* LinvY, int* info, int want_grad, T* dX, T* dY, T* dnoise, T* dls, T* dvar, hipStream_t st) {
    const int64_t NN = N * N, NP = N * P;
    T* sld; double* ss; T* Linv = nullptr; T* dK = nullptr; T* alpha = nullptr;
    size_t need;
    const bool ok = carve_scratch(h, [&](Carver& cv) {
        sld = cv.take<T>(S); ss = cv.take<double>(S);
        if (want_grad) { Linv = cv.take<T>((size_t)S * NN); dK = cv.take<T>((size_t)S * NN); alpha = cv.take<T>((size_t)S * NP); }
    }, need);
    if (!ok) MXF_FAIL(h, -4, "mxf_gp_logpdf: cannot allocate %zu bytes of scratch", need);
    int rc;
    // K = k(X,X) + (noise + jitter) I   (gp_regression.py:55-60), built straight into the L buffer
    rc = mxf_gram_internal(h, st, {.kind = kind, .dtype = dtype, .S = S, .N = N, .Q = Q, .X = X, .sX = sX, .ls = ls, .ard = ard, .sls = sls, .var = var,
                                   .svar = svar, .diag_add = noise, .sdiag = snoise, .jitter = jitter, .K = {L, N, NN}});
    if (rc) return rc;
    // L^-1 Y (:66).  Large N with gradients: the reverse mode needs L^-1 anyway, and L^-1 Y as ONE product replaces N / 64 dependent
    // block steps (6.9 ms at N = 8192); small N keeps the reference's trsm.
    const bool via_inverse = want_grad && N >= 2048;
    // (r06) one matrix, few right-hand sides: the two skinny products with L^-1 as triangular streaming reads, 1/2 alpha alpha^T folded into
    // the symmetrisation of dK
    const bool tri_skinny = via_inverse && S == 1 && P <= 8;
    // (r05) float64, one matrix: the factorisation forms L^-1 itself, row block by row block on a third stream next to its serial chain
    bool inv_done = false;
    rc = mxf_potrf_internal(h, st, {.dtype = dtype, .S = S, .n = N, .A = {L, N, NN}, .info = info,
                                    .Linv = {(via_inverse && S == 1 && sizeof(T) == 8) ? Linv : nullptr, N}, .inv_done = &inv_done});   // :61
    if (rc) return rc;
    auto trtri = [&] { return mxf_trtri_internal(h, st, {.dtype = dtype, .S = S, .n = N, .L = {L, N, NN}, .Linv = {Linv, N, NN}}); };
    if (via_inverse) {
        if (!inv_done) rc = trtri();
        if (rc) return rc;
        if (tri_skinny) hipLaunchKernelGGL((trmv_lower_kernel<T>), dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, N, P, (const T*)Linv, N, Y, (int64_t)P, LinvY);
        else {
        rc = mxf_gemm_internal(h, st, {.dtype = dtype, .M = N, .N = P, .K = N, .A = {Linv, N, NN}, .B = {Y, P, sY}, .C = {LinvY, P, NP}, .batch = S});
        if (rc) return rc;
        }
    } else {
        hipLaunchKernelGGL((bcast_copy_kernel<T>), dim3(gridn(S * NP)), dim3(256), 0, st, S, NP, Y, sY, LinvY, (T)1);
        rc = mxf_trsm_internal(h, st, {.dtype = dtype, .S = S, .n = N, .nrhs = P, .L = {L, N, NN}, .B = {LinvY, P, NP}});
        if (rc) return rc;
    }
    rc = mxf_sumlogdiag_internal(h, st, {.dtype = dtype, .S = S, .n = N, .L = {L, N, NN}, .out = sld});                    // :67
    if (rc) return rc;
    hipLaunchKernelGGL((sumsq_kernel<T>), dim3(S), dim3(256), 0, st, NP, LinvY, NP, ss);
    hipLaunchKernelGGL((gp_finalize_kernel<T>), dim3((S + 63) / 64), dim3(64), 0, st, S, N, P, sld, ss, logL);   // :68-70
    MXF_LAUNCH_CHECK(h);
    if (!want_grad) return 0;

    // reverse mode: dlogL/dK = 1/2 (alpha alpha^T - P K^-1), alpha = K^-1 Y; dlogL/dY = -alpha
    if (!via_inverse) {
        rc = trtri();
        if (rc) return rc;
    }
    // per sample, lower triangle: dK = -P/2 Linv^T Linv + beta dK (L^-1 lower triangular: tile (i, j <= i) needs k >= i only)
    auto kinv_term = [&](double beta) {
        return mxf_gemm_internal(h, st, {.dtype = dtype, .ta = 1, .M = N, .N = N, .K = N, .alpha = -0.5 * P, .A = {Linv, N, NN}, .B = {Linv, N, NN},
                                         .beta = beta, .C = {dK, N, NN}, .batch = S, .lower_only = 1, .tri = MXF_TRI_UPPER});
    };
    if (tri_skinny) {
        MXF_HIP(h, hipMemsetAsync(alpha, 0, sizeof(T) * NP, st));
        hipLaunchKernelGGL((trmv_lower_t_kernel<T>), dim3((unsigned)((N + 255) / 256), (unsigned)((N + 127) / 128)), dim3(256), 0, st, N, P, (const T*)Linv, N,
                           (const T*)LinvY, alpha);                                                                 // alpha = Linv^T LinvY
        rc = kinv_term(0.0);
        if (rc) return rc;
        hipLaunchKernelGGL((symmetrize_rankp_kernel<T>), dim3((unsigned)((N + 31) / 32), (unsigned)((N + 31) / 32)), dim3(256), 0, st, dK, N, N, (const T*)alpha, P, (T)0.5);
    } else {
    rc = mxf_gemm_internal(h, st, {.dtype = dtype, .ta = 1, .M = N, .N = P, .K = N, .A = {Linv, N, NN}, .B = {LinvY, P, NP}, .C = {alpha, P, NP}, .batch = S});   // alpha = Linv^T LinvY
    if (rc) return rc;
    rc = mxf_gemm_internal(h, st, {.dtype = dtype, .tb = 1, .M = N, .N = N, .K = P, .alpha = 0.5, .A = {alpha, P, NP}, .B = {alpha, P, NP}, .C = {dK, N, NN},
                                   .batch = S, .lower_only = 1});                                                  // 1/2 alpha alpha^T (lower)
    if (rc) return rc;
    rc = kinv_term(1.0);                                                                                            // - P/2 Linv^T Linv (lower)
    if (rc) return rc;
    hipLaunchKernelGGL((symmetrize_kernel<T>), dim3((unsigned)((N + 31) / 32), (unsigned)((N + 31) / 32), S), dim3(256), 0, st, dK, N, N, NN);
    }
    if (dY) hipLaunchKernelGGL((bcast_copy_kernel<T>), dim3(gridn(S * NP)), dim3(256), 0, st, S, NP, (const T*)alpha, NP, dY, (T)-1);
    if (dnoise) hipLaunchKernelGGL((trace_kernel<T>), dim3(S), dim3(256), 0, st, N, (const T*)dK, N, NN, dnoise);
    const int lsn = ard ? Q : 1;
    if (dX) MXF_HIP(h, hipMemsetAsync(dX, 0, sizeof(T) * S * N * Q, st));
    if (dls) MXF_HIP(h, hipMemsetAsync(dls, 0, sizeof(T) * S * lsn, st));
    if (dvar) MXF_HIP(h, hipMemsetAsync(dvar, 0, sizeof(T) * S, st));
    // outputs are per sample (S, ...) even when the primal is broadcast: use per-sample strides for the outputs
    // by running one sample at a time when the primal stride is 0
    for (int s = 0; s < S; ++s) {
        rc = mxf_gram_bwd_internal(h, st, {.kind = kind, .dtype = dtype, .N = N, .Q = Q, .X = X + (int64_t)s * sX, .ls = ls + (int64_t)s * sls, .ard = ard,
                                           .var = var + (int64_t)s * svar, .dK = dK + (int64_t)s * NN, .lddk = N, .sdK = NN,
                                           .dX = dX ? dX + (int64_t)s * N * Q : nullptr, .dls = dls ? dls + (int64_t)s * lsn : nullptr,
                                           .dvar = dvar ? dvar + s : nullptr, .dk_symmetric = true /* dK was symmetrised above */});
        if (rc) return rc;
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

// ================================================================================================ SVGP
// per column n (of all S*B columns): e = y - u, q = k^T (H0 k); T <- a1*beta*(P*T + w e); partial sums per sample
template <typename T>
__global__ __launch_bounds__(256) void svgp_mid_kernel(int64_t SB, int64_t B, int64_t M, int P, const T* __restrict__ Kuf,
                                                       T* __restrict__ Text, const T* __restrict__ Y, int64_t sY,
                                                       const T* __restrict__ w /* M x P */, const T* __restrict__ noise, double a1,
                                                       int want_grad, T* __restrict__ E /* SB x P */, T* __restrict__ dY, int dY_shared,
                                                       double* __restrict__ scal /* [S][2] : sum q, sum e^2 */) {
    __shared__ double red[16];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < SB;
    const int64_t s = valid ? n / B : 0, nb = valid ? n % B : 0;
    const T beta = (T)1 / noise[0];
    constexpr int PMAX = 8;
    T e[PMAX];
    double e2 = 0;
#pragma unroll
    for (int p = 0; p < PMAX; ++p) {
        e[p] = 0;
        if (p < P && valid) {
            e[p] = Y[s * sY + nb * P + p] - Text[(M + p) * SB + n];
            e2 += (double)e[p] * (double)e[p];
            if (E) E[n * P + p] = e[p];
            if (want_grad && dY) {
                const T g = (T)(-a1) * beta * e[p];
                if (dY_shared) atomic_add(dY + nb * P + p, g); else dY[n * P + p] = g;
            }
        }
    }
    T q = 0;
    const T c1 = (T)a1 * beta, cP = (T)P;
    if (valid) {
        for (int64_t m = 0; m < M; ++m) {
            const T k = Kuf[m * SB + n], t = Text[m * SB + n];
            q = fma(k, t, q);
            if (want_grad) {
                T we = 0;
#pragma unroll
                for (int p = 0; p < PMAX; ++p) if (p < P) we = fma(w[m * P + p], e[p], we);
                Text[m * SB + n] = c1 * (cP * t + we);
            }
        }
    }
    // blocks never straddle... they may: reduce per sample with a segmented approach (block spans <= 2 samples when B>=256;
    // general case: per-thread atomics when the block straddles)
    const int64_t n0 = (int64_t)blockIdx.x * 256, n1 = (n0 + 255 < SB - 1) ? n0 + 255 : SB - 1;
    if (n0 / B == n1 / B) {
        double qs = block_sum<double>((double)q, red);
        double es = block_sum<double>(e2, red);
        if (threadIdx.x == 0) { atomic_add(scal + 2 * (n0 / B), qs); atomic_add(scal + 2 * (n0 / B) + 1, es); }
    } else if (valid) {
        atomic_add(scal + 2 * s, (double)q);
        atomic_add(scal + 2 * s + 1, e2);
    }
}

// U[p][n] = sum_m w[m][p] * Kuf[m][n]  (the w^T row block of [H0; w^T] Kuf, kept out of the MFMA GEMM: a 1-row tile would waste
// a whole 128-row tile).  HBM-read bound (M*SB*e bytes), 16-byte loads, lanes <-> columns.
// gridDim.y > 1 (few columns: r05): the M rows are dealt to gridDim.y workgroups per column block, which ADD into U (zeroed by the caller) --
// with 1 024 columns the one-workgroup-per-512-columns form is two workgroups walking 1 024 dependent rows each: 0.37 ms of a 2 ms step
template <typename T, int PT>
__global__ __launch_bounds__(256) void wt_kuf_kernel(int64_t M, int64_t SB, int P, const T* __restrict__ Kuf, const T* __restrict__ w,
                                                     T* __restrict__ U) {
    constexpr int VEC = Vec16<T>::n;
    typedef typename Vec16<T>::type V;
    const int64_t n0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (n0 >= SB) return;
    if (gridDim.y > 1) {
        const int64_t mc = (M + gridDim.y - 1) / gridDim.y, mb = (int64_t)blockIdx.y * mc, me = mb + mc < M ? mb + mc : M;
        T a2[PT][VEC];
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int v = 0; v < VEC; ++v) a2[p][v] = 0;
        for (int64_t m = mb; m < me; ++m)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const T k = (n0 + v < SB) ? Kuf[m * SB + n0 + v] : (T)0;
#pragma unroll
                for (int p = 0; p < PT; ++p) a2[p][v] = fma((p < P) ? w[m * P + p] : (T)0, k, a2[p][v]);
            }
#pragma unroll
        for (int p = 0; p < PT; ++p)
            if (p < P)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (n0 + v < SB) atomic_add(U + (int64_t)p * SB + n0 + v, a2[p][v]);
        return;
    }
    T acc[PT][VEC];
#pragma unroll
    for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[p][v] = 0;
    if (n0 + VEC <= SB && (SB % VEC) == 0) {
        for (int64_t m = 0; m < M; ++m) {
            const V kv = *reinterpret_cast<const V*>(Kuf + m * SB + n0);
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                const T wp = (p < P) ? w[m * P + p] : (T)0;
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[p][v] = fma(wp, kv[v], acc[p][v]);
            }
        }
    } else {
        for (int64_t m = 0; m < M; ++m)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const T k = (n0 + v < SB) ? Kuf[m * SB + n0 + v] : (T)0;
#pragma unroll
                for (int p = 0; p < PT; ++p) acc[p][v] = fma((p < P) ? w[m * P + p] : (T)0, k, acc[p][v]);
            }
    }
#pragma unroll
    for (int p = 0; p < PT; ++p)
        if (p < P)
#pragma unroll
            for (int v = 0; v < VEC; ++v) if (n0 + v < SB) U[(int64_t)p * SB + n0 + v] = acc[p][v];
}

// The same row block from the split planes of Kfu (operand (n, k = m), gemm_split.hip layout): U[p][n] = sum_m w[m][p] Kfu[n][m].
// lane <-> column n (32 contiguous bytes per lane and plane per k block); HBM-read bound (4 bytes per element in the f16x2 format, 6 in bf16x3).
// NP = 2: f16x2 planes holding k / variance * 2^14 (result scaled by variance * 2^-14).
template <int PT, int NP>
__global__ __launch_bounds__(256) void wt_planes_kernel(int64_t M, int64_t SB, int P, const unsigned short* __restrict__ pl, int64_t pstride,
                                                        const float* __restrict__ w, float* __restrict__ U, const float* __restrict__ var) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= SB) return;
    float acc[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) acc[p] = 0.f;
    const int64_t K16 = (M + 15) / 16;
    for (int64_t kb = 0; kb < K16; ++kb) {
        const unsigned short* base = pl + (kb * SB + n) * 16;
        u4 v[NP][2];
#pragma unroll
        for (int q = 0; q < NP; ++q) { v[q][0] = *reinterpret_cast<const u4*>(base + q * pstride); v[q][1] = *reinterpret_cast<const u4*>(base + q * pstride + 8); }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float x = 0.f;
#pragma unroll
            for (int q = NP - 1; q >= 0; --q) {
                const unsigned word = v[q][j >> 3][(j & 7) >> 1];
                if (NP == 2) {
                    x += (float)__builtin_bit_cast(_Float16, (unsigned short)((j & 1) ? (word >> 16) : (word & 0xffffu)));
                } else {
                    const unsigned bits = (j & 1) ? (word & 0xffff0000u) : (word << 16);
                    x += __builtin_bit_cast(float, bits);
                }
            }
            const int64_t m = kb * 16 + j;
            if (m < M) {
#pragma unroll
                for (int p = 0; p < PT; ++p) acc[p] = fma((p < P) ? w[m * P + p] : 0.f, x, acc[p]);
            }
        }
    }
    const float sc = NP == 2 ? var[0] * (1.f / 16384.f) : 1.f;
#pragma unroll
    for (int p = 0; p < PT; ++p) if (p < P) U[(int64_t)p * SB + n] = acc[p] * sc;
}

// A_Ki = (G - T1 - T1^T) + 1/2 (Gw mu^T + mu Gw^T) - b (P/2 Su + 1/2 mu mu^T)
__global__ void aki_kernel(int64_t M, int P, const double* __restrict__ G, const double* __restrict__ T1, const double* __restrict__ Gw,
                           const double* __restrict__ mu, const double* __restrict__ Su, double b, double* __restrict__ A) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < M * M; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx / M, j = idx % M;
        double v = G[idx] - T1[idx] - T1[j * M + i];
        double r1 = 0, mm = 0;
        for (int p = 0; p < P; ++p) { if (Gw) r1 += Gw[i * P + p] * mu[j * P + p] + mu[i * P + p] * Gw[j * P + p]; mm += mu[i * P + p] * mu[j * P + p]; }
        A[idx] = v + 0.5 * r1 - b * (0.5 * P * Su[idx] + 0.5 * mm);
    }
}
// (r06) dSu = -X + c (Su^-1 - Ki)
__global__ void dsu_kernel(int64_t n, const double* __restrict__ X, const double* __restrict__ Sui, const double* __restrict__ Ki, double c, double* __restrict__ dSu) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dSu[i] = c * (Sui[i] - Ki[i]) - X[i];
}
// (r06) dKuu0 = -X + Y + Y^T + b (P/2 KSK + 1/2 w w^T) - bP/2 Ki,  KSK = Ki Su Ki given or = Ki - H0
__global__ void dkuu0_kernel(int64_t M, int P, const double* __restrict__ X, const double* __restrict__ Y, const double* __restrict__ Ki, const double* __restrict__ KSK,
                             const double* __restrict__ H0, const double* __restrict__ w, double b, double* __restrict__ dKuu) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < M * M; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx / M, j = idx % M;
        double ww = 0;
        for (int p = 0; p < P; ++p) ww += w[i * P + p] * w[j * P + p];
        const double ksk = KSK ? KSK[idx] : Ki[idx] - H0[idx];
        dKuu[idx] = -X[idx] + Y[idx] + Y[j * M + i] + b * (0.5 * P * ksk + 0.5 * ww) - 0.5 * b * P * Ki[idx];
    }
}
// (r06) Gw == nullptr above: the part A0 of A_Ki that does not depend on the reverse pass's R.  -Ki A_Ki Ki is linear in A_Ki and
// Ki (Gw mu^T) Ki = (Ki Gw)(Ki mu)^T = v w^T, so the two M^3 products run on A0 under the T product / the reverse pass and what is left for the
// step's tail is the rank-2P term:  dKuu -= 1/2 (v w^T + w v^T),  v = Ki Gw = dmu + b w  (dmu = Ki Gw - b w is formed anyway)
__global__ void dkuu_rank_kernel(int64_t M, int P, const double* __restrict__ dmu, const double* __restrict__ w, double b, double* __restrict__ dKuu) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < M * M; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx / M, j = idx % M;
        double r = 0;
        for (int p = 0; p < P; ++p) {
            const double vi = dmu[i * P + p] + b * w[i * P + p], vj = dmu[j * P + p] + b * w[j * P + p];
            r += vi * w[j * P + p] + w[i * P + p] * vj;
        }
        dKuu[idx] -= 0.5 * r;
    }
}
// G' = (P/2 * a1 * beta) * Psi2 ; Gw = a1*beta*R   (beta on device)
template <typename T>
__global__ void scale_beta_kernel(int64_t n, const T* __restrict__ src, const double* __restrict__ noise, double c, double* __restrict__ dst) {
    const double beta = 1.0 / noise[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = c * beta * (double)src[i];
}
// logL[s], and the direct (non-Gram) gradient terms w.r.t. noise and kernel variance
template <typename T>
__global__ void svgp_finalize_kernel(int S, int64_t B, int64_t M, int P, const double* __restrict__ scal, const double* __restrict__ noise,
                                     const double* __restrict__ var, const double* __restrict__ sldL, const double* __restrict__ sldLs,
                                     const double* __restrict__ trKiSu, const double* __restrict__ muw, double scaling, double a1,
                                     T* __restrict__ logL, double* __restrict__ dnoise, double* __restrict__ dvar_direct,
                                     const double* __restrict__ qfix = nullptr) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double s2 = noise[0], beta = 1.0 / s2, vk = var[0];
    const double negKL = 0.5 * P * ((double)M + 2.0 * sldLs[0] - 2.0 * sldL[0] - trKiSu[0]) - 0.5 * muw[0];
    // whitened tier: sum_n q_n over ALL samples = tr((I - A_s A_s^T) Phi), formed in float64 from Phi = V V^T (qfix = [c tr Phi, c tr(Su L^-T Phi L^-1)],
    // c = P a1 beta / 2).  The reverse pass's own per-sample sums q_n = k_n . T_n multiply a recomputed float32 k_n by |T| ~ sqrt(cond): they
    // keep the split between the samples, their total is replaced (the mean over samples -- the only reduction the reference applies,
    // factor_graph.py:233 -- then carries the accurate total).
    double qshift = 0;
    if (qfix) {
        double qs = 0;
        for (int s = 0; s < S; ++s) qs += scal[2 * s];
        qshift = ((qfix[0] - qfix[1]) / (0.5 * P * a1 * beta) - qs) / (double)S;
    }
    double dn = 0;
    for (int s = 0; s < S; ++s) {
        const double Q0 = scal[2 * s] + qshift, E2 = scal[2 * s + 1];
        const double l = -0.5 * (double)B * P * (LOG2PI + log(s2)) - 0.5 * P * beta * (double)B * vk - 0.5 * beta * E2 + 0.5 * P * beta * Q0;
        logL[s] = (T)(scaling * l + negKL);
        dn += 0.5 * (double)B * P / beta - 0.5 * P * (double)B * vk - 0.5 * E2 + 0.5 * P * Q0;
    }
    if (dnoise) dnoise[0] = a1 * (-beta * beta) * dn;
    // (whitened tier: the reverse pass's kernel-variance gradient contains P beta sum_n q_n / variance through Kuf -- the same total, corrected the same way)
    if (dvar_direct) dvar_direct[0] = a1 * (double)S * (-0.5 * P * beta * (double)B) + a1 * P * beta * qshift * (double)S / vk;
}

// materialised-Gram mode (any kernel with an autograd-capable K on the host: Add / Multiply / Linear ... ): the caller passes
// Kuu (M x M, without jitter), Kuf (M x B), Kdiag (B) and receives d/dKuu, d/dKuf, d/dKdiag instead of kernel-parameter gradients
template <typename T>
struct SvgpMat { const T* Kuu = nullptr; const T* Kuf = nullptr; const T* Kdiag = nullptr; T* dKuu = nullptr; T* dKuf = nullptr; T* dKdiag = nullptr; };
__global__ void add_diag_kernel(int64_t n, double* __restrict__ A, double v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) A[i * n + i] += v;
}
// ---- heteroscedastic / per-output noise (svgp_regression.py:61-67): noise is (nrows, ncols), nrows in {1,B}, ncols in {1,P} ------
// one thread per column n: beta_d = 1/noise[n|0][d|0], bs = sum_d beta_d, e = y - u, q = k^T H0 k;
//   l_s += -1/2 sum_d (beta_d e_d^2 + log 2pi + log noise_d) - 1/2 bs (var - q)
// reverse: dY = -a1 beta.e ; Eb = a1 beta.e (for Gw = Kuf Eb) ; T[:,n] <- a1 (bs T[:,n] + w (beta.e)) = dKuf ; Ksc = 1/2 a1 bs Kuf[:,n]
// per-column quantities of one Y sample (shared by the two passes below).  ys = index of the Y sample: the column's own sample, or -- when
// X (hence Kuf) is shared and only Y is sampled -- one of the SY samples that share the column
template <typename T>
__device__ __forceinline__ void het_column(int64_t n, int64_t ys, int64_t SB, int64_t B, int64_t M, int P, const T* __restrict__ Text,
                                           const T* __restrict__ Y, int64_t sY, const T* __restrict__ noise, int64_t nrows, int ncols,
                                           double (&be)[8], double (&beta)[8], double& e2b, double& lg, double& bs) {
    const int64_t nb = n % B, nr = (nrows > 1) ? nb : 0;
    e2b = 0; lg = 0; bs = 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        be[p] = 0; beta[p] = 0;
        if (p < P) {
            const double nz = (double)noise[nr * ncols + (ncols > 1 ? p : 0)];
            beta[p] = 1.0 / nz;
            const double e = (double)Y[ys * sY + nb * P + p] - (double)Text[(M + p) * SB + n];
            be[p] = beta[p] * e;
            e2b += be[p] * e; lg += LOG2PI + log(nz); bs += beta[p];
        }
    }
}
// pass 1, grid (column tiles, row chunks of RCH rows): q_n partial sums (atomics into qbuf) and, for the reverse mode, the in-place
// T[:,n] <- a1 (SY bs T[:,n] + w sum_ys(beta.e)) and Ksc = 1/2 a1 SY bs Kuf[:,n].  Rows are split over blockIdx.y so that M x S*B pairs fill
// the chip (one thread per column alone left it latency bound: 4 ms at 512 x 131072).
constexpr int HET_RCH = 32;
template <typename T>
__global__ __launch_bounds__(256) void svgp_het_rows_kernel(int64_t SB, int64_t B, int64_t M, int P, int SY, const T* __restrict__ Kuf,
                                                            T* __restrict__ Text, const T* __restrict__ Y, int64_t sY, const T* __restrict__ w,
                                                            const T* __restrict__ noise, int64_t nrows, int ncols, double a1, int want_grad,
                                                            T* __restrict__ Ksc, T* __restrict__ qbuf) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= SB) return;
    double be[8], beta[8], e2b, lg, bs, besum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int ys = 0; ys < SY; ++ys) {
        het_column<T>(n, SY > 1 ? ys : n / B, SB, B, M, P, Text, Y, sY, noise, nrows, ncols, be, beta, e2b, lg, bs);
#pragma unroll
        for (int p = 0; p < 8; ++p) besum[p] += be[p];
    }
    const double bst = bs * (double)SY;
    const int64_t m0 = (int64_t)blockIdx.y * HET_RCH, m1 = (m0 + HET_RCH < M) ? m0 + HET_RCH : M;
    double q = 0;
    for (int64_t m = m0; m < m1; ++m) {
        const double k = (double)Kuf[m * SB + n], t = (double)Text[m * SB + n];
        q = fma(k, t, q);
        if (want_grad) {
            double we = 0;
#pragma unroll
            for (int p = 0; p < 8; ++p) if (p < P) we = fma((double)w[m * P + p], besum[p], we);
            Text[m * SB + n] = (T)(a1 * (bst * t + we));
            Ksc[m * SB + n] = (T)(0.5 * a1 * bst * k);
        }
    }
    atomic_add(qbuf + n, (T)q);
}
// pass 2, one thread per column: l_s, sum bs, dY, Eb, dnoise, dKdiag.  Sums that land on ONE address (the per-sample scalars; dnoise when the
// noise is shared by all rows) are reduced over the block first -- 131 072 same-address float64 atomics cost 4 ms.
template <typename T>
__global__ __launch_bounds__(256) void svgp_het_cols_kernel(int64_t SB, int64_t B, int64_t M, int P, int SY, const T* __restrict__ Text,
                                                            const T* __restrict__ Y, int64_t sY, const T* __restrict__ noise, int64_t nrows,
                                                            int ncols, const double* __restrict__ var,
                                                            const T* __restrict__ kdiag /* per column, or NULL -> var[0] */, double a1,
                                                            int want_grad, const T* __restrict__ qbuf, T* __restrict__ Eb, T* __restrict__ dY,
                                                            int dY_shared, T* __restrict__ dnoise, T* __restrict__ dkdiag,
                                                            double* __restrict__ scal /* [S][2]: l_s, sum bs */) {
    __shared__ double red[16];
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < SB;
    const int64_t nn = valid ? n : SB - 1;
    const int64_t s = nn / B, nb = nn % B, nr = (nrows > 1) ? nb : 0;
    const double q = (double)qbuf[nn];
    const double vk = kdiag ? (double)kdiag[nn] : var[0];
    const int64_t n0 = (int64_t)blockIdx.x * 256, n1 = (n0 + 255 < SB - 1) ? n0 + 255 : SB - 1;
    const bool one_sample = (n0 / B) == (n1 / B);
    double besum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gn[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bs = 0;
    for (int ys = 0; ys < SY; ++ys) {
        double be[8], beta[8], e2b, lg;
        // NOTE: U (rows M.. of Text) is untouched by pass 1, so e is recomputed from the same values
        const int64_t sidx = SY > 1 ? ys : s;
        het_column<T>(nn, sidx, SB, B, M, P, Text, Y, sY, noise, nrows, ncols, be, beta, e2b, lg, bs);
        const double lval = valid ? -0.5 * (e2b + lg) - 0.5 * bs * (vk - q) : 0.0, bval = valid ? bs : 0.0;
        if (one_sample || SY > 1) {
            const double ls_ = block_sum<double>(lval, red), bb_ = block_sum<double>(bval, red);
            const int64_t sw = SY > 1 ? ys : n0 / B;
            if (threadIdx.x == 0) { atomic_add(scal + 2 * sw, ls_); atomic_add(scal + 2 * sw + 1, bb_); }
        } else if (valid) {
            atomic_add(scal + 2 * s, lval);
            atomic_add(scal + 2 * s + 1, bval);
        }
        if (want_grad) {
#pragma unroll
            for (int p = 0; p < 8; ++p)
                if (p < P) {
                    besum[p] += be[p];
                    gn[p] += a1 * (0.5 * be[p] * be[p] - 0.5 * beta[p] + 0.5 * (vk - q) * beta[p] * beta[p]);
                    if (valid && dY) {
                        const T g = (T)(-a1 * be[p]);
                        if (SY > 1) dY[(ys * B + nb) * P + p] = g;
                        else if (dY_shared) atomic_add(dY + nb * P + p, g);
                        else dY[n * P + p] = g;
                    }
                }
        }
    }
    if (!want_grad) return;
    if (valid && dkdiag) dkdiag[n] = (T)(-0.5 * a1 * bs * (double)SY);
#pragma unroll
    for (int p = 0; p < 8; ++p)
        if (p < P) {
            if (valid) Eb[n * P + p] = (T)(a1 * besum[p]);
            if (dnoise) {
                const double g = valid ? gn[p] : 0.0;
                if (nrows > 1) { if (valid) atomic_add(dnoise + nr * ncols + (ncols > 1 ? p : 0), (T)g); }
                else {
                    const double gs = block_sum<double>(g, red);          // shared noise: one address per output column
                    if (threadIdx.x == 0) atomic_add(dnoise + (ncols > 1 ? p : 0), (T)gs);
                }
            }
        }
}
template <typename T>
__global__ void svgp_het_finalize_kernel(int S, int64_t M, int P, const double* __restrict__ scal, const double* __restrict__ sldL,
                                         const double* __restrict__ sldLs, const double* __restrict__ trKiSu, const double* __restrict__ muw,
                                         double scaling, double a1, T* __restrict__ logL, double* __restrict__ dvar_direct) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double negKL = 0.5 * P * ((double)M + 2.0 * sldLs[0] - 2.0 * sldL[0] - trKiSu[0]) - 0.5 * muw[0];
    double sb = 0;
    for (int s = 0; s < S; ++s) { logL[s] = (T)(scaling * scal[2 * s] + negKL); sb += scal[2 * s + 1]; }
    if (dvar_direct) dvar_direct[0] = -0.5 * a1 * sb;
}

// ---- streaming heteroscedastic bound (r04): per-row noise (B, 1), one output column, float32 split path ------------------------------------
// svgp_regression.py:61-67 with noise (N, 1): beta_n = 1 / noise_n.  With nmin = min_n noise_n and the weights r_n = nmin beta_n <= 1:
//   planes of Kuf diag(sqrt r)  ->  Psi2' = nmin sum_n beta_n k_n k_n^T           (the core's G = P a1 / 2 (1/nmin) Psi2': the homoscedastic code with noise := nmin)
//   planes of diag(r) Kfu (+ U' = r U)  ->  T'' = T diag(r),  y' = r y            (the fused reverse pass with noise := nmin sees e'' = r e and forms exactly
//                                                                                  a1 beta_n (w e_n + P T_n), sum_n beta_n q_n, dY = -a1 beta_n e_n, R = Kuf (beta e))
// What the fused pass cannot deliver -- sum_n beta_n e_n^2 and the per-row noise gradient, which needs q_n per COLUMN -- comes from one
// extra pass over the Kfu planes and T'' (het_stats_kernel).
__global__ __launch_bounds__(256) void het_min_kernel(int64_t B, const float* __restrict__ noise, unsigned* __restrict__ minbits) {
    __shared__ unsigned wm[4];
    unsigned m = 0x7f800000u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B; i += (int64_t)gridDim.x * 256) { const unsigned b = __builtin_bit_cast(unsigned, noise[i]); m = b < m ? b : m; }
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = t < m ? t : m; }
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) { for (int w = 1; w < 4; ++w) m = wm[w] < m ? wm[w] : m; atomicMin(minbits, m); }      // positive floats order as their bits
}
__global__ __launch_bounds__(256) void het_prep_kernel(int64_t B, const float* __restrict__ noise, const unsigned* __restrict__ minbits, float* __restrict__ cs,
                                                       float* __restrict__ rs, double* __restrict__ hs /* [0] sum log noise, [1] sum 1/noise */,
                                                       float* __restrict__ nzf, double* __restrict__ noised) {
    __shared__ double red[16];
    const float nmin = __builtin_bit_cast(float, minbits[0]);
    double sl = 0, sb = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B; i += (int64_t)gridDim.x * 256) {
        const float nz = noise[i], r = nmin / nz;
        rs[i] = r; cs[i] = sqrtf(r);
        sl += log((double)nz); sb += 1.0 / (double)nz;
    }
    sl = block_sum<double>(sl, red); sb = block_sum<double>(sb, red);
    if (threadIdx.x == 0) { atomic_add(hs + 0, sl); atomic_add(hs + 1, sb); }
    if (blockIdx.x == 0 && threadIdx.x == 0) { nzf[0] = nmin; noised[0] = (double)nmin; }
}
__global__ void het_scale_y_kernel(int64_t n, int64_t B, const float* __restrict__ Y, const float* __restrict__ rs, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = Y[i] * rs[i % B];
}
// one wave per 16-column block: lane = (column c = lane % 16, row phase lane / 16); rows m = phase, phase + 4, ...: the T'' reads of one step
// are 4 rows x 64 bytes contiguous.  q_n = (sum_m kpl_mn T''_mn) sigma^2 2^-14 / r_n^2, e_n = (y'_n - U'_n) / r_n.
__global__ __launch_bounds__(256) void het_stats_kernel(int64_t SB, int64_t B, int64_t M, const unsigned short* __restrict__ pl, int64_t pstride,
                                                        const float* __restrict__ Tb /* T'' in 16-column blocks, then U' at Tb + M * SB */,
                                                        const float* __restrict__ ysc, int64_t sY, const float* __restrict__ noise,
                                                        const float* __restrict__ rs, const float* __restrict__ var, double a1, int want_grad,
                                                        float* __restrict__ dnoise, double* __restrict__ sbe2 /* [S] */) {
    const int lane = threadIdx.x & 63, c = lane & 15, ph = lane >> 4;
    const int64_t nb16 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (nb16 * 16 >= SB) return;
    const int64_t n = nb16 * 16 + c;
    float acc = 0.f;
    typedef unsigned int hs_u32x2 __attribute__((ext_vector_type(2)));
    for (int64_t mb = 0; mb < M; mb += 16) {          // (M % 16 == 0) rows mb + 4 ph .. + 3: one 8-byte piece of each plane, four T'' rows
        const int64_t off = ((mb >> 4) * SB + n) * 16 + 4 * ph;
        const hs_u32x2 vh = *reinterpret_cast<const hs_u32x2*>(pl + off), vl = *reinterpret_cast<const hs_u32x2*>(pl + pstride + off);
        const float* tp = Tb + (nb16 * M + mb + 4 * ph) * 16 + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned wh = vh[i >> 1], wl = vl[i >> 1];
            const unsigned short hb = (unsigned short)((i & 1) ? (wh >> 16) : (wh & 0xffffu)), lb = (unsigned short)((i & 1) ? (wl >> 16) : (wl & 0xffffu));
            acc = fmaf((float)__builtin_bit_cast(_Float16, hb) + (float)__builtin_bit_cast(_Float16, lb), tp[i * 16], acc);
        }
    }
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    const int64_t nbr = n % B, s = n / B;
    const double r = (double)rs[nbr], nz = (double)noise[nbr], beta = 1.0 / nz, vk = (double)var[0];
    const double q = (double)acc * vk * (1.0 / 16384.0) / (r * r);
    const double e = ((double)ysc[s * sY + nbr] - (double)Tb[M * SB + n]) / r;
    double be2 = (ph == 0) ? beta * e * e : 0.0;
    // the 16 columns of a block lie in one sample when B % 16 == 0 (host guarantees it): one atomic per wave
    for (int o = 8; o > 0; o >>= 1) be2 += __shfl_xor(be2, o, 64);
    if (lane == 0) atomic_add(sbe2 + s, be2);
    if (want_grad && dnoise && ph == 0) atomic_add(dnoise + nbr, (float)(a1 * (0.5 * beta * beta * e * e - 0.5 * beta + 0.5 * (vk - q) * beta * beta)));
}
template <typename T>
__global__ void svgp_finalize_hets_kernel(int S, int64_t B, int64_t M, const double* __restrict__ scal, const double* __restrict__ sbe2,
                                          const double* __restrict__ hs, const double* __restrict__ noised /* nmin */, const double* __restrict__ var,
                                          const double* __restrict__ sldL, const double* __restrict__ sldLs, const double* __restrict__ trKiSu,
                                          const double* __restrict__ muw, double scaling, double a1, T* __restrict__ logL, double* __restrict__ dvar_direct) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double vk = var[0], bmax = 1.0 / noised[0];
    const double negKL = 0.5 * ((double)M + 2.0 * sldLs[0] - 2.0 * sldL[0] - trKiSu[0]) - 0.5 * muw[0];
    for (int s = 0; s < S; ++s) {
        const double l = -0.5 * (sbe2[s] + (double)B * LOG2PI + hs[0]) - 0.5 * vk * hs[1] + 0.5 * bmax * scal[2 * s];
        logL[s] = (T)(scaling * l + negKL);
    }
    if (dvar_direct) dvar_direct[0] = a1 * (double)S * (-0.5 * hs[1]);
}

// the training call's first launch on the caller's stream: its status words (LAPACK info of the two factorisations, the split scale word)
// cleared in ONE launch instead of a hipMemsetAsync each in front of the kernels of the critical chain (~10 us apiece there)
__global__ void svgp_init_kernel(int* __restrict__ info, int* __restrict__ info2, double* __restrict__ cond_dev) {
    if (threadIdx.x == 0 && info) info[0] = 0;
    if (threadIdx.x < 8) info2[threadIdx.x] = 0;
    // the condition accumulators of THIS call (its norm kernels fold in with atomicMax): cleared here and not only by the previous call's
    // last launch -- a call that returned early (an error between its norm kernels and cond_publish_kernel) must not leak its norms
    if (threadIdx.x < 2) cond_dev[threadIdx.x] = 0.0;
}
// the same launch with the float64 copies of Z, the length-scales and the variance the core works on (and sigma for the whitened tier): three
// more dependent launches in front of the Kuu Gram otherwise
template <typename T>
__global__ __launch_bounds__(256) void svgp_prologue_kernel(int* __restrict__ info, int* __restrict__ info2, double* __restrict__ cond_dev, int64_t nZ,
                                                            const T* __restrict__ Z, double* __restrict__ Zd, int64_t nls, const T* __restrict__ ls,
                                                            double* __restrict__ lsd, const T* __restrict__ var, double* __restrict__ vard,
                                                            float* __restrict__ sig) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && info) info[0] = 0;
        if (threadIdx.x < 8) info2[threadIdx.x] = 0;
        if (threadIdx.x < 2) cond_dev[threadIdx.x] = 0.0;
        if (threadIdx.x == 0) { vard[0] = (double)var[0]; if (sig) sig[0] = sqrtf((float)var[0]); }
        for (int64_t i = threadIdx.x; i < nls; i += blockDim.x) lsd[i] = (double)ls[i];
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nZ; i += (int64_t)gridDim.x * blockDim.x) Zd[i] = (double)Z[i];
}
// sigma = sqrt(variance) as a float word (the whitened tier's planes hold V / sigma * 2^14: |v_n|^2 <= k_nn = variance)
__global__ void svgp_sigma_kernel(const float* __restrict__ var, float* __restrict__ sig) { if (threadIdx.x == 0) sig[0] = sqrtf(var[0]); }

// the training call's last launch: cond_1(Kuu + jitter I) = |K|_1 |K^-1|_1 of this call folded into the running maximum the host can read
// without synchronising (pinned, device-visible memory; mxf_svgp_cond_nowait)
__global__ void cond_publish_kernel(double* __restrict__ cond_dev, double* __restrict__ host_slot /* [0] running max, [1] last */) {
    const double c = cond_dev[0] * cond_dev[1];
    if (c > host_slot[0]) host_slot[0] = c;
    host_slot[1] = c;
    __threadfence_system();
    cond_dev[2] = cond_dev[0]; cond_dev[3] = cond_dev[1];       // kept for mxf_svgp_last_cond
    cond_dev[0] = 0.0; cond_dev[1] = 0.0;                       // the next call's norm kernels accumulate with atomicMax: no memset in front of them
}

// |A|_1 of a symmetric (n x n) float64 matrix: max over rows of the absolute row sum (= column sum), into *out as a double (non-negative
// doubles order like unsigned 64-bit integers: one atomicMax per workgroup; *out must be zeroed).  16 rows per workgroup -- one row per wave
// at a time (coalesced loads + a DPP wave sum, no barrier per row) and ONE atomic per workgroup: n / 16 same-address atomics instead of n
// (they serialise: 1024 of them were most of the 80 us one workgroup per row took on the critical path in front of the Cholesky factorisation).
__global__ __launch_bounds__(256) void norm1_sym16_kernel(int64_t n, const double* __restrict__ A, int64_t lda, double* __restrict__ out) {
    __shared__ double wmax[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double best = 0;
    for (int r = wave; r < 16; r += 4) {
        const int64_t row = (int64_t)blockIdx.x * 16 + r;
        if (row >= n) break;
        double s = 0;
        for (int64_t j = lane; j < n; j += 64) s += fabs(A[row * lda + j]);
        s = wave_sum(s);
        best = s > best ? s : best;
    }
    if (lane == 0) wmax[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = wmax[w] > best ? wmax[w] : best;
        atomicMax(reinterpret_cast<unsigned long long*>(out), __builtin_bit_cast(unsigned long long, best));
    }
}

// One SVGP call: its arguments, its plan (svgp_plan.h), its scratch and the stages that queue its launches.  The stages run in enqueue order,
// which is priority order across the three streams -- the host needs ~5 us per launch and a step has ~280 of them.
template <typename T>
struct SvgpCall : SvgpPlan, SvgpScratch<T> {
    typedef double D;
    mxf_ctx* h; int kind, dtype, S; int64_t B; int Q, P;
    const T* X; int64_t sX; const T* Y; int64_t sY; const T* Z; const T* noise; int64_t nrows; int ncols;
    const T* mu; const T* W; const T* sdiag; const T* ls; int ard; const T* var;
    double jitter, scaling, gscale;
    T* logL; int* info; int want_grad;
    T* dX; T* dY; T* dZ; T* dnoise; T* dmu; T* dW; T* dSdiag; T* dls; T* dvar;
    hipStream_t st;
    SvgpMat<T> mat;
    double a1, bw;                  // gscale * scaling, gscale * S
    const float* split_var;
    SvgpRequest req;
    SvgpSchedule sched;

    SvgpCall(mxf_ctx* h_, const MxfSvgp& d)
        : SvgpScratch<T>(), h(h_), kind(d.kind), dtype(d.dtype), S(d.S), B(d.B), Q(d.Q), P(d.P), X((const T*)d.X), sX(d.sX), Y((const T*)d.Y), sY(d.sY), Z((const T*)d.Z),
          noise((const T*)d.noise), nrows(d.nrows), ncols(d.ncols), mu((const T*)d.mu), W((const T*)d.W), sdiag((const T*)d.sdiag), ls((const T*)d.ls),
          ard(d.ard), var((const T*)d.var), jitter(d.jitter), scaling(d.scaling), gscale(d.gscale), logL((T*)d.logL), info(d.info), want_grad(d.want_grad),
          dX((T*)d.dX), dY((T*)d.dY), dZ((T*)d.dZ), dnoise((T*)d.dnoise), dmu((T*)d.dmu), dW((T*)d.dW), dSdiag((T*)d.dSdiag), dls((T*)d.dls),
          dvar((T*)d.dvar), st((hipStream_t)d.stream),
          mat{(const T*)d.Kuu, (const T*)d.Kuf, (const T*)d.Kdiag, (T*)d.dKuu, (T*)d.dKuf, (T*)d.dKdiag}, a1(d.gscale * d.scaling),
          bw(d.gscale * (double)d.S), split_var((const float*)d.var) {
        M = d.M;
    }
    // (the scratch pointers live in a base that depends on T: named here so that the stages read them as plain members)
    typedef SvgpScratch<T> Sc;
    using Sc::Zd, Sc::lsd, Sc::vard, Sc::noised, Sc::mud, Sc::Wd, Sc::sd, Sc::Lm, Sc::Linv, Sc::Ki, Sc::Su, Sc::Lsinv, Sc::Sui, Sc::KiSu, Sc::H0,
          Sc::tmp, Sc::wd, Sc::sc, Sc::scal, Sc::ad, Sc::hhs, Sc::hbe2, Sc::G, Sc::T1, Sc::AKi, Sc::T2, Sc::dKuu, Sc::dSu, Sc::Gw, Sc::dmud, Sc::dZc,
          Sc::dlsc, Sc::dvc, Sc::Aext, Sc::wT, Sc::Text, Sc::qbuf, Sc::Kuf, Sc::Kfu, Sc::Psi2, Sc::R, Sc::Eb, Sc::aT, Sc::plKfu, Sc::plH0, Sc::plKuf,
          Sc::plLi, Sc::wpl, Sc::plVt, Sc::hsA, Sc::hsK, Sc::hsS, Sc::gscr0, Sc::gscr1, Sc::sigf, Sc::upart, Sc::hcs, Sc::hrs, Sc::hys, Sc::hnz, Sc::info2,
          Sc::hsw, Sc::pVt;

    // float32 mode: the symmetric products of the core -- Ki, H0 and X = Ki G Ki -- as lower tiles + mirror (half the work of a product that
    // runs on the 88 CUs Psi2 leaves in the few-sample regime; the results become exactly symmetric), and the core's reverse mode in the X form.
    // dKuu then comes out exactly symmetric, and its Gram reverse pass skips the row side (dk_symmetric): one condition for both.
    // (The float64 path is the parity path and stays operation for operation what the trajectory tests were recorded with --
    //  tests/test_svgp_notebook.py's 100-epoch float64 run moved its learned noise by 12 % with exactly symmetric Ki / H0, past its 10 % band.)
    static constexpr bool sym_core = sizeof(T) == 4;
    static constexpr int split_mode = MXF_SPLIT_F16X2;
    static constexpr float split_ga = 1.f / 16384.f;     // Gram planes hold k / variance * 2^14 in the f16x2 format

    hipStream_t sd_ = nullptr, s2_ = nullptr;             // h->side, h->side2
    double* cond_slot = nullptr;

    // C = alpha op(A) op(B) + beta C for M x M float64 operands (lower: the lower tiles only)
    int mm(int ta, int tb, double alpha, const D* A, const D* Bm, double beta, D* C, hipStream_t s_, int lower = 0) {
        return mxf_gemm_internal(h, s_, {.dtype = MXF_F64, .ta = ta, .tb = tb, .M = M, .N = M, .K = M, .alpha = alpha, .A = {A, M}, .B = {Bm, M}, .beta = beta,
                                         .C = {C, M}, .lower_only = lower});
    }
    template <typename U> void symmetrize(U* A, hipStream_t s_) {      // mirror the lower triangle of an M x M matrix
        hipLaunchKernelGGL((symmetrize_kernel<U>), dim3((unsigned)((M + 31) / 32), (unsigned)((M + 31) / 32), 1), dim3(256), 0, s_, A, M, M, MM);
    }
    // the accumulate-into gradient outputs: dY and (the caller's Gram not given) dZ, dls, dvar, dX; the core's float64 dZ, dls, dvar
    int clear_grads(hipStream_t s_) {
        if (dY) MXF_HIP(h, hipMemsetAsync(dY, 0, sizeof(T) * (size_t)(ysamp ? (int64_t)S * B : (sY == 0 ? B : SB)) * P, s_));
        if (use_mat) return 0;
        if (dZ) MXF_HIP(h, hipMemsetAsync(dZ, 0, sizeof(T) * M * Q, s_));
        if (dls) MXF_HIP(h, hipMemsetAsync(dls, 0, sizeof(T) * lsn, s_));
        if (dvar) MXF_HIP(h, hipMemsetAsync(dvar, 0, sizeof(T), s_));
        if (dX) MXF_HIP(h, hipMemsetAsync(dX, 0, sizeof(T) * (size_t)SB * Q, s_));
        return 0;
    }
    int clear_core_grads(hipStream_t s_) {
        MXF_HIP(h, hipMemsetAsync(dZc, 0, sizeof(D) * M * Q, s_));
        MXF_HIP(h, hipMemsetAsync(dlsc, 0, sizeof(D) * lsn, s_));
        MXF_HIP(h, hipMemsetAsync(dvc, 0, sizeof(D) * 4, s_));
        return 0;
    }
    void publish_cond() { hipLaunchKernelGGL(cond_publish_kernel, dim3(1), dim3(1), 0, st, h->cond_dev, cond_slot); }

    // the path flags and sizes (svgp_plan.h), the Psi2 / Phi / V schedule with the probe build's knobs, and the scratch
    int plan() {
        req.esize = sizeof(T); req.kind = kind; req.S = S; req.B = B; req.M = M; req.Q = Q; req.P = P; req.sX = sX; req.sY = sY; req.nrows = nrows; req.ncols = ncols;
        req.ard = ard; req.want_grad = want_grad; req.use_mat = mat.Kuu != nullptr; req.form = h->svgp_form; req.x_aligned16 = ((uintptr_t)X % 16) == 0;
        static_cast<SvgpPlan&>(*this) = svgp_plan(req);
        if (refusal) MXF_FAIL(h, rc, "%s", refusal);
        sched = svgp_psi2_schedule(*this, mxf_svgp_knobs());
        size_t need;
        if (!carve_scratch(h, [&](Carver& cv) { this->carve(cv, req, *this); }, need)) MXF_FAIL(h, -4, "mxf_svgp_logpdf: cannot allocate %zu bytes of scratch", need);
        // whitened tier: the planes of V^T (operand (n, k = m) of T = Hh V) go into the THIRD plane slots of the two big buffers (sized for the
        // three-plane bf16 format; the whitened tier runs two-plane f16x2 only) -- the V product writes them next to V's own planes while other
        // workgroups still read the Kfu planes, so they cannot share that buffer's first two slots
        if (whiten) { plVt = plKfu + 2 * pl_big; pVt = (int64_t)((plKuf + 2 * pl_big) - plVt); }
        return 0;
    }

    // caller's stream: the status words, the float64 copies of the Kuu Gram's parameters; het_stream: the row weights
    int prologue() {
        MXF_STAGE(h, "start", st);
        if (!mxf_cond_init(h)) MXF_FAIL(h, -4, "mxf_svgp_logpdf: cannot allocate the condition words");
        cond_slot = h->cond_host + 2 * h->cond_slot;
        for (int i = 0; i < MXF_NT; ++i) h->tm.used[i] = false;
        MXF_T0(h, MXF_T_CALL, st); MXF_T0(h, MXF_T_CHAIN, st);
        if (!use_mat)
            hipLaunchKernelGGL((svgp_prologue_kernel<T>), dim3(gridn(M * Q) > 64 ? 64 : gridn(M * Q)), dim3(256), 0, st, info, info2, h->cond_dev, (int64_t)(M * Q), Z, Zd,
                               (int64_t)lsn, ls, lsd, var, vard, whiten ? sigf : (float*)nullptr);
        else {
            hipLaunchKernelGGL(svgp_init_kernel, dim3(1), dim3(64), 0, st, info, info2, h->cond_dev);
            if (whiten) hipLaunchKernelGGL(svgp_sigma_kernel, dim3(1), dim3(64), 0, st, (const float*)var, sigf);
        }
        if (het_stream) {       // nmin, the row weights, sum log noise / sum beta, y' = r y -- before the fork: both side streams read them
            MXF_HIP(h, hipMemsetAsync(info2 + 5, 0x7f, sizeof(int), st));                 // 0x7f7f7f7f: a huge finite float, above any noise variance
            MXF_HIP(h, hipMemsetAsync(hhs, 0, 4 * sizeof(D), st));
            MXF_HIP(h, hipMemsetAsync(hbe2, 0, (size_t)S * sizeof(D), st));
            const unsigned pg = (unsigned)((B + 255) / 256 > 256 ? 256 : (B + 255) / 256);
            hipLaunchKernelGGL(het_min_kernel, dim3(pg), dim3(256), 0, st, B, (const float*)noise, (unsigned*)(info2 + 5));
            hipLaunchKernelGGL(het_prep_kernel, dim3(pg), dim3(256), 0, st, B, (const float*)noise, (const unsigned*)(info2 + 5), hcs, hrs, hhs, hnz, noised);
            const int64_t ny = sY == 0 ? B : SB;
            hipLaunchKernelGGL(het_scale_y_kernel, dim3(gridn(ny)), dim3(256), 0, st, ny, B, (const float*)Y, (const float*)hrs, hys);
        }
        return 0;
    }

    // caller's stream: Kuu (+ jitter), then the fork of the two side streams.  The core runs in float64, once; two independent chains run
    // concurrently (main: Kuu -> L -> Ki, w; side: Kuf_all, Su -> Ls -> Su^-1)
    int kuu_fork() {
        if (!mxf_side_init(h)) MXF_FAIL(h, -5, "mxf_svgp_logpdf: cannot create the internal side stream");
        sd_ = h->side; s2_ = h->side2;
        if (use_mat) {
            copy_convert(MM, mat.Kuu, Lm, st);
            if (jitter != 0.0) hipLaunchKernelGGL(add_diag_kernel, dim3(gridn(M)), dim3(256), 0, st, M, Lm, jitter);
        } else {
            const int rc = kuu_f64(h, st, kind, M, Q, Zd, lsd, ard, vard, jitter, Lm);   // Kuu (+jitter) :69-72
            if (rc) return rc;
        }
        MXF_HIP(h, hipEventRecord(h->ev_fork, st));
        MXF_HIP(h, hipStreamWaitEvent(sd_, h->ev_fork, 0));
        MXF_HIP(h, hipStreamWaitEvent(s2_, h->ev_fork, 0));
        return 0;
    }

    // second side stream, first thing: Su (H0 on the critical path needs it; its Cholesky comes later and is off the critical path).  Everything
    // the Kuu chain does not need itself -- noise, mu, W, diag(s), the scalar accumulators -- is prepared here too; the main stream waits for
    // ev_su before it first touches them.
    int su_side2() {
        MXF_HIP(h, hipMemsetAsync(sc, 0, 16 * sizeof(D), s2_));
        MXF_HIP(h, hipMemsetAsync(scal, 0, 2 * (size_t)S * sizeof(D), s2_));
        // the accumulate-into outputs of the fused reverse pass and of the core's reverse mode are cleared HERE, on the second side stream at
        // the start of the call (it joins the caller's stream before the reverse pass): between the T product and the reverse pass on the
        // critical path these nine fills cost ~10 us of queue latency apiece (0.1 ms of a 4.6 ms per-rank step)
        if (fused) {           // (fused: neither ysamp nor use_mat)
            if (int rc = clear_grads(s2_)) return rc;
            MXF_HIP(h, hipMemsetAsync(R, 0, sizeof(T) * MP, s2_));
            if (int rc = clear_core_grads(s2_)) return rc;
        }
        if (!het && !het_stream) copy_convert((int64_t)1, noise, noised, s2_);
        copy_convert(MP, mu, mud, s2_);
        copy_convert(MM, W, Wd, s2_);
        copy_convert(M, sdiag, sd, s2_);
        hipLaunchKernelGGL((diag_embed_kernel<D>), dim3(gridn(MM)), dim3(256), 0, s2_, M, (const D*)sd, Su);
        const int rc = mm(0, 1, 1.0, Wd, Wd, 1.0, Su, s2_);       // Su = W W^T + diag(s) :76
        if (rc) return rc;
        MXF_HIP(h, hipEventRecord(h->ev_su, s2_));           // H0 needs Su only; its Cholesky (log-det, Su^-1 for the reverse mode) is OFF the critical path
        MXF_STAGE(h, "Su formed (s2)", s2_);
        return 0;
    }

    // side stream: Kuf_all (as a Gram or as split planes; whitened: the Kfu planes), Kfu_all and Psi2.  Queued before the Kuu chain: these few
    // launches carry the bulk of the device work.
    int kuf_psi2() {
        int rc;
        if (use_mat) {
            Kuf = const_cast<T*>(mat.Kuf);          // the caller's Gram is only ever read (a copy into the scratch: 268 MB, 0.13 ms at 512 x 131 072)
        } else if (whiten) {
            // whitened tier: only the Kfu planes (operand (n, k = m) of V = L^-1 Kuf); they need nothing from the core, so they are written
            // first; V, its transposition (+ U = a^T V) and Phi = V V^T follow on this stream once L^-1 exists (whiten_v_phi)
            MXF_T0(h, MXF_T_PLANES_A, sd_);
            rc = mxf_gram_planes_internal(h, sd_, {.kind = kind, .R = SB, .Kn = M, .Q = Q, .Xmin = (const float*)X, .Xmaj = (const float*)Z, .ls = (const float*)ls,
                                                   .ard = ard, .var = (const float*)var, .planes = plKfu, .pstride = (int64_t)pl_big, .scratch = gscr1});
            if (rc) return rc;
            MXF_T1(h, MXF_T_PLANES_A, sd_);
            MXF_STAGE(h, "Kfu planes (sd)", sd_);
        } else if (use_split) {
            // float32 training step: the Grams are written directly as split planes (two scaled f16 terms = 4 bytes per element, never as f32):
            // Kuf planes (operand (m, k = n)) feed Psi2 and come first so that Psi2 (MFMA bound) starts early; the Kfu planes (operand
            // (n, k = m): T GEMM and the w^T Kuf row) are then written (HBM bound) on the second side stream NEXT TO Psi2 (su_chain), unless
            // the T product reads these planes (bt_path).
            MXF_T0(h, MXF_T_PLANES_A, sd_);
            rc = mxf_gram_planes_internal(h, sd_, {.kind = kind, .R = M, .Kn = SB, .Q = Q, .Xmin = (const float*)Z, .Xmaj = (const float*)X, .ls = (const float*)ls,
                                                   .ard = ard, .var = (const float*)var, .planes = plKuf, .pstride = (int64_t)pl_big, .scratch = gscr0,
                                                   .majs = het_stream ? (const float*)hcs : nullptr, .period = B});
            if (rc) return rc;
            MXF_T1(h, MXF_T_PLANES_A, sd_);
            MXF_STAGE(h, "Kuf planes (sd)", sd_);
            if (bt_path) MXF_HIP(h, hipEventRecord(h->ev_aux, sd_));     // the T product reads THESE planes
        } else {
            rc = cross_gram(h, sd_, kind, dtype, Q, M, Z, SB, X, ls, ard, var, Kuf);          // Kuf_all = k(Z, X_all) :73
            if (rc) return rc;
        }
        if (!use_split) MXF_HIP(h, hipEventRecord(h->ev_aux, sd_));          // Kuf ready: the T GEMM waits for it
        if (!fused || whiten) return 0;
        // Psi2 = Kuf Kuf^T in the two launches of the schedule (svgp_plan.h), lower blocks only, split-K.  float32: from the split planes of Kuf
        // (gemm_split.hip); float64 / fallback: from the TRANSPOSED Gram Kfu (S*B x M, rows = contiguous lines) as a TN GEMM (the NT form on Kuf
        // reads 256 K-strided streams per workgroup).
        const int64_t KA = sched.KA;
        MXF_T0(h, MXF_T_PSI2, sd_);
        if (use_split) {
            const MxfSplitScale kuf2 = {.alpha = (double)split_ga * split_ga, .ad0 = split_var, .pow0 = 2};      // both operands are Kuf planes: k / variance 2^14
            if (KA > 0) {
                rc = mxf_gemm_split_internal(h, sd_, split_mode, M, M, KA, kuf2, {plKuf, (int64_t)pl_big}, {plKuf, (int64_t)pl_big},
                                             {.C = (float*)Psi2, .ldc = M, .lower_only = 1}, {.reserve_cus = sched.reserve_a});
                if (rc) return rc;
            }
            if (KA < SB) {
                const unsigned short* pk = plKuf + (KA / 16) * M * 16;
                rc = mxf_gemm_split_internal(h, sd_, split_mode, M, M, SB - KA, kuf2, {pk, (int64_t)pl_big}, {pk, (int64_t)pl_big},
                                             {.C = (float*)Psi2, .ldc = M, .beta = KA > 0 ? 1.0 : 0.0, .lower_only = 1}, {.reserve_cus = sched.reserve_b});
                if (rc) return rc;
            }
        } else {
            rc = cross_gram(h, sd_, kind, dtype, Q, SB, X, M, Z, ls, ard, var, Kfu);
            if (rc) return rc;
            if (KA > 0) {
                rc = mxf_gemm_internal(h, sd_, {.dtype = dtype, .ta = 1, .M = M, .N = M, .K = KA, .A = {Kfu, M}, .B = {Kfu, M}, .C = {Psi2, M}, .lower_only = 1,
                                                .reserve_cus = sched.reserve_a});
                if (rc) return rc;
            }
            if (KA < SB) {
                rc = mxf_gemm_internal(h, sd_, {.dtype = dtype, .ta = 1, .M = M, .N = M, .K = SB - KA, .A = {Kfu + KA * M, M}, .B = {Kfu + KA * M, M},
                                                .beta = KA > 0 ? 1.0 : 0.0, .C = {Psi2, M}, .lower_only = 1, .reserve_cus = sched.reserve_b});
                if (rc) return rc;
            }
        }
        symmetrize(Psi2, sd_);
        MXF_T1(h, MXF_T_PSI2, sd_);
        MXF_STAGE(h, "Psi2 (sd)", sd_);
        MXF_HIP(h, hipEventRecord(h->ev_join2, sd_));
        return 0;
    }

    // caller's stream: Kuu -> L -> L^-1 (the critical path up to the T GEMM); |Kuu|_1 on the second side stream
    int kuu_chain() {
        // condition number of Kuu + jitter I (1-norm), for the float32 validity check of mxf_svgp_last_cond: |Kuu|_1 here, |Ki|_1 in value_scalars.
        // What the T product does not need leaves the caller's stream -- the two condition norms (64 workgroups walking 16 rows each: 0.05 ms
        // alone, 0.22 ms in front of the factorisation while the planes pass holds every CU), mu.w, tr(Ki Su), log|Kuu| go to the second side
        // stream.  Kuu is copied for its norm (the factorisation works in place) into Su^-1's buffer, which the end of the Su chain writes on the
        // same stream as the norm.
        copy_convert(MM, (const D*)Lm, Sui, st);
        MXF_HIP(h, hipEventRecord(h->ev_k1, st));
        MXF_HIP(h, hipStreamWaitEvent(s2_, h->ev_k1, 0));
        hipLaunchKernelGGL(norm1_sym16_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, s2_, M, (const double*)Sui, M, h->cond_dev);
        int rc = potrf_f64(h, st, M, Lm, info, true);                                                          // L :83 (trtri / sumlogdiag read the lower triangle only)
        if (rc) return rc;
        MXF_STAGE(h, "potrf Kuu", st);
        rc = trtri_f64(h, st, M, Lm, Linv);
        if (rc) return rc;
        MXF_STAGE(h, "trtri Kuu", st);
        return 0;
    }

    // whitened tier: the planes of L^-1 and a = L^-1 mu on the caller's stream; V = L^-1 Kuf, U = a^T V and Phi = V V^T on the side stream
    int whiten_v_phi() {
        if (!whiten) return 0;
        unsigned* limax = (unsigned*)(info2 + 4);           // bit pattern of max |L^-1| (word cleared by svgp_init_kernel)
        // L^-1 as f16x2 planes (the A operand of V = L^-1 Kuf); Aext is free until Hh is formed
        hipLaunchKernelGGL((convert_kernel<D, T>), dim3(gridn(MM)), dim3(256), 0, st, M, M, (const D*)Linv, M, Aext, M);
        int rc = mxf_maxabs_internal(h, M, M, (const float*)Aext, M, limax, st, false);
        if (rc) return rc;
        rc = mxf_split_planes_internal(h, M, M, (const float*)Aext, M, plLi, st, MXF_SPLIT_F16X2, limax);
        if (rc) return rc;
        // a = L^-1 mu (float64, then the streaming dtype): the V product's epilogue forms U = a^T V from it
        MXF_HIP(h, hipStreamWaitEvent(st, h->ev_su, 0));                                              // mu (second side stream)
        hipLaunchKernelGGL((trmv_lower_kernel<D>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, M, P, (const D*)Linv, M, (const D*)mud, (int64_t)P, ad);
        copy_convert(MP, (const D*)ad, aT, st);
        MXF_HIP(h, hipEventRecord(h->ev_aux2, st));                                                   // L^-1 planes and a ready
        // side stream: V = L^-1 Kuf, written as the planes of the (m, k = n) operand holding V / sigma * 2^14 (|v_n|^2 <= k_nn = sigma^2):
        // acc = (s_L L^-1) (Kfu / sigma^2 2^14)^T  ->  acc sigma / s_L.  L^-1 is lower triangular: a row tile's k loop stops at its last row.
        // Without bt_wh the SAME launch writes the planes of V^T (the (n, k = m) operand of T = Hh V) and, for one output column, the 128-row
        // partial sums of U = a^T V (a separate transposition + U pass over the planes took 3.3 ms of the 35 ms step -- 17 GB of traffic).
        MXF_HIP(h, hipStreamWaitEvent(sd_, h->ev_aux2, 0));
        MXF_T0(h, MXF_T_VGEMM, sd_);
        const bool vt = !bt_wh, u1 = vt && P == 1;      // (bt_wh: planes of V only -- T and U come from them, gemm_bt.hip)
        MxfSplitOut v = {.planes = plKuf, .pstride = (int64_t)pl_big, .a_lower = 1};
        if (vt) { v.planes_t = plVt; v.pstride_t = pVt; }
        if (u1) { v.avec = (const float*)aT; v.Upart = upart; }
        rc = mxf_gemm_split_internal(h, sd_, split_mode, M, SB, M, {.alpha = 1.0, .ad0 = sigf, .pow0 = 1}, {plLi, (int64_t)pl_h0, (const unsigned*)limax},
                                     {plKfu, (int64_t)pl_big}, v, {.reserve_cus = sched.reserve_v});
        if (rc) return rc;
        MXF_T1(h, MXF_T_VGEMM, sd_);
        MXF_STAGE(h, "V = Linv Kuf (sd)", sd_);
        MXF_T0(h, MXF_T_PLANES_B, sd_);
        if (!bt_wh) {           // U = a^T V: the V product's partial sums reduced (P = 1), or one pass over the V^T planes
            if (P == 1) {
                rc = mxf_upart_reduce_internal(h, SB, (int)(M / 128), upart, sigf, 1.f / 16384.f, (float*)(Text + M * SB), sd_);
                if (rc) return rc;
            } else {
                hipLaunchKernelGGL((wt_planes_kernel<8, 2>), dim3((unsigned)((SB + 255) / 256)), dim3(256), 0, sd_, M, SB, P, (const unsigned short*)plVt,
                                   pVt, (const float*)aT, (float*)(Text + M * SB), (const float*)sigf);
            }
        }
        MXF_T1(h, MXF_T_PLANES_B, sd_);
        MXF_HIP(h, hipEventRecord(h->ev_aux, sd_));      // V^T planes and U ready: the T GEMM / the reverse pass wait for it
        // Phi = V V^T (lower tiles, split-K) = sigma^2 2^-28 (planes)(planes)^T
        MXF_T0(h, MXF_T_PSI2, sd_);
        rc = mxf_gemm_split_internal(h, sd_, split_mode, M, M, SB, {.alpha = (double)split_ga * split_ga, .ad0 = split_var, .pow0 = 1},
                                     {plKuf, (int64_t)pl_big}, {plKuf, (int64_t)pl_big}, {.C = (float*)Psi2, .ldc = M, .lower_only = 1},
                                     {.reserve_cus = sched.reserve_phi});
        if (rc) return rc;
        symmetrize(Psi2, sd_);
        MXF_T1(h, MXF_T_PSI2, sd_);
        MXF_STAGE(h, "Phi (sd)", sd_);
        return 0;
    }

    // caller's stream: Ki = L^-T L^-1, w = Ki mu (one wave per row) and its streaming-dtype copy
    int ki_w() {
        const int rc = mm(1, 0, 1.0, Linv, Linv, 0.0, Ki, st, sym_core);   // Ki = Linv^T Linv
        if (rc) return rc;
        if (sym_core) symmetrize(Ki, st);
        MXF_HIP(h, hipStreamWaitEvent(st, h->ev_su, 0));                                                  // Su, mu, noise, accumulators (second side stream)
        hipLaunchKernelGGL((gemv_rows_kernel<D>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, M, P, (const D*)Ki, M, (const D*)mud, (int64_t)P, wd);   // w = Ki mu
        copy_convert(MP, (const D*)wd, wT, st);                                                          // w in the streaming dtype
        MXF_STAGE(h, "Ki, w", st);
        if (use_split && !whiten) MXF_HIP(h, hipEventRecord(h->ev_aux2, st));                             // w ready: the Kfu planes + U pass may start
        return 0;
    }

    // second side stream: Su -> Ls -> log|Su|, Su^-1; then (split path without bt_path) the Kfu planes and U = w^T Kuf
    int su_chain() {
        // (a plain kernel, not hipMemcpyAsync: the runtime's copy path sat idle for ~1 ms before it started next to busy queues -- r02 timeline:
        //  the Su chain did not begin until 1.66 ms although nothing in the Kuu chain feeds it)
        copy_convert(MM, (const D*)Su, tmp, s2_);
        int rc = potrf_f64(h, s2_, M, tmp, info2, true);                                                      // Ls = chol(Su) :84
        if (rc) return rc;
        MXF_STAGE(h, "potrf Su (s2)", s2_);
        rc = sumlogdiag_f64(h, s2_, M, tmp, sc + 1);
        if (rc) return rc;
        if (want_grad) {
            rc = trtri_f64(h, s2_, M, tmp, Lsinv);
            if (rc) return rc;
            rc = mm(1, 0, 1.0, Lsinv, Lsinv, 0.0, Sui, s2_);
            if (rc) return rc;
        }
        MXF_STAGE(h, "Su^-1 (s2)", s2_);
        MXF_HIP(h, hipEventRecord(h->ev_join, s2_));
        if (use_split && !whiten && !bt_path) {
            // Kfu planes (operand (n, k = m) of the T GEMM) + the row U = w^T Kuf in ONE pass, behind the Su chain on the second side stream:
            // HBM-write bound.  (r03, tests/probes/svgp_stages.py: the pass starts when w = Kuu^-1 mu exists, and the Kuu chain -- potrf, trtri,
            // Ki -- shares the chip with the Kuf planes pass and Psi2 and finishes just after Psi2: 0.9 / 1.4 / 1.6 ms at 4 samples against 0.6
            // alone.  A stream of its own for this pass changes nothing: H0, hence the T GEMM, waits for the same chain.)
            MXF_HIP(h, hipStreamWaitEvent(s2_, h->ev_aux2, 0));
            MXF_T0(h, MXF_T_PLANES_B, s2_);
            rc = mxf_gram_planes_internal(h, s2_, {.kind = kind, .R = SB, .Kn = M, .Q = Q, .Xmin = (const float*)X, .Xmaj = (const float*)Z, .ls = (const float*)ls,
                                                   .ard = ard, .var = (const float*)var, .planes = plKfu, .pstride = (int64_t)pl_big, .scratch = gscr1,
                                                   .w = (const float*)wT, .Pw = P, .U = (float*)(Text + M * SB), .ldU = SB,
                                                   .mins = het_stream ? (const float*)hrs : nullptr, .period = B});
            if (rc) return rc;
            MXF_T1(h, MXF_T_PLANES_B, s2_);
            MXF_STAGE(h, "Kfu planes + U (s2)", s2_);
            MXF_HIP(h, hipEventRecord(h->ev_aux, s2_));      // Kfu planes and U ready: the T GEMM / the reverse pass wait for it
        }
        return 0;
    }

    // caller's stream: Ki Su, H0 = Ki - Ki Su Ki (whitened: Hh = L^-T - Ki Su L^-T), A_ext = H0 in the streaming dtype (split path: its planes)
    int h0_planes() {
        MXF_HIP(h, hipStreamWaitEvent(st, h->ev_su, 0));                                                  // Su formed (second side stream)
        int rc = mm(0, 0, 1.0, Ki, Su, 0.0, KiSu, st);
        if (rc) return rc;
        if (whiten) {
            // Hh = L^-T (I - A_s A_s^T) = L^-T - Ki Su L^-T   (T = Hh V; |Hh| ~ sqrt(cond) where |H0| ~ cond)
            hipLaunchKernelGGL((transpose_convert_kernel<D, D>), dim3(gridn(MM)), dim3(256), 0, st, M, M, (const D*)Linv, M, H0, M);
            rc = mm(0, 1, -1.0, KiSu, Linv, 1.0, H0, st);
            if (rc) return rc;
        } else {
            copy_convert(MM, (const D*)Ki, H0, st);     // H0 <- Ki (a plain kernel: the runtime's copy engine path costs ~10x as much next to busy queues)
            rc = mm(0, 0, -1.0, KiSu, Ki, 1.0, H0, st, sym_core);     // H0 = Ki - Ki Su Ki
            if (rc) return rc;
            if (sym_core) symmetrize(H0, st);
        }
        if (use_split) {
            // H0 -> float32 and the bit pattern of max |H0| (the power-of-two scale of its f16x2 planes; word cleared by svgp_init_kernel) in one launch
            unsigned* h0max = (unsigned*)(info2 + 2);
            hipLaunchKernelGGL(convert_max_kernel, dim3((unsigned)(gridn(MM) > 256 ? 256 : gridn(MM))), dim3(256), 0, st, MM, (const D*)H0, (float*)Aext, h0max);
            rc = mxf_split_planes_internal(h, M, M, (const float*)Aext, M, plH0, st, split_mode, h0max);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL((convert_kernel<D, T>), dim3(gridn(MM)), dim3(256), 0, st, M, M, (const D*)H0, M, Aext, M);
        }
        MXF_T1(h, MXF_T_CHAIN, st);
        MXF_STAGE(h, "H0 planes", st);
        MXF_HIP(h, hipEventRecord(h->ev_fork, st));                                                       // core (Ki, KiSu, H0, w) ready
        return 0;
    }

    // second side stream, behind the Su chain: |Ki|_1, mu.w, tr(Ki Su), log|Kuu|; the caller's stream picks them up behind the T product
    int value_scalars() {
        MXF_HIP(h, hipStreamWaitEvent(s2_, h->ev_fork, 0));
        hipLaunchKernelGGL(norm1_sym16_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, s2_, M, (const double*)Ki, M, h->cond_dev + 1);
        hipLaunchKernelGGL((dot_kernel<D>), dim3(dotgrid(MP)), dim3(256), 0, s2_, MP, (const D*)mud, (const D*)wd, 1.0, sc + 3);
        hipLaunchKernelGGL((dot_kernel<D>), dim3(dotgrid(MM)), dim3(256), 0, s2_, MM, (const D*)Ki, (const D*)Su, 1.0, sc + 2);
        const int rc = sumlogdiag_f64(h, s2_, M, Lm, sc + 0);
        if (rc) return rc;
        MXF_HIP(h, hipEventRecord(h->ev_k3, s2_));
        return 0;
    }

    // caller's stream: [T; U] = [H0; w^T] Kuf_all
    int t_product() {
        MXF_HIP(h, hipStreamWaitEvent(st, h->ev_aux, 0));                                                 // Kuf_all from the side stream
        // (in-step timing only: the T product is held until Psi2 has finished, so that `t_gemm` is the product's own duration -- untimed, its
        //  first workgroups take the CUs Psi2's last work items free, and the event pair would count that queueing)
        if (h->tm.on && bt_path) MXF_HIP(h, hipStreamWaitEvent(st, h->ev_join2, 0));
        MXF_T0(h, MXF_T_TGEMM, st);
        int rc;
        // split path: planes of H0 (scaled from max |H0|) x planes of Kuf (k / variance 2^14).  The whitened tier is the same product with Hh for
        // H0, V for Kuf (V / sigma 2^14), a for w.  Both write max |T| for the reverse pass (word cleared by svgp_init_kernel).
        const MxfSplitScale tscale = {.alpha = (double)split_ga, .ad0 = whiten ? sigf : split_var, .pow0 = 1};
        const MxfPlanes h0 = {plH0, (int64_t)pl_h0, (const unsigned*)(info2 + 2)};
        const MxfSplitOut tout = {.C = (float*)Text, .ldc = SB, .blocked = t_blocked, .maxout = (unsigned*)(info2 + 3)};
        if (bt_path || bt_wh)     // T = H0 Kuf straight from the planes Psi2 reads, U = w^T Kuf from the same fragments (gemm_bt.hip)
            rc = mxf_gemm_bt_internal(h, st, M, SB, M, tscale, h0, {plKuf, (int64_t)pl_big}, M, tout,
                                      {.w = whiten ? (const float*)aT : (const float*)wT, .U = (float*)(Text + M * SB), .uscale = 1.0 / 16384.0, .wscratch = wpl});
        else if (use_split)       // T = H0 Kuf = H0 Kfu^T on the 16-bit matrix pipe (f32-equivalent splitting, gemm_split.hip)
            rc = mxf_gemm_split_internal(h, st, split_mode, M, SB, M, tscale, h0, {whiten ? plVt : plKfu, whiten ? pVt : (int64_t)pl_big}, tout);
        else if (het_split) {
            rc = mxf_maxabs_internal(h, M, M, (const float*)Aext, M, hsw + 0, st);
            if (!rc) rc = mxf_split_planes_internal(h, M, M, (const float*)Aext, M, hsA, st, MXF_SPLIT_F16X2, hsw + 0);
            if (!rc) rc = mxf_maxabs_internal(h, M, SB, (const float*)Kuf, SB, hsw + 1, st);
            if (!rc) rc = mxf_split_planes_internal(h, M, SB, (const float*)Kuf, SB, hsK, st, MXF_SPLIT_F16X2, hsw + 1);      // (m, k = n): the K-major operand of T, the row operand of G'
            if (!rc) rc = mxf_gemm_bt_internal(h, st, M, SB, M, {.alpha = 1.0}, {hsA, (int64_t)pl_h0, hsw + 0}, {hsK, (int64_t)pl_big, hsw + 1}, M,
                                               {.C = (float*)Text, .ldc = SB});
        } else
            rc = mxf_gemm_internal(h, st, {.dtype = dtype, .M = M, .N = SB, .K = M, .A = {Aext, M}, .B = {Kuf, SB}, .C = {Text, SB}});   // T = H0 Kuf (MFMA)
        if (rc) return rc;
        MXF_T1(h, MXF_T_TGEMM, st);
        MXF_STAGE(h, "T", st);
        if (use_split) return 0;          // (U = w^T Kuf was written with the Kfu planes or by the T product)
        constexpr int VEC = Vec16<T>::n;
        dim3 gu((unsigned)((SB + 256 * VEC - 1) / (256 * VEC)));
        if (gu.x <= 256 && M >= 64) {            // few columns: split the rows as well (the kernel then adds into U)
            // (up to one workgroup per CU -- 512 x 131 072, the deep GP's first layer, was 128 workgroups walking 512 dependent rows: 0.24 ms)
            int64_t ch = 1024 / gu.x; if (ch > M / 16) ch = M / 16; if (ch > 64) ch = 64;
            if (ch > 1) { gu.y = (unsigned)ch; MXF_HIP(h, hipMemsetAsync(Text + M * SB, 0, sizeof(T) * (size_t)P * SB, st)); }
        }
        if (P == 1) hipLaunchKernelGGL((wt_kuf_kernel<T, 1>), gu, dim3(256), 0, st, M, SB, P, (const T*)Kuf, (const T*)wT, Text + M * SB);
        else hipLaunchKernelGGL((wt_kuf_kernel<T, 8>), gu, dim3(256), 0, st, M, SB, P, (const T*)Kuf, (const T*)wT, Text + M * SB);   // U = w^T Kuf
        return 0;
    }

    // dW = 2 dSu W (into Lsinv's buffer, free by then) and dSdiag = diag(dSu), on stream s_
    int dsu_outputs(hipStream_t s_) {
        if (dW) {
            const int rc = mm(0, 0, 2.0, dSu, Wd, 0.0, Lsinv, s_);
            if (rc) return rc;
            hipLaunchKernelGGL((add_convert_kernel<D, T>), dim3(gridn(MM)), dim3(256), 0, s_, MM, (T)1, (const D*)Lsinv, dW, 0);
        }
        if (dSdiag) hipLaunchKernelGGL((diag_extract_kernel<D, T>), dim3(gridn(M)), dim3(256), 0, s_, M, (const D*)dSu, M, dSdiag);
        return 0;
    }

    // the part of the core reverse mode that depends on Psi2 only (not on R), in the float64 flow: dSu = -Ki G Ki + bP/2 (Su^-1 - Ki),
    // dW = 2 dSu W, dSdiag = diag(dSu), with_t1: T1 = G Ki Su.  Forming A_Ki = G - G Ki Su - ... FIRST and multiplying by Ki afterwards cancels
    // before it amplifies; the X form (float32) multiplies first and loses ~2 digits on ill-conditioned Kuu (uncertain-input toy of
    // tests/test_gpu_config4.py, cond ~ 1e6: float64 lengthscale gradient 8.6e-10 -> 5.8e-8 against the oracle) -- nothing next to float32
    // streaming (1e-5), but the float64 path is the parity path.
    int su_reverse(hipStream_t s_, bool with_t1) {
        int rc = mm(0, 0, 1.0, Ki, G, 0.0, tmp, s_);            // T3 = Ki G
        if (rc) return rc;
        hipLaunchKernelGGL((axpby_kernel<D>), dim3(gridn(MM)), dim3(256), 0, s_, MM, 1.0, (const D*)Sui, -1.0, (const D*)Ki, dSu);   // Sui - Ki
        rc = mm(0, 0, -1.0, tmp, Ki, 0.5 * bw * P, dSu, s_);
        if (rc) return rc;
        rc = dsu_outputs(s_);
        if (rc) return rc;
        if (with_t1) rc = mm(0, 0, 1.0, G, KiSu, 0.0, T1, s_);           // T1 = G Ki Su
        return rc;
    }

    // side stream, fused path: the R-independent part of the core's reverse mode, right behind Psi2 -- it runs under the T GEMM / the reverse
    // pass instead of in the step's tail
    int core_reverse_side() {
        if (!fused) return 0;
        MXF_HIP(h, hipStreamWaitEvent(sd_, h->ev_fork, 0));      // Ki, KiSu, H0 (main)
        MXF_HIP(h, hipStreamWaitEvent(sd_, h->ev_join, 0));      // Su^-1; `tmp` (chol(Su)) is free from here on
        int rc;
        if (!sym_core) {
            hipLaunchKernelGGL((scale_beta_kernel<T>), dim3(gridn(MM)), dim3(256), 0, sd_, MM, (const T*)Psi2, (const D*)noised, 0.5 * P * a1, G);
            rc = su_reverse(sd_, true);
            if (rc) return rc;
        } else {
            // float32: the whole R-independent part, dKuu0 included, from X = Ki G Ki (G = c Psi2, c = P a1 beta / 2):
            //   dSu   = -X + bP/2 (Su^-1 - Ki)
            //   dKuu0 = -Ki A0 Ki - bP/2 Ki,  A0 = G - T1 - T1^T - b (P/2 Su + 1/2 mu mu^T),  T1 = G Ki Su
            //         = -X + Y + Y^T + b (P/2 Ki Su Ki + 1/2 w w^T) - bP/2 Ki,  Y = X (Ki Su)^T,  Ki Su Ki = Ki - H0 (explicit form)
            // i.e. FOUR M^3 products (Ki G, . Ki, dSu W, X (Ki Su)^T) where the float64 flow takes six (Ki G, . Ki, dSu W, G Ki Su, Ki A, . Ki), the
            // last two of them in the step's tail behind the reverse pass.  Whitened form: X = c L^-T Phi L^-1 directly (Phi = V V^T; G = c L Phi L^T
            // is never formed) + Ki Su Ki as a product: five instead of eight.  These products run on the CUs the T product leaves free (few samples:
            // 40), so their number is the length of the side stream: stage stamps at 4 samples, six-product flow: Su reverse ends 3.70 ms, reverse
            // pass 3.54, end 3.97.
            // X = F^T Gc F (symmetric: lower tiles, mirrored) -- G = c Psi2 and F = Ki, or whitened: c Phi and F = L^-1
            D* Xb = whiten ? G : T2;
            D* Gc = whiten ? T2 : G;
            const D* F = whiten ? Linv : Ki;
            hipLaunchKernelGGL((scale_beta_kernel<T>), dim3(gridn(MM)), dim3(256), 0, sd_, MM, (const T*)Psi2, (const D*)noised, 0.5 * P * a1, Gc);
            if (whiten) hipLaunchKernelGGL((trace_kernel<D>), dim3(1), dim3(256), 0, sd_, M, (const D*)T2, M, (int64_t)0, sc + 6);          // c tr(Phi)
            rc = mm(whiten ? 1 : 0, 0, 1.0, F, Gc, 0.0, tmp, sd_);
            if (rc) return rc;
            rc = mm(0, 0, 1.0, tmp, F, 0.0, Xb, sd_, sym_core);
            if (rc) return rc;
            symmetrize(Xb, sd_);
            if (whiten) hipLaunchKernelGGL(dot_t_kernel, dim3(dotgrid(MM)), dim3(256), 0, sd_, M, (const D*)Su, (const D*)Xb, sc + 7);   // tr(Su X): the accurate total of the q_n
            hipLaunchKernelGGL(dsu_kernel, dim3(gridn(MM)), dim3(256), 0, sd_, MM, (const D*)Xb, (const D*)Sui, (const D*)Ki, 0.5 * bw * P, dSu);
            rc = dsu_outputs(sd_);
            if (rc) return rc;
            rc = mm(0, 1, 1.0, Xb, KiSu, 0.0, T1, sd_);             // Y = X (Ki Su)^T
            if (rc) return rc;
            if (whiten) {
                rc = mm(0, 0, 1.0, KiSu, Ki, 0.0, AKi, sd_);        // Ki Su Ki (H0 holds Hh in this form)
                if (rc) return rc;
            }
            hipLaunchKernelGGL(dkuu0_kernel, dim3(gridn(MM)), dim3(256), 0, sd_, M, P, (const D*)Xb, (const D*)T1, (const D*)Ki, whiten ? (const D*)AKi : (const D*)nullptr,
                               (const D*)H0, (const D*)wd, bw, dKuu);
        }
        MXF_STAGE(h, "Su reverse (sd)", sd_);
        MXF_HIP(h, hipEventRecord(h->ev_join2, sd_));            // Psi2, G, T1, dSu outputs (float32 mode: dKuu0 as well)
        return 0;
    }

    // caller's stream: the pass over T (value terms and the Kuf-side reverse mode) and logL.  !want_grad: the call ends here.
    int reverse_pass() {
        MXF_HIP(h, hipStreamWaitEvent(st, h->ev_join, 0));      // Su chain complete (log-det for the value, Su^-1 for the reverse mode); hidden under the T GEMM
        MXF_HIP(h, hipStreamWaitEvent(st, h->ev_k3, 0));      // ... and the condition norms and value scalars behind it
        const int dY_shared = (sY == 0 && SS > 1) ? 1 : 0;
        D* dnz = fused ? sc + 4 : nullptr;           // dnoise, dvar_direct
        D* dvdir = want_grad ? sc + 5 : nullptr;
        int rc;
        if (het) {
            if (want_grad) {
                if ((rc = clear_grads(st))) return rc;
                if (dnoise) MXF_HIP(h, hipMemsetAsync(dnoise, 0, sizeof(T) * (size_t)nrows * ncols, st));
            }
            T* Ksc = Kfu;   // the transposed-Gram slot is unused on this path
            MXF_HIP(h, hipMemsetAsync(qbuf, 0, sizeof(T) * (size_t)SB, st));
            hipLaunchKernelGGL((svgp_het_rows_kernel<T>), dim3((unsigned)((SB + 255) / 256), (unsigned)((M + HET_RCH - 1) / HET_RCH)), dim3(256), 0, st, SB, B, M,
                               P, SYc, (const T*)Kuf, Text, Y, sY, (const T*)wT, noise, nrows, ncols, a1, want_grad, Ksc, qbuf);
            hipLaunchKernelGGL((svgp_het_cols_kernel<T>), dim3((unsigned)((SB + 255) / 256)), dim3(256), 0, st, SB, B, M, P, SYc, (const T*)Text, Y, sY, noise,
                               nrows, ncols, (const D*)vard, mat.Kdiag, a1, want_grad, (const T*)qbuf, Eb, dY, dY_shared, dnoise, mat.dKdiag, scal);
            hipLaunchKernelGGL((svgp_het_finalize_kernel<T>), dim3(1), dim3(64), 0, st, S, M, P, (const D*)scal, (const D*)(sc + 0), (const D*)(sc + 1),
                               (const D*)(sc + 2), (const D*)(sc + 3), scaling, a1, logL, dvdir);
            MXF_LAUNCH_CHECK(h);
            if (!want_grad) { publish_cond(); return 0; }
            // G' = 1/2 a1 Kuf diag(bs) Kuf^T (-> Psi2 slot), Gw = Kuf (a1 beta.e) (-> R slot), Kuf-side reverse mode from dKuf = Text
            if (het_split) {
                rc = mxf_maxabs_internal(h, M, SB, (const float*)Ksc, SB, hsw + 2, st);
                if (!rc) rc = mxf_split_planes_internal(h, M, SB, (const float*)Ksc, SB, hsS, st, MXF_SPLIT_F16X2, hsw + 2);
                if (!rc) rc = mxf_gemm_split_internal(h, st, MXF_SPLIT_F16X2, M, M, SB, {.alpha = 1.0}, {hsS, (int64_t)pl_big, hsw + 2}, {hsK, (int64_t)pl_big, hsw + 1},
                                                      {.C = (float*)Psi2, .ldc = M});
            } else
                rc = mxf_gemm_internal(h, st, {.dtype = dtype, .tb = 1, .M = M, .N = M, .K = SB, .A = {Ksc, SB}, .B = {Kuf, SB}, .C = {Psi2, M}});
            if (rc) return rc;
            if (SB >= 4096 && M <= 65535) hipLaunchKernelGGL((rowdot_kernel<T>), dim3((unsigned)M), dim3(256), 0, st, SB, P, (const T*)Kuf, SB, (const T*)Eb, R);
            else {
                rc = mxf_gemm_internal(h, st, {.dtype = dtype, .M = M, .N = P, .K = SB, .A = {Kuf, SB}, .B = {Eb, P}, .C = {R, P}});
                if (rc) return rc;
            }
            if (use_mat) {
                if (mat.dKuf) MXF_HIP(h, hipMemcpyAsync(mat.dKuf, Text, sizeof(T) * (size_t)M * SB, hipMemcpyDeviceToDevice, st));
            } else {
                rc = mxf_gram_bwd_internal(h, st, {.kind = kind, .dtype = dtype, .N = M, .N2 = SB, .Q = Q, .X = Z, .X2 = X, .ls = ls, .ard = ard, .var = var,
                                                   .dK = Text, .lddk = SB, .dX = dZ, .dX2 = dX, .dls = dls, .dvar = dvar});
                if (rc) return rc;
            }
        } else if (!want_grad) {
            hipLaunchKernelGGL((svgp_mid_kernel<T>), dim3((unsigned)((SB + 255) / 256)), dim3(256), 0, st, SB, B, M, P, (const T*)Kuf, Text, Y, sY,
                               (const T*)wT, noise, a1, 0, (T*)nullptr, (T*)nullptr, 0, scal);
        } else {
            // (dY, dZ, dls, dvar, dX, R were cleared on the second side stream at the start of the call: su_side2)
            // one pass over T: q_n, |e_n|^2, dY, R = Kuf E, and the Kuf-side reverse mode (dX, dZ, dls, dvar) without materialising dKuf
            MXF_T0(h, MXF_T_BWD, st);
            rc = mxf_svgp_bwd_fused_internal(h, st, {.kind = kind, .dtype = dtype, .M = M, .SB = SB, .B = B, .Q = Q, .P = P, .Z = Z, .Xall = X, .ls = ls, .ard = ard,
                                                     .var = var, .Text = Text, .Y = het_stream ? (const T*)hys : Y, .sY = sY, .w = wT,
                                                     .noise = het_stream ? (const T*)hnz : noise, .a1 = a1, .dZ = dZ, .dXall = dX, .dls = dls, .dvar = dvar,
                                                     .dY = dY, .dY_shared = dY_shared, .R = R, .scal = scal, .t_blocked = t_blocked,
                                                     .h0max = use_split ? (const unsigned*)(info2 + 2) : nullptr, .tmax = (const unsigned*)(info2 + 3)});
            if (rc) return rc;
        }
        if (fused) MXF_T1(h, MXF_T_BWD, st);
        MXF_STAGE(h, "reverse pass", st);
        if (het_stream) {
            // sum_n beta_n e_n^2 per sample and the per-row noise gradient: one more pass over the Kfu planes and T''
            if (dnoise) MXF_HIP(h, hipMemsetAsync(dnoise, 0, sizeof(T) * (size_t)B, st));
            hipLaunchKernelGGL(het_stats_kernel, dim3((unsigned)((SB / 16 + 3) / 4)), dim3(256), 0, st, SB, B, M, (const unsigned short*)plKfu, (int64_t)pl_big,
                               (const float*)Text, (const float*)hys, sY, (const float*)noise, (const float*)hrs, (const float*)var, a1, want_grad,
                               (float*)dnoise, hbe2);
            hipLaunchKernelGGL((svgp_finalize_hets_kernel<T>), dim3(1), dim3(64), 0, st, S, B, M, (const D*)scal, (const D*)hbe2, (const D*)hhs, (const D*)noised,
                               (const D*)vard, (const D*)(sc + 0), (const D*)(sc + 1), (const D*)(sc + 2), (const D*)(sc + 3), scaling, a1, logL, dvdir);
            MXF_LAUNCH_CHECK(h);
        } else if (!het) {
            if (whiten) MXF_HIP(h, hipStreamWaitEvent(st, h->ev_join2, 0));      // Phi and the core's Su part (side stream): the value needs tr(C Phi)
            hipLaunchKernelGGL((svgp_finalize_kernel<T>), dim3(1), dim3(64), 0, st, S, B, M, P, (const D*)scal, (const D*)noised, (const D*)vard,
                               (const D*)(sc + 0), (const D*)(sc + 1), (const D*)(sc + 2), (const D*)(sc + 3), scaling, a1, logL, dnz, dvdir,
                               whiten ? (const D*)(sc + 6) : (const D*)nullptr);
            MXF_LAUNCH_CHECK(h);
            if (!want_grad) publish_cond();
        }
        return 0;
    }

    // caller's stream (het: the Su part on the side stream): the rest of the core's reverse mode, dmu, the Kuu Gram's reverse pass and the
    // gradient outputs in one launch; then the join of the side streams
    int finish() {
        int rc;
        if (het) {
            copy_convert(MM, (const T*)Psi2, G, st);
            copy_convert(MP, (const T*)R, Gw, st);
            MXF_HIP(h, hipEventRecord(h->ev_fork, st));
            MXF_HIP(h, hipStreamWaitEvent(sd_, h->ev_fork, 0));
            rc = su_reverse(sd_, false);
            if (rc) return rc;
            MXF_HIP(h, hipEventRecord(h->ev_join, sd_));
            rc = mm(0, 0, 1.0, G, KiSu, 0.0, T1, st);           // T1 = G Ki Su
            if (rc) return rc;
        } else {
            MXF_HIP(h, hipStreamWaitEvent(st, h->ev_join2, 0));      // side stream: Psi2 -> G, T1, dSu / dW / dSdiag (already done)
            hipLaunchKernelGGL((scale_beta_kernel<T>), dim3(gridn(MP)), dim3(256), 0, st, MP, (const T*)R, (const D*)noised, a1, Gw);
        }
        // dKuu = -Ki A_Ki Ki - bP/2 Ki (float32 fused: dKuu0 from the side stream + the rank-2P term below); dmu = Ki Gw - b w
        const bool sym_dkuu = sym_core && !het;
        if (!sym_dkuu) {
            hipLaunchKernelGGL(aki_kernel, dim3(gridn(MM)), dim3(256), 0, st, M, P, (const D*)G, (const D*)T1, (const D*)Gw, (const D*)mud, (const D*)Su, bw, AKi);
            rc = mm(0, 0, 1.0, Ki, AKi, 0.0, T2, st);           // T2 = Ki A_Ki
            if (rc) return rc;
            copy_convert(MM, (const D*)Ki, dKuu, st);
            rc = mm(0, 0, -1.0, T2, Ki, -0.5 * bw * P, dKuu, st);
            if (rc) return rc;
        }
        hipLaunchKernelGGL((gemv_rows_kernel<D>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, M, P, (const D*)Ki, M, (const D*)Gw, (int64_t)P, dmud, -bw, (const D*)wd);
        if (sym_dkuu) hipLaunchKernelGGL(dkuu_rank_kernel, dim3(gridn(MM)), dim3(256), 0, st, M, P, (const D*)dmud, (const D*)wd, bw, dKuu);
        // Kuu-side reverse mode in float64, then added to the streaming-side gradients
        FinishArgs fa;
        fa.cnt = 0;
        auto fin = [&](const D* src, const D* src2, void* dst, int64_t n, int acc) {
            fa.src[fa.cnt] = src; fa.src2[fa.cnt] = src2; fa.dst[fa.cnt] = dst; fa.n[fa.cnt] = n; fa.acc[fa.cnt] = acc; ++fa.cnt;
        };
        if (dmu) fin(dmud, nullptr, dmu, MP, 0);
        if (use_mat) {
            if (mat.dKuu) fin(dKuu, nullptr, mat.dKuu, MM, 0);
        } else {
            if (!fused && (rc = clear_core_grads(st))) return rc;
            // (sym_dkuu: dKuu is formed from the mirrored X, Ki and H0, i.e. symmetric -- the row side of its reverse pass is skipped)
            rc = mxf_gram_bwd_internal(h, st, {.kind = kind, .dtype = MXF_F64, .N = M, .Q = Q, .X = Zd, .ls = lsd, .ard = ard, .var = vard, .dK = dKuu, .lddk = M,
                                               .dX = dZc, .dls = dlsc, .dvar = dvc, .dk_symmetric = sym_dkuu});
            if (rc) return rc;
            if (dZ) fin(dZc, nullptr, dZ, M * Q, 1);
            if (dls) fin(dlsc, nullptr, dls, lsn, 1);
            if (dvar) fin(dvc, sc + 5, dvar, 1, 1);
        }
        if (dnoise && !het && !het_stream) fin(sc + 4, nullptr, dnoise, 1, 0);
        if (fa.cnt) {
            int64_t nmax = 1;
            for (int i = 0; i < fa.cnt; ++i) nmax = fa.n[i] > nmax ? fa.n[i] : nmax;
            hipLaunchKernelGGL((svgp_finish_kernel<T>), dim3(gridn(nmax), (unsigned)fa.cnt), dim3(256), 0, st, fa);
        }
        MXF_STAGE(h, "core reverse", st);
        publish_cond();
        MXF_HIP(h, hipStreamWaitEvent(st, h->ev_join, 0));     // join the Su chain: every output is ordered on the caller's stream
        MXF_T1(h, MXF_T_CALL, st);
        MXF_STAGE(h, "end", st);
        MXF_STAGE_DUMP(h);
        MXF_LAUNCH_CHECK(h);
        return 0;
    }
};

template <typename T>
int svgp_logpdf_typed(SvgpCall<T>& c) {
    if (int rc = c.plan()) return rc;
    if (int rc = c.prologue()) return rc;               // st
    if (int rc = c.kuu_fork()) return rc;               // st
    if (int rc = c.su_side2()) return rc;               // side2
    if (int rc = c.kuf_psi2()) return rc;               // side
    if (int rc = c.kuu_chain()) return rc;              // st, side2
    if (int rc = c.whiten_v_phi()) return rc;           // st, side
    if (int rc = c.ki_w()) return rc;                   // st
    if (int rc = c.su_chain()) return rc;               // side2
    if (int rc = c.h0_planes()) return rc;              // st
    if (int rc = c.value_scalars()) return rc;          // side2
    if (int rc = c.t_product()) return rc;              // st
    if (int rc = c.core_reverse_side()) return rc;      // side
    if (int rc = c.reverse_pass()) return rc;           // st
    if (!c.want_grad) return 0;
    return c.finish();                                  // st, side
}

// ================================================================================================ sparse (Titsias) GP
// SparseGPRegressionLogPdf.compute (sparsegp_regression.py:42-108), one sample, in sufficient statistics:
//   C = Kuu + Psi2/s2 (= L A L^T of the reference, so LA = L^-1 chol(C)), a = C^-1 psi1,
//   logL = -P/2 (log|C| - log|Kuu|) - 1/2 (ups/s2 + BP log 2pi + BP log s2) + tr(psi1^T a)/(2 s2^2) - P B var/(2 s2) + P tr(Ki Psi2)/(2 s2)
// reverse mode (verified against autograd of the oracle to 1e-14):
//   GC = -P/2 C^-1 - a a^T/(2 s2^2);  dPsi2 = GC/s2 + P/(2 s2) Ki;  dKuu = GC + P/2 Ki - P/(2 s2) Ki Psi2 Ki;  dpsi1 = a/s2^2
__global__ void sgp_add_psi2_kernel(int64_t n, double* __restrict__ C, const double* __restrict__ Psi2, const double* __restrict__ noise) {
    const double beta = 1.0 / noise[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) C[i] += beta * Psi2[i];
}
template <typename T>
__global__ void sgp_grads_kernel(int64_t M, int P, const double* __restrict__ Ci, const double* __restrict__ Ki, const double* __restrict__ KPK,
                                 const double* __restrict__ a, const double* __restrict__ noise, double gscale, T* __restrict__ G2,
                                 double* __restrict__ GKuu, T* __restrict__ Gpsi1) {
    const double s2 = noise[0], is2 = 1.0 / s2;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < M * M; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = idx / M, j = idx % M;
        double aa = 0;
        for (int p = 0; p < P; ++p) aa += a[i * P + p] * a[j * P + p];
        const double GC = -0.5 * P * Ci[idx] - 0.5 * is2 * is2 * aa;
        G2[idx] = (T)(gscale * 2.0 * (GC * is2 + 0.5 * P * is2 * Ki[idx]));
        GKuu[idx] = gscale * (GC + 0.5 * P * Ki[idx] - 0.5 * P * is2 * KPK[idx]);
    }
    // Gpsi1 is M x P: a loop of its own, not a branch of the M x M one -- with P > M that left its entries from M M on unwritten (stale
    // scratch in dKuf and dY, i.e. in every gradient but dnoise, under a correct logL)
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < M * P; idx += (int64_t)gridDim.x * blockDim.x)
        Gpsi1[idx] = (T)(gscale * a[idx] * is2 * is2);
}
// sc: [0] sumlogdiag L  [1] sumlogdiag Lc  [2] <psi1,a>  [3] <Ki,Psi2>  [4] <Ci,Psi2>  [5] a^T Psi2 a  [6] ups
template <typename T>
__global__ void sgp_finalize_kernel(int64_t B, int64_t M, int P, const double* __restrict__ sc, const double* __restrict__ noise,
                                    const double* __restrict__ var, double gscale, T* __restrict__ logL, double* __restrict__ dnoise,
                                    double* __restrict__ dvar_direct, const double* __restrict__ a, T* __restrict__ wv) {
    const double s2 = noise[0], is2 = 1.0 / s2, vk = var[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double l = -(double)P * (sc[1] - sc[0]) - 0.5 * (sc[6] * is2 + (double)B * P * (LOG2PI + log(s2))) + 0.5 * sc[2] * is2 * is2
                         - 0.5 * P * (double)B * vk * is2 + 0.5 * P * sc[3] * is2;
        logL[0] = (T)l;
        const double gcpsi = -0.5 * P * sc[4] - 0.5 * is2 * is2 * sc[5];       // <GC, Psi2>
        if (dnoise) dnoise[0] = gscale * (-gcpsi * is2 * is2 + 0.5 * sc[6] * is2 * is2 - 0.5 * (double)B * P * is2 - sc[2] * is2 * is2 * is2
                                          + 0.5 * P * (double)B * vk * is2 * is2 - 0.5 * P * sc[3] * is2 * is2);
        if (dvar_direct) dvar_direct[0] = gscale * (-0.5 * P * (double)B * is2);
    }
    if (wv) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * P; i += (int64_t)gridDim.x * blockDim.x) wv[i] = (T)(a[i] * is2);
}
// dY = dY (= Kuf^T Gpsi1) - gscale * Y / s2
template <typename T>
__global__ void sgp_dy_kernel(int64_t n, const T* __restrict__ Y, const T* __restrict__ noise, double gscale, T* __restrict__ dY) {
    const T c = (T)gscale / noise[0];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dY[i] -= c * Y[i];
}

template <typename T>
int sgp_logpdf_typed(mxf_ctx* h, int kind, int dtype, int64_t B, int64_t M, int Q, int P, const T* X, const T* Y, const T* Z, const T* noise,
                     const T* ls, int ard, const T* var, double jitter, double gscale, T* logL, T* wv, T* Lout, T* LAout, int* info,
                     int want_grad, T* dX, T* dY, T* dZ, T* dnoise, T* dls, T* dvar, hipStream_t st) {
    typedef double D;
    const int64_t MM = M * M, MP = M * P;
    const int lsn = ard ? Q : 1;
    D *Zd, *lsd, *vard, *noised, *Lm, *Linv, *Ki, *Cm, *Lcinv, *Ci, *Psi2d, *KPK, *tmp, *GKuu, *psi1d, *ad, *PA, *sc, *dZc, *dlsc, *dvc;
    int* info2;
    T *Kuf, *Kfu, *Psi2, *psi1, *G2, *Gpsi1;
    size_t need;
    const bool ok = carve_scratch(h, [&](Carver& cv) {
        Zd = cv.take<D>(M * Q); lsd = cv.take<D>(lsn); vard = cv.take<D>(1); noised = cv.take<D>(1);
        Lm = cv.take<D>(MM); Linv = cv.take<D>(MM); Ki = cv.take<D>(MM); Cm = cv.take<D>(MM); Lcinv = cv.take<D>(MM);
        Ci = cv.take<D>(MM); Psi2d = cv.take<D>(MM); KPK = cv.take<D>(MM); tmp = cv.take<D>(MM); GKuu = cv.take<D>(MM);
        psi1d = cv.take<D>(MP); ad = cv.take<D>(MP); PA = cv.take<D>(MP); sc = cv.take<D>(16); info2 = cv.take<int>(4);
        Kuf = cv.take<T>((size_t)M * B); Kfu = cv.take<T>((size_t)M * B); Psi2 = cv.take<T>(MM); psi1 = cv.take<T>(MP);
        G2 = cv.take<T>(MM); Gpsi1 = cv.take<T>(MP);
        dZc = cv.take<D>(M * Q); dlsc = cv.take<D>(lsn); dvc = cv.take<D>(4);
    }, need);
    if (!ok) MXF_FAIL(h, -4, "mxf_sgp_logpdf: cannot allocate %zu bytes of scratch", need);
    copy_convert(M * Q, Z, Zd, st); copy_convert((int64_t)lsn, ls, lsd, st); copy_convert((int64_t)1, var, vard, st); copy_convert((int64_t)1, noise, noised, st);
    MXF_HIP(h, hipMemsetAsync(sc, 0, 16 * sizeof(D), st));
    // (r04) cond_1(Kuu + jitter I) is published exactly as the SVGP call does (mxf_svgp_cond_slot / mxf_svgp_last_cond): the float32 form of
    // this bound feeds a float32 Psi2 into C = Kuu + Psi2 / s2 and K^-1 Psi2 K^-1 -- ELBO 7e-6 at cond 3e4, a non-PD C at 1e6 -- and the
    // module's guard widens the call to float64 above its limit
    if (!mxf_cond_init(h)) MXF_FAIL(h, -4, "mxf_sgp_logpdf: cannot allocate the condition words");
    MXF_HIP(h, hipMemsetAsync(h->cond_dev, 0, 2 * sizeof(double), st));
    // the float64 core products: C (M x n) = op(A) (M x M) Bm (M x n)
    auto mm64 = [&](int ta, const D* A, const D* Bm, int64_t n, D* C) {
        return mxf_gemm_internal(h, st, {.dtype = MXF_F64, .ta = ta, .M = M, .N = n, .K = M, .A = {A, M}, .B = {Bm, n}, .C = {C, n}});
    };
    int rc;
    rc = kuu_f64(h, st, kind, M, Q, Zd, lsd, ard, vard, jitter, Lm);   // Kuu :69-72
    if (rc) return rc;
    hipLaunchKernelGGL(norm1_sym16_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, st, M, (const double*)Lm, M, h->cond_dev);
    MXF_HIP(h, hipMemcpyAsync(Cm, Lm, MM * sizeof(D), hipMemcpyDeviceToDevice, st));
    rc = potrf_f64(h, st, M, Lm, info);                                                              // L :77
    if (rc) return rc;
    rc = trtri_f64(h, st, M, Lm, Linv);
    if (rc) return rc;
    rc = mm64(1, Linv, Linv, M, Ki);
    if (rc) return rc;
    hipLaunchKernelGGL(norm1_sym16_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, st, M, (const double*)Ki, M, h->cond_dev + 1);
    hipLaunchKernelGGL(cond_publish_kernel, dim3(1), dim3(1), 0, st, h->cond_dev, h->cond_host + 2 * h->cond_slot);
    rc = sumlogdiag_f64(h, st, M, Lm, sc + 0);
    if (rc) return rc;
    // streaming statistics: Psi2 = Kuf Kuf^T (TN on the transposed Gram), psi1 = Kuf Y, ups = |Y|^2
    rc = cross_gram(h, st, kind, dtype, Q, M, Z, B, X, ls, ard, var, Kuf);                 // Kuf :74
    if (rc) return rc;
    rc = cross_gram(h, st, kind, dtype, Q, B, X, M, Z, ls, ard, var, Kfu);
    if (rc) return rc;
    rc = mxf_gemm_internal(h, st, {.dtype = dtype, .ta = 1, .M = M, .N = M, .K = B, .A = {Kfu, M}, .B = {Kfu, M}, .C = {Psi2, M}, .lower_only = 1});
    if (rc) return rc;
    hipLaunchKernelGGL((symmetrize_kernel<T>), dim3((unsigned)((M + 31) / 32), (unsigned)((M + 31) / 32), 1), dim3(256), 0, st, Psi2, M, M, MM);
    rc = mxf_gemm_internal(h, st, {.dtype = dtype, .M = M, .N = P, .K = B, .A = {Kuf, B}, .B = {Y, P}, .C = {psi1, P}});
    if (rc) return rc;
    copy_convert(MM, (const T*)Psi2, Psi2d, st); copy_convert(MP, (const T*)psi1, psi1d, st);
    hipLaunchKernelGGL((sumsq_kernel<T>), dim3(1), dim3(256), 0, st, B * P, Y, (int64_t)0, sc + 6);
    // C = Kuu + Psi2/s2, Lc = chol(C), Ci, a = Ci psi1
    hipLaunchKernelGGL(sgp_add_psi2_kernel, dim3(gridn(MM)), dim3(256), 0, st, MM, Cm, (const D*)Psi2d, (const D*)noised);
    rc = potrf_f64(h, st, M, Cm, info2);
    if (rc) return rc;
    rc = sumlogdiag_f64(h, st, M, Cm, sc + 1);
    if (rc) return rc;
    rc = trtri_f64(h, st, M, Cm, Lcinv);
    if (rc) return rc;
    rc = mm64(1, Lcinv, Lcinv, M, Ci);
    if (rc) return rc;
    rc = mm64(0, Ci, psi1d, P, ad);
    if (rc) return rc;
    rc = mm64(0, Psi2d, ad, P, PA);
    if (rc) return rc;
    hipLaunchKernelGGL((dot_kernel<D>), dim3(dotgrid(MP)), dim3(256), 0, st, MP, (const D*)psi1d, (const D*)ad, 1.0, sc + 2);
    hipLaunchKernelGGL((dot_kernel<D>), dim3(dotgrid(MM)), dim3(256), 0, st, MM, (const D*)Ki, (const D*)Psi2d, 1.0, sc + 3);
    hipLaunchKernelGGL((dot_kernel<D>), dim3(dotgrid(MM)), dim3(256), 0, st, MM, (const D*)Ci, (const D*)Psi2d, 1.0, sc + 4);
    hipLaunchKernelGGL((dot_kernel<D>), dim3(dotgrid(MP)), dim3(256), 0, st, MP, (const D*)ad, (const D*)PA, 1.0, sc + 5);
    hipLaunchKernelGGL((sgp_finalize_kernel<T>), dim3(gridn(MP)), dim3(256), 0, st, B, M, P, (const D*)sc, (const D*)noised, (const D*)vard, gscale,
                       logL, want_grad ? sc + 8 : (D*)nullptr, want_grad ? sc + 9 : (D*)nullptr, (const D*)ad, wv);
    // posterior side products (:99-106): L, LA = L^-1 chol(C)
    if (Lout) hipLaunchKernelGGL((convert_kernel<D, T>), dim3(gridn(MM)), dim3(256), 0, st, M, M, (const D*)Lm, M, Lout, M);
    if (LAout) {
        rc = mm64(0, Linv, Cm, M, tmp);
        if (rc) return rc;
        hipLaunchKernelGGL((convert_kernel<D, T>), dim3(gridn(MM)), dim3(256), 0, st, M, M, (const D*)tmp, M, LAout, M);
    }
    MXF_LAUNCH_CHECK(h);
    if (!want_grad) return 0;
    rc = mm64(0, Ki, Psi2d, M, tmp);
    if (rc) return rc;
    rc = mm64(0, tmp, Ki, M, KPK);
    if (rc) return rc;
    hipLaunchKernelGGL((sgp_grads_kernel<T>), dim3(gridn(MM)), dim3(256), 0, st, M, P, (const D*)Ci, (const D*)Ki, (const D*)KPK, (const D*)ad,
                       (const D*)noised, gscale, G2, GKuu, Gpsi1);
    // dKuf = 2 dPsi2 Kuf + dpsi1 Y^T  (into the Kfu buffer), then the Gram reverse mode
    T* dKuf = Kfu;
    rc = mxf_gemm_internal(h, st, {.dtype = dtype, .M = M, .N = B, .K = M, .A = {G2, M}, .B = {Kuf, B}, .C = {dKuf, B}});
    if (rc) return rc;
    rc = mxf_gemm_internal(h, st, {.dtype = dtype, .tb = 1, .M = M, .N = B, .K = P, .A = {Gpsi1, P}, .B = {Y, P}, .beta = 1.0, .C = {dKuf, B}});
    if (rc) return rc;
    if (dZ) MXF_HIP(h, hipMemsetAsync(dZ, 0, sizeof(T) * M * Q, st));
    if (dls) MXF_HIP(h, hipMemsetAsync(dls, 0, sizeof(T) * lsn, st));
    if (dvar) MXF_HIP(h, hipMemsetAsync(dvar, 0, sizeof(T), st));
    if (dX) MXF_HIP(h, hipMemsetAsync(dX, 0, sizeof(T) * B * Q, st));
    rc = mxf_gram_bwd_internal(h, st, {.kind = kind, .dtype = dtype, .N = M, .N2 = B, .Q = Q, .X = Z, .X2 = X, .ls = ls, .ard = ard, .var = var,
                                       .dK = dKuf, .lddk = B, .dX = dZ, .dX2 = dX, .dls = dls, .dvar = dvar});
    if (rc) return rc;
    if (dY) {
        rc = mxf_gemm_internal(h, st, {.dtype = dtype, .ta = 1, .M = B, .N = P, .K = M, .A = {Kuf, B}, .B = {Gpsi1, P}, .C = {dY, P}});     // Kuf^T dpsi1
        if (rc) return rc;
        hipLaunchKernelGGL((sgp_dy_kernel<T>), dim3(gridn(B * P)), dim3(256), 0, st, B * P, Y, noise, gscale, dY);
    }
    MXF_HIP(h, hipMemsetAsync(dZc, 0, sizeof(D) * M * Q, st));
    MXF_HIP(h, hipMemsetAsync(dlsc, 0, sizeof(D) * lsn, st));
    MXF_HIP(h, hipMemsetAsync(dvc, 0, sizeof(D) * 4, st));
    rc = mxf_gram_bwd_internal(h, st, {.kind = kind, .dtype = MXF_F64, .N = M, .Q = Q, .X = Zd, .ls = lsd, .ard = ard, .var = vard, .dK = GKuu, .lddk = M,
                                       .dX = dZc, .dls = dlsc, .dvar = dvc});
    if (rc) return rc;
    if (dZ) hipLaunchKernelGGL((add_convert_kernel<D, T>), dim3(gridn(M * Q)), dim3(256), 0, st, M * Q, (T)1, (const D*)dZc, dZ, 1);
    if (dls) hipLaunchKernelGGL((add_convert_kernel<D, T>), dim3(gridn(lsn)), dim3(64), 0, st, (int64_t)lsn, (T)1, (const D*)dlsc, dls, 1);
    if (dvar) {
        hipLaunchKernelGGL((add_convert_kernel<D, T>), dim3(1), dim3(64), 0, st, (int64_t)1, (T)1, (const D*)dvc, dvar, 1);
        hipLaunchKernelGGL((add_convert_kernel<D, T>), dim3(1), dim3(64), 0, st, (int64_t)1, (T)1, (const D*)(sc + 9), dvar, 1);
    }
    if (dnoise) hipLaunchKernelGGL((add_convert_kernel<D, T>), dim3(1), dim3(64), 0, st, (int64_t)1, (T)1, (const D*)(sc + 8), dnoise, 0);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

extern "C" int mxf_gp_logpdf(mxf_handle h, int kind, int dtype, int S, int64_t N, int Q, int P,
                             const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y,
                             const void* noise_var, int64_t strideS_noise,
                             const void* lengthscale, int ard, int64_t strideS_ls,
                             const void* variance, int64_t strideS_var, double jitter,
                             void* logL, void* L, void* LinvY, int* info, int want_grad,
                             void* dX, void* dY, void* dnoise, void* dls, void* dvar, void* stream) {
    if (!h) return -1;
    if (S <= 0 || N <= 0 || Q <= 0 || P <= 0) MXF_FAIL(h, -2, "mxf_gp_logpdf: bad shape");
    if (!X || !Y || !noise_var || !lengthscale || !variance || !logL || !L || !LinvY) MXF_FAIL(h, -2, "mxf_gp_logpdf: null argument");
    if (kind > MXF_K_MATERN52) MXF_FAIL(h, -2, "mxf_gp_logpdf: stationary kernels only");
    return by_dtype(h, "mxf_gp_logpdf", dtype, [&](auto t) {
        typedef decltype(t) T;
        return gp_logpdf_typed<T>(h, kind, dtype, S, N, Q, P, (const T*)X, strideS_X, (const T*)Y, strideS_Y, (const T*)noise_var, strideS_noise,
                                  (const T*)lengthscale, ard, strideS_ls, (const T*)variance, strideS_var, jitter, (T*)logL, (T*)L, (T*)LinvY, info,
                                  want_grad, (T*)dX, (T*)dY, (T*)dnoise, (T*)dls, (T*)dvar, (hipStream_t)stream);
    });
}

// the typed call behind every SVGP entry point; svgp_checked: behind those that take coordinates
static int svgp_run(mxf_handle h, const char* fn, const MxfSvgp& d) {
    return by_dtype(h, fn, d.dtype, [&](auto t) {
        SvgpCall<decltype(t)> c(h, d);
        return svgp_logpdf_typed(c);
    });
}
static int svgp_checked(mxf_handle h, const char* fn, const MxfSvgp& d) {
    if (!h) return -1;
    if (d.S <= 0 || d.B <= 0 || d.M <= 0 || d.Q <= 0 || d.P <= 0) MXF_FAIL(h, -2, "%s: bad shape", fn);
    if (!d.X || !d.Y || !d.Z || !d.noise || !d.mu || !d.W || !d.sdiag || !d.ls || !d.var || !d.logL) MXF_FAIL(h, -2, "%s: null argument", fn);
    if (d.kind > MXF_K_MATERN52) MXF_FAIL(h, -2, "%s: stationary kernels only", fn);
    return svgp_run(h, fn, d);
}

extern "C" int mxf_svgp_logpdf(mxf_handle h, int kind, int dtype, int S, int64_t B, int64_t M, int Q, int P,
                               const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y,
                               const void* Z, const void* noise_var, const void* qU_mean, const void* qU_cov_W,
                               const void* qU_cov_diag, const void* lengthscale, int ard, const void* variance,
                               double jitter, double scaling, double gscale,
                               void* logL, int* info, int want_grad,
                               void* dX, void* dY, void* dZ, void* dnoise, void* dmu, void* dW, void* dSdiag,
                               void* dls, void* dvar, void* stream) {
    return svgp_checked(h, "mxf_svgp_logpdf",
                        {.kind = kind, .dtype = dtype, .S = S, .B = B, .M = M, .Q = Q, .P = P, .X = X, .sX = strideS_X, .Y = Y, .sY = strideS_Y, .Z = Z,
                         .noise = noise_var, .mu = qU_mean, .W = qU_cov_W, .sdiag = qU_cov_diag, .ls = lengthscale, .ard = ard, .var = variance,
                         .jitter = jitter, .scaling = scaling, .gscale = gscale, .logL = logL, .info = info, .want_grad = want_grad, .dX = dX, .dY = dY,
                         .dZ = dZ, .dnoise = dnoise, .dmu = dmu, .dW = dW, .dSdiag = dSdiag, .dls = dls, .dvar = dvar, .stream = stream});
}

// Sampled hyper-parameters / inducing inputs / q(u) (runtime_variable.py:96-118: every operand may carry its own sample axis; the
// reference broadcasts them all to S and evaluates S independent bounds).  ONE call: sample s uses slice s of every operand whose sample
// stride is non-zero (stride 0 = shared), its own (M x M) core included; the samples run back to back on the caller's stream with the
// handle's scratch reused.  Every gradient output carries the sample axis (slice s = gradient of gscale * logL[s] with respect to the
// operands sample s used): a caller whose operand was shared sums its slices.
extern "C" int mxf_svgp_logpdf_sampled(mxf_handle h, int kind, int dtype, int S, int64_t B, int64_t M, int Q, int P,
                                       const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y, const void* Z, int64_t strideS_Z,
                                       const void* noise_var, int64_t strideS_noise, const void* qU_mean, int64_t strideS_mu,
                                       const void* qU_cov_W, int64_t strideS_W, const void* qU_cov_diag, int64_t strideS_sd,
                                       const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                                       double jitter, double scaling, double gscale, void* logL, int* info, int want_grad,
                                       void* dX, void* dY, void* dZ, void* dnoise, void* dmu, void* dW, void* dSdiag, void* dls, void* dvar,
                                       void* stream) {
    if (!h) return -1;
    if (S <= 0) MXF_FAIL(h, -2, "mxf_svgp_logpdf_sampled: bad shape");
    if (dtype != MXF_F32 && dtype != MXF_F64) MXF_FAIL(h, -2, "mxf_svgp_logpdf_sampled: bad dtype %d", dtype);
    const int64_t e = (int64_t)mxf_esize(dtype), lsn = ard ? Q : 1;
    // one sample per call (S = 1, sample strides 0): the whole call's descriptor, then per sample a copy with its operands moved to slice s
    const MxfSvgp all = {.kind = kind, .dtype = dtype, .B = B, .M = M, .Q = Q, .P = P, .X = X, .Y = Y, .Z = Z, .noise = noise_var, .mu = qU_mean, .W = qU_cov_W,
                         .sdiag = qU_cov_diag, .ls = lengthscale, .ard = ard, .var = variance, .jitter = jitter, .scaling = scaling, .gscale = gscale,
                         .logL = logL, .info = info, .want_grad = want_grad, .dX = dX, .dY = dY, .dZ = dZ, .dnoise = dnoise, .dmu = dmu, .dW = dW,
                         .dSdiag = dSdiag, .dls = dls, .dvar = dvar, .stream = stream};
    auto in = [&](const void*& p, int64_t off) { if (p) p = (const char*)p + off * e; };
    auto out = [&](void*& p, int64_t off) { if (p) p = (char*)p + off * e; };
    for (int64_t s = 0; s < S; ++s) {
        MxfSvgp d = all;
        in(d.X, s * strideS_X); in(d.Y, s * strideS_Y); in(d.Z, s * strideS_Z); in(d.noise, s * strideS_noise); in(d.mu, s * strideS_mu);
        in(d.W, s * strideS_W); in(d.sdiag, s * strideS_sd); in(d.ls, s * strideS_ls); in(d.var, s * strideS_var);
        out(d.logL, s); if (info) d.info = info + s;
        out(d.dX, s * B * Q); out(d.dY, s * B * P); out(d.dZ, s * M * Q); out(d.dnoise, s); out(d.dmu, s * M * P); out(d.dW, s * M * M);
        out(d.dSdiag, s * M); out(d.dls, s * lsn); out(d.dvar, s);
        if (const int rc = svgp_checked(h, "mxf_svgp_logpdf_sampled", d)) return rc;
    }
    return 0;
}

extern "C" int mxf_svgp_logpdf_het(mxf_handle h, int kind, int dtype, int S, int64_t B, int64_t M, int Q, int P,
                                   const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y,
                                   const void* Z, const void* noise_var, int64_t noise_rows, int noise_cols,
                                   const void* qU_mean, const void* qU_cov_W, const void* qU_cov_diag, const void* lengthscale, int ard,
                                   const void* variance, double jitter, double scaling, double gscale,
                                   void* logL, int* info, int want_grad,
                                   void* dX, void* dY, void* dZ, void* dnoise, void* dmu, void* dW, void* dSdiag,
                                   void* dls, void* dvar, void* stream) {
    return svgp_checked(h, "mxf_svgp_logpdf_het",
                        {.kind = kind, .dtype = dtype, .S = S, .B = B, .M = M, .Q = Q, .P = P, .X = X, .sX = strideS_X, .Y = Y, .sY = strideS_Y, .Z = Z,
                         .noise = noise_var, .nrows = noise_rows, .ncols = noise_cols, .mu = qU_mean, .W = qU_cov_W, .sdiag = qU_cov_diag, .ls = lengthscale, .ard = ard, .var = variance,
                         .jitter = jitter, .scaling = scaling, .gscale = gscale, .logL = logL, .info = info, .want_grad = want_grad, .dX = dX, .dY = dY,
                         .dZ = dZ, .dnoise = dnoise, .dmu = dmu, .dW = dW, .dSdiag = dSdiag, .dls = dls, .dvar = dvar, .stream = stream});
}

extern "C" int mxf_svgp_logpdf_mat(mxf_handle h, int dtype, int S, int64_t B, int64_t M, int P, const void* Kuu, const void* Kuf, const void* Kdiag,
                                   const void* Y, int64_t strideS_Y, const void* noise_var, int64_t noise_rows, int noise_cols, const void* qU_mean,
                                   const void* qU_cov_W, const void* qU_cov_diag, double jitter, double scaling, double gscale, void* logL,
                                   int* info, int want_grad, void* dKuu, void* dKuf, void* dKdiag, void* dY, void* dnoise, void* dmu,
                                   void* dW, void* dSdiag, void* stream) {
    if (!h) return -1;
    if (S <= 0 || B <= 0 || M <= 0 || P <= 0) MXF_FAIL(h, -2, "mxf_svgp_logpdf_mat: bad shape");
    if (S > 1 && strideS_Y != B * P) MXF_FAIL(h, -2, "mxf_svgp_logpdf_mat: S > 1 needs contiguous Y samples (S, B, P)");
    if (!Kuu || !Kuf || !Kdiag || !Y || !noise_var || !qU_mean || !qU_cov_W || !qU_cov_diag || !logL) MXF_FAIL(h, -2, "mxf_svgp_logpdf_mat: null argument");
    return svgp_run(h, "mxf_svgp_logpdf_mat",
                    {.dtype = dtype, .S = S, .B = B, .M = M, .P = P, .Y = Y, .sY = S > 1 ? strideS_Y : 0, .noise = noise_var, .nrows = noise_rows,
                     .ncols = noise_cols, .mu = qU_mean, .W = qU_cov_W, .sdiag = qU_cov_diag, .jitter = jitter, .scaling = scaling, .gscale = gscale,
                     .logL = logL, .info = info, .want_grad = want_grad, .dY = dY, .dnoise = dnoise, .dmu = dmu, .dW = dW, .dSdiag = dSdiag,
                     .stream = stream, .Kuu = Kuu, .Kuf = Kuf, .Kdiag = Kdiag, .dKuu = dKuu, .dKuf = dKuf, .dKdiag = dKdiag});
}

extern "C" int mxf_sgp_logpdf(mxf_handle h, int kind, int dtype, int64_t B, int64_t M, int Q, int P, const void* X, const void* Y,
                              const void* Z, const void* noise_var, const void* lengthscale, int ard, const void* variance,
                              double jitter, double gscale, void* logL, void* wv, void* L, void* LA, int* info, int want_grad,
                              void* dX, void* dY, void* dZ, void* dnoise, void* dls, void* dvar, void* stream) {
    if (!h) return -1;
    if (B <= 0 || M <= 0 || Q <= 0 || P <= 0) MXF_FAIL(h, -2, "mxf_sgp_logpdf: bad shape");
    if (!X || !Y || !Z || !noise_var || !lengthscale || !variance || !logL) MXF_FAIL(h, -2, "mxf_sgp_logpdf: null argument");
    if (kind > MXF_K_MATERN52) MXF_FAIL(h, -2, "mxf_sgp_logpdf: stationary kernels only");
    return by_dtype(h, "mxf_sgp_logpdf", dtype, [&](auto t) {
        typedef decltype(t) T;
        return sgp_logpdf_typed<T>(h, kind, dtype, B, M, Q, P, (const T*)X, (const T*)Y, (const T*)Z, (const T*)noise_var, (const T*)lengthscale, ard,
                                   (const T*)variance, jitter, gscale, (T*)logL, (T*)wv, (T*)L, (T*)LA, info, want_grad, (T*)dX, (T*)dY, (T*)dZ,
                                   (T*)dnoise, (T*)dls, (T*)dvar, (hipStream_t)stream);
    });
}
