// Matrix-free product of a stationary covariance matrix with a block of vectors, and the reverse mode of its bilinear form in the kernel
// parameters, for wide inputs, MXF_KMV_WIDE_MIN_Q <= Q <= MXF_KMV_WIDE_MAX_Q (gfx950): mxf_kmv_wide, mxf_kmv_wide_bwd.  The contract is
// kmv.hip's, the covariance of a pair kmv.h's, the tiling of the distances gram_wide.hip's; the launch shape, the LDS layout and the
// scratch are kmv_wide_plan.h.
//   out[s,n,j] = sum_n2 k(X[s,n,:], X2[s,n2,:]) V[s,n2,j]  (+ diag_add[s] V[s,n,j], square)                         (S, N, J)
//   dls, dvar += the gradient of sum_j w_j A[s,:,j]^T K(X, X2) V[s,:,j] in lengthscale and variance
// Nothing of size N x N2 is stored, in HBM or in LDS: a tile's covariances exist in registers only.
//
// Mapping (wave64, both passes): a workgroup of 256 lanes owns a band of 64 rows and walks the tiles of 64 columns of its share of n2;
// lane (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 pairs of rows 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3 of the tile, whose r^2
// live in 16 registers.  KwStage moves two operands through LDS one chunk of kw_qc() columns at a time: the band's rows and the tile's rows
// of a row-major matrix, staged TRANSPOSED, ps[q][row] and zs[q][column], zero-padded beyond the operands' rows and row length, next to one
// scalar per column of the chunk; a lane reads its 4 rows and its 4 columns as two 16-byte LDS loads for 16 pairs.  The next chunk's
// global loads are issued before the current chunk's arithmetic and land in the other LDS buffer after it: one barrier per chunk.  With
// (X, X2, (c / l_q)^2) it serves the distances, d = x - z first, r2 = sum_q d_q^2 (c / l_q)^2 after -- the difference form only; with
// (A, V, w_j) it serves the cotangent of the reverse mode.
//
// Forward.  Per tile: the global loads of the tile of V (64 x JB, zero-padded) are issued, the sweep over Q rebuilds r2, V lands in LDS,
// cov_from at unit variance gives 16 covariances, each multiplied into the JB accumulators of its row: 4 x JB accumulators per lane.
// JB = 4 for J <= 4, else 16 (float32) / 8 (float64); a larger J takes further passes inside the launch.  The 16 lanes of a DPP row share
// their 4 rows: row_reduce_scatter sums 16 accumulators at a time over them, and lane tx keeps accumulator 16 c + tx of call c in a
// double register (4 JB / 16 of them per lane).  float32: after every tile, so a float32 partial covers the tile's 64 values of n2
// (kmv.hip's rule); float64: once, at the end.  The variance multiplies the finished sums.  n2 is split over grid.y only while the
// bands alone give fewer than KW_TARGET workgroups; the partial sums then meet in zeroed double scratch that mxf_narrow_kernel narrows.
//
// Reverse.  Per tile: the sweep over J forms the cotangent g = sum_j w_j A[n,j] V[n2,j] of the lane's 16 pairs; sweep one over Q rebuilds
// r2; then g f goes to the lane's dvar partial and W = g f'(r2) replaces g (the variance and -2 / l_q wait for the close kernel).  An
// isotropic length-scale is done with sum W r2.  ARD: sweep two walks the chunks again, per coordinate sum W d^2 over the lane's pairs,
// over the DPP row by a reduce-scatter, over the workgroup in LDS doubles (double-buffered like the chunks), and after the chunk's
// barrier one global atomic per coordinate into the zeroed doubles (S, Q).  kw_close_kernel scales and adds them to the caller's buffers.
#include "common.h"
#include "kmv.h"             // coord_scale, cov_from, cov_slope
#include "kmv_wide_plan.h"
#include "shared_grad.h"     // mxf_narrow_kernel

namespace {

constexpr int TILE = KW_TILE, MT = KW_MICRO, LANES = KW_LANES;

template <typename T>
struct KwOps {
    int S; int64_t N, N2; int Q, J, ard, square;
    const T* X; int64_t ss_X;
    const T* Z; int64_t ss_Z;       // the second operand: X2, or X itself for a square product
    const T* ls; int64_t ss_ls;
    const T* var; int64_t ss_var;
    const T* da; int64_t ss_da;     // diag_add, or null
    const T* V; int64_t ss_V;
};

struct KwWeights { double w[KW_WG]; };

// four consecutive elements, 16-byte aligned, from LDS
template <typename T> __device__ __forceinline__ void kw_ld4(const T* p, T* v) {
    if constexpr (sizeof(T) == 4) {
        const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        const f64x2_t t = *reinterpret_cast<const f64x2_t*>(p), u = *reinterpret_cast<const f64x2_t*>(p + 2);
        v[0] = t.x; v[1] = t.y; v[2] = u.x; v[3] = u.y;
    }
}

// Rows [r0, r0 + 64) of P (NP rows) and rows [c0, c0 + 64) of Z (NZ rows), both row-major with rows of L elements, and the L scalars sc,
// through LDS a chunk of QC columns at a time.
template <typename T>
struct KwStage {
    static constexpr int QC = kw_qc(sizeof(T)), LD = kw_ld(sizeof(T)), EP = TILE * QC / LANES;
    const T* P; const T* Z; const T* sc;
    int64_t r0, c0, NP, NZ;
    int L, tid;
    T* ps; T* zs; T* ss;                       // LDS
    T gp[EP], gz[EP], gs;                      // a chunk on its way from global memory to LDS

    __device__ __forceinline__ void load(int q0) {
#pragma unroll
        for (int k = 0; k < EP; ++k) {
            const int i = tid + k * LANES, r = i / QC, q = q0 + i % QC;
            gp[k] = (r0 + r < NP && q < L) ? P[(r0 + r) * L + q] : (T)0;
            gz[k] = (c0 + r < NZ && q < L) ? Z[(c0 + r) * L + q] : (T)0;
        }
        if (tid < QC) gs = q0 + tid < L ? sc[q0 + tid] : (T)0;
    }
    __device__ __forceinline__ void store(int buf) {
#pragma unroll
        for (int k = 0; k < EP; ++k) {
            const int i = tid + k * LANES, r = i / QC, q = i % QC;
            ps[(buf * QC + q) * LD + r] = gp[k];
            zs[(buf * QC + q) * LD + r] = gz[k];
        }
        if (tid < QC) ss[buf * QC + tid] = gs;
    }
    // body(c, buf) on every chunk c, staged in buffer buf; after(c, buf) once the whole workgroup has run body(c, buf).  The sweep ends on a
    // barrier, so the next sweep may overwrite buffer 0 at once.
    template <typename F, typename G>
    __device__ __forceinline__ void sweep(F&& body, G&& after) {
        const int nc = (L + QC - 1) / QC;
        load(0);
        store(0);
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            if (c + 1 < nc) load((c + 1) * QC);
            body(c, c & 1);
            if (c + 1 < nc) store((c + 1) & 1);
            __syncthreads();
            after(c, c & 1);
        }
    }
    // the lane's 4 rows and 4 columns of coordinate q of the chunk in buffer buf
    __device__ __forceinline__ void pair(int buf, int q, int tx, int ty, T* pv, T* zv) const {
        kw_ld4<T>(ps + (buf * QC + q) * LD + ty * MT, pv);
        kw_ld4<T>(zs + (buf * QC + q) * LD + tx * MT, zv);
    }
    // r2[i][j] += sum over the chunk's coordinates of (x_i - z_j)^2 (c / l)^2
    __device__ __forceinline__ void add_r2(int buf, int tx, int ty, T (&r2)[MT][MT]) const {
#pragma unroll 4
        for (int q = 0; q < QC; ++q) {
            T xv[MT], zv[MT];
            pair(buf, q, tx, ty, xv, zv);
            const T s = ss[buf * QC + q];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) { const T d = xv[i] - zv[j]; r2[i][j] = fma(d * d, s, r2[i][j]); }
        }
    }
    // g[i][j] += sum over the chunk's columns of (a_i w) v_j
    __device__ __forceinline__ void add_outer(int buf, int tx, int ty, T (&g)[MT][MT]) const {
#pragma unroll 4
        for (int q = 0; q < QC; ++q) {
            T av[MT], vv[MT];
            pair(buf, q, tx, ty, av, vv);
            const T w = ss[buf * QC + q];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const T aw = av[i] * w;
#pragma unroll
                for (int j = 0; j < MT; ++j) g[i][j] = fma(aw, vv[j], g[i][j]);
            }
        }
    }
};

template <typename T>
__device__ __forceinline__ KwStage<T> kw_stage(char* smem, const KwLds& l, const T* P, int64_t NP, const T* Z, int64_t NZ, const T* sc, int L) {
    KwStage<T> t;
    t.P = P; t.Z = Z; t.sc = sc; t.NP = NP; t.NZ = NZ; t.L = L;
    t.r0 = (int64_t)blockIdx.x * TILE; t.c0 = 0; t.tid = threadIdx.x;
    t.ps = reinterpret_cast<T*>(smem + l.ps); t.zs = reinterpret_cast<T*>(smem + l.zs); t.ss = reinterpret_cast<T*>(smem + l.ss);
    return t;
}

// the n2 of workgroup row blockIdx.y: [c0, c1), ch values (a multiple of TILE)
__device__ __forceinline__ void kw_range(int64_t N2, int64_t ch, int64_t& c0, int64_t& c1) {
    c0 = (int64_t)blockIdx.y * ch;
    c1 = c0 + ch < N2 ? c0 + ch : N2;
}

// m2 (S|1, Q): (c / l_q)^2, the scale of a squared difference; one copy where the samples share the lengthscale
template <typename T, int KIND>
__global__ __launch_bounds__(256) void kw_scale_kernel(KwOps<T> o, int64_t total, T* __restrict__ m2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / o.Q, q = i - s * o.Q;
        const T m = coord_scale<T, KIND>() / o.ls[s * o.ss_ls + (o.ard ? q : 0)];
        m2[i] = m * m;
    }
}

// wd[j0 + k] = w[k], the weights of the bilinear form, KW_WG of them per launch
template <typename T>
__global__ __launch_bounds__(KW_WG) void kw_weights_kernel(KwWeights wt, int j0, int J, T* __restrict__ wd) {
    const int j = j0 + threadIdx.x;
    if (j < J) wd[j] = (T)wt.w[threadIdx.x];
}

__global__ __launch_bounds__(256) void kw_zero_kernel(int64_t total, double* __restrict__ p) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0.0;
}

// out[s][n][j] = variance sum_n2 f(n, n2) V[n2][j] (+ diag_add V[n][j]).  With grid.y = 1 a lane writes its results (out); otherwise it
// adds them to the zeroed doubles acc (S, N, J), narrowed by mxf_narrow_kernel; the diagonal term is workgroup row 0's.
template <typename T, int KIND, int JB>
__global__ __launch_bounds__(LANES) void kmvw_fwd_kernel(KwOps<T> o, const T* __restrict__ m2_all, int64_t ss_m2, int npass, int64_t ch,
                                                         double* __restrict__ acc, T* __restrict__ out) {
    constexpr KwLds L = kw_lds(sizeof(T), JB, false);
    constexpr int VLD = kw_vld(sizeof(T), JB), NR = MT * JB / 16, VP = TILE * JB / LANES;
    constexpr bool PER_TILE = sizeof(T) == 4;      // a float32 partial leaves for its double after every tile
    __shared__ __attribute__((aligned(16))) char smem[L.bytes];
    const int tid = threadIdx.x, lane = tid & 63, tx = tid & 15, ty = tid >> 4;
    const int64_t s = blockIdx.z;
    KwStage<T> st = kw_stage<T>(smem, L, o.X + s * o.ss_X, o.N, o.Z + s * o.ss_Z, o.N2, m2_all + s * ss_m2, o.Q);
    T* vt = reinterpret_cast<T*>(smem + L.vt);
    const T* __restrict__ V = o.V + s * o.ss_V;
    int64_t y0, y1;
    kw_range(o.N2, ch, y0, y1);
    const double variance = (double)o.var[s * o.ss_var];
    const bool diag = o.square && o.da != nullptr && blockIdx.y == 0;
    const double dadd = diag ? (double)o.da[s * o.ss_da] : 0.0;
    for (int pass = 0; pass < npass; ++pass) {
        const int j0 = pass * JB;
        double R[NR];
        T a[MT * JB];                               // a[i JB + jb]: row i of the micro-tile, column j0 + jb of V
#pragma unroll
        for (int c = 0; c < NR; ++c) R[c] = 0;
#pragma unroll
        for (int k = 0; k < MT * JB; ++k) a[k] = 0;
        for (int64_t c0 = y0; c0 < y1; c0 += TILE) {
            st.c0 = c0;
            T gv[VP];
#pragma unroll
            for (int k = 0; k < VP; ++k) {
                const int e = tid + k * LANES, r = e / JB, jb = e % JB;
                gv[k] = (c0 + r < o.N2 && j0 + jb < o.J) ? V[(c0 + r) * o.J + j0 + jb] : (T)0;
            }
            T r2[MT][MT] = {};
            st.sweep([&](int, int buf) { st.add_r2(buf, tx, ty, r2); }, [](int, int) {});
            // the tile of V: its last readers passed the sweep's barriers
#pragma unroll
            for (int k = 0; k < VP; ++k) {
                const int e = tid + k * LANES, r = e / JB, jb = e % JB;
                vt[r * VLD + jb] = gv[k];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                T v[JB];
#pragma unroll
                for (int b = 0; b < JB / 4; ++b) kw_ld4<T>(vt + (tx * MT + j) * VLD + 4 * b, v + 4 * b);
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const T f = cov_from<T, KIND>(r2[i][j], (T)1);
#pragma unroll
                    for (int jb = 0; jb < JB; ++jb) a[i * JB + jb] = fma(f, v[jb], a[i * JB + jb]);
                }
            }
            if (PER_TILE || c0 + TILE >= y1) {      // over the 16 lanes that share the rows: lane tx keeps a[16 c + tx]
#pragma unroll
                for (int c = 0; c < NR; ++c) {
                    R[c] += (double)row_reduce_scatter<T, 16>(a + 16 * c, lane);
#pragma unroll
                    for (int k = 0; k < 16; ++k) a[16 * c + k] = 0;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            const int k = 16 * c + tx, jb = k % JB;
            const int64_t n = st.r0 + ty * MT + k / JB, j = j0 + jb;
            if (n < o.N && j < o.J) {
                double r = variance * R[c];
                if (diag) r += dadd * (double)V[n * o.J + j];       // square: N2 = N
                const int64_t at = (s * o.N + n) * o.J + j;
                if (acc) atomic_add(acc + at, r);
                else out[at] = (T)r;
            }
        }
    }
}

// The sums of the reverse mode: dlacc[s][q] += sum_{n,n2} g f' d_q^2 (one value per sample without ARD: sum g f' r2) and
// dvacc[s] += sum_{n,n2} g f, with d_q the scaled difference and g = sum_j w_j A[n][j] V[n2][j].
template <typename T, int KIND>
__global__ __launch_bounds__(LANES) __attribute__((amdgpu_waves_per_eu(KW_BWD_WAVES))) void kmvw_bwd_kernel(KwOps<T> o, const T* __restrict__ m2_all, int64_t ss_m2, const T* __restrict__ wd, int64_t ch,
                                                         const T* __restrict__ A, int64_t ss_A, double* __restrict__ dlacc, double* __restrict__ dvacc) {
    constexpr KwLds L = kw_lds(sizeof(T), 0, true);
    constexpr int QC = kw_qc(sizeof(T));
    __shared__ __attribute__((aligned(16))) char smem[L.bytes];
    const int tid = threadIdx.x, lane = tid & 63, tx = tid & 15, ty = tid >> 4;
    const int64_t s = blockIdx.z;
    KwStage<T> sq = kw_stage<T>(smem, L, o.X + s * o.ss_X, o.N, o.Z + s * o.ss_Z, o.N2, m2_all + s * ss_m2, o.Q);
    KwStage<T> sj = kw_stage<T>(smem, L, A + s * ss_A, o.N, o.V + s * o.ss_V, o.N2, wd, o.J);
    double* dlsacc = reinterpret_cast<double*>(smem + L.dls);      // [2][QC]
    double* red = reinterpret_cast<double*>(smem + L.red);
    if (tid < 2 * QC) dlsacc[tid] = 0.0;                           // (the first sweep's barrier comes before any use)
    const bool ard_ls = dlacc != nullptr && o.ard;
    int64_t y0, y1;
    kw_range(o.N2, ch, y0, y1);
    double DV = 0, DLI = 0;
    for (int64_t c0 = y0; c0 < y1; c0 += TILE) {
        sq.c0 = sj.c0 = c0;
        T w[MT][MT] = {}, r2[MT][MT] = {};
        sj.sweep([&](int, int buf) { sj.add_outer(buf, tx, ty, w); }, [](int, int) {});      // the cotangent g, for now
        sq.sweep([&](int, int buf) { sq.add_r2(buf, tx, ty, r2); }, [](int, int) {});
        // W = g f'(r2) in place of g; pairs beyond N or N2 have g = 0 (A and V are staged zero-padded) and so weigh nothing
        T dv_ = 0, dl_ = 0;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                T f, df;
                cov_slope<T, KIND>(r2[i][j], f, df);
                dv_ = fma(w[i][j], f, dv_);
                w[i][j] *= df;
                dl_ = fma(w[i][j], r2[i][j], dl_);
            }
        DV += (double)dv_;
        DLI += (double)dl_;
        if (ard_ls) {
            sq.sweep(
                [&](int, int buf) {
#pragma unroll 1
                    for (int g4 = 0; g4 < QC / 4; ++g4) {      // four coordinates at a time
                        T gl[4];
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) {
                            const int q = g4 * 4 + qq;
                            T xv[MT], zv[MT], glq = 0;
                            sq.pair(buf, q, tx, ty, xv, zv);
#pragma unroll
                            for (int i = 0; i < MT; ++i)
#pragma unroll
                                for (int j = 0; j < MT; ++j) { const T d = xv[i] - zv[j]; glq = fma(d * d, w[i][j], glq); }
                            gl[qq] = glq * sq.ss[buf * QC + q];
                        }
                        const T v = row_reduce_scatter<T, 4>(gl, lane);      // lane tx < 4 of every DPP row: coordinate 4 g4 + tx of the chunk
                        if (tx < 4) lds_add(dlsacc + buf * QC + g4 * 4 + tx, (double)v);
                    }
                },
                [&](int c, int buf) {
                    if (tid < QC) {
                        const double v = dlsacc[buf * QC + tid];
                        dlsacc[buf * QC + tid] = 0.0;
                        if (c * QC + tid < o.Q) atomic_add(dlacc + s * o.Q + c * QC + tid, v);
                    }
                });
        }
    }
    if (dvacc) {
        const double v = block_sum<double>(DV, red);
        if (tid == 0) atomic_add(dvacc + s, v);
    }
    if (dlacc && !o.ard) {
        const double v = block_sum<double>(DLI, red);
        if (tid == 0) atomic_add(dlacc + s, v);
    }
}

// dls[q] += -2 variance / l_q dlacc[q] (d red / d l_q = -2 d_q^2 / l_q) and dvar += dvacc, over the samples that share them: a thread per
// length-scale, thread 0 the variance as well, no atomics
template <typename T>
__global__ __launch_bounds__(256) void kw_close_kernel(KwOps<T> o, int nl, const double* __restrict__ dlacc, const double* __restrict__ dvacc, T* dls,
                                                       int own_l, T* dvar, int own_v) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (dls && q < nl)
        for (int64_t s = 0; s < o.S; ++s) {
            T* d = dls + (own_l ? s : 0) * nl + q;
            *d = (T)((double)*d - 2.0 * (double)o.var[s * o.ss_var] / (double)o.ls[s * o.ss_ls + q] * dlacc[s * nl + q]);
        }
    if (dvar && q == 0)
        for (int64_t s = 0; s < o.S; ++s) {
            T* d = dvar + (own_v ? s : 0);
            *d = (T)((double)*d + dvacc[s]);
        }
}

struct KwArgs {
    int kind = MXF_K_RBF, dtype = MXF_F32, S = 0; int64_t N = 0, N2 = 0; int Q = 0, J = 0;
    const void *X = nullptr, *X2 = nullptr, *ls = nullptr, *var = nullptr, *da = nullptr, *V = nullptr;
    int64_t ss_X = 0, ss_X2 = 0, ss_ls = 0, ss_var = 0, ss_da = 0, ss_V = 0; int ard = 0;
    void* out = nullptr;                                                                                      // forward
    const void* A = nullptr; int64_t ss_A = 0; const double* w = nullptr; void *dls = nullptr, *dvar = nullptr;      // reverse
};

// carve the plan's scratch, prepare the scales (and the weights), launch
template <typename T, int KIND>
int kw_launch(mxf_handle h, const char* name, const KwArgs& a, const KmvWidePlan& p, bool bwd, hipStream_t st) {
    const KwOps<T> o = {a.S, a.N, p.N2, a.Q, a.J, a.ard, (int)p.square, (const T*)a.X, a.ss_X, (const T*)(p.square ? a.X : a.X2), p.ss_Z,
                        (const T*)a.ls, a.ss_ls, (const T*)a.var, a.ss_var, (const T*)a.da, a.ss_da, (const T*)a.V, a.ss_V};
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    double* zero = p.n_zero ? (double*)(ws + p.at_zero) : nullptr;
    if (zero) hipLaunchKernelGGL(kw_zero_kernel, dim3(grid_for((int64_t)p.n_zero)), dim3(256), 0, st, (int64_t)p.n_zero, zero);
    T* m2 = (T*)(ws + p.at_m2);
    hipLaunchKernelGGL((kw_scale_kernel<T, KIND>), dim3(grid_for(p.n_scale)), dim3(256), 0, st, o, p.n_scale, m2);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    if (!bwd) {
        const int rc = dispatch<KW_JB_SMALL, kw_jb(sizeof(T))>(p.jb, [&](auto jb) {
            hipLaunchKernelGGL((kmvw_fwd_kernel<T, KIND, decltype(jb)::value>), grid, dim3(LANES), 0, st, o, (const T*)m2, p.ss_m2, p.npass, p.ch, zero,
                               (T*)a.out);
            return 0;
        });
        if (rc) return rc;
        if (zero) hipLaunchKernelGGL((mxf_narrow_kernel<T>), dim3(grid_for(p.n_out)), dim3(256), 0, st, p.n_out, (const double*)zero, (T*)a.out);
    } else {
        T* wd = (T*)(ws + p.at_w);
        for (int j0 = 0; j0 < a.J; j0 += KW_WG) {
            KwWeights wt;
            for (int k = 0; k < KW_WG; ++k) wt.w[k] = j0 + k < a.J ? a.w[j0 + k] : 0.0;
            hipLaunchKernelGGL((kw_weights_kernel<T>), dim3(1), dim3(KW_WG), 0, st, wt, j0, a.J, wd);
        }
        double *dlacc = zero, *dvacc = (double*)(ws + p.at_dv);
        hipLaunchKernelGGL((kmvw_bwd_kernel<T, KIND>), grid, dim3(LANES), 0, st, o, (const T*)m2, p.ss_m2, (const T*)wd, p.ch, (const T*)a.A, a.ss_A,
                           a.dls ? dlacc : nullptr, a.dvar ? dvacc : nullptr);
        hipLaunchKernelGGL((kw_close_kernel<T>), dim3(grid_for(p.n_close)), dim3(256), 0, st, o, p.nl, (const double*)dlacc, (const double*)dvacc,
                           (T*)a.dls, (int)(a.ss_ls != 0), (T*)a.dvar, (int)(a.ss_var != 0));
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

int run(mxf_handle h, const char* name, const KwArgs& a, bool bwd, void* stream) {
    if (!h) return -1;
    if (a.dtype != MXF_F32 && a.dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, a.dtype);
    if (a.kind != MXF_K_RBF && a.kind != MXF_K_MATERN12 && a.kind != MXF_K_MATERN32 && a.kind != MXF_K_MATERN52)
        MXF_FAIL(h, -2, "%s: stationary kernels only (kind %d)", name, a.kind);
    const KmvWidePlan p = kmv_wide_plan({.esize = mxf_esize(a.dtype), .bwd = bwd, .S = a.S, .N = a.N, .N2 = a.N2, .Q = a.Q, .J = a.J, .ard = a.ard,
                                         .ss_X = a.ss_X, .ss_X2 = a.ss_X2, .ss_ls = a.ss_ls, .ss_var = a.ss_var, .ss_da = a.ss_da, .ss_V = a.ss_V,
                                         .ss_A = a.ss_A, .has_X = a.X != nullptr, .has_X2 = a.X2 != nullptr, .has_ls = a.ls != nullptr,
                                         .has_var = a.var != nullptr, .has_da = a.da != nullptr, .has_V = a.V != nullptr, .has_out = a.out != nullptr,
                                         .has_A = a.A != nullptr, .has_w = a.w != nullptr, .has_dls = a.dls != nullptr, .has_dvar = a.dvar != nullptr});
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    return dispatch<MXF_F32, MXF_F64>(a.dtype, [&](auto dt) {
        return dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52>(a.kind, [&](auto kind) {
            return kw_launch<mxf_elem_t<decltype(dt)::value>, decltype(kind)::value>(h, name, a, p, bwd, (hipStream_t)stream);
        });
    });
}

}  // namespace

extern "C" int mxf_kmv_wide(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int J, const void* X, int64_t strideS_X,
                            const void* X2, int64_t strideS_X2, const void* lengthscale, int64_t strideS_ls, int ard, const void* variance,
                            int64_t strideS_var, const void* diag_add, int64_t strideS_da, const void* V, int64_t strideS_V, void* out, void* stream) {
    const KwArgs a = {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .J = J, .X = X, .X2 = X2, .ls = lengthscale, .var = variance,
                      .da = X2 ? nullptr : diag_add, .V = V, .ss_X = strideS_X, .ss_X2 = strideS_X2, .ss_ls = strideS_ls, .ss_var = strideS_var,
                      .ss_da = strideS_da, .ss_V = strideS_V, .ard = ard, .out = out};
    return run(h, "mxf_kmv_wide", a, false, stream);
}

extern "C" int mxf_kmv_wide_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int J, const void* X, int64_t strideS_X,
                                const void* X2, int64_t strideS_X2, const void* lengthscale, int64_t strideS_ls, int ard, const void* variance,
                                int64_t strideS_var, const void* A, int64_t strideS_A, const void* V, int64_t strideS_V, const double* w, void* dls_acc,
                                void* dvar_acc, void* stream) {
    const KwArgs a = {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .J = J, .X = X, .X2 = X2, .ls = lengthscale, .var = variance,
                      .V = V, .ss_X = strideS_X, .ss_X2 = strideS_X2, .ss_ls = strideS_ls, .ss_var = strideS_var, .ss_V = strideS_V, .ard = ard,
                      .A = A, .ss_A = strideS_A, .w = w, .dls = dls_acc, .dvar = dvar_acc};
    return run(h, "mxf_kmv_wide_bwd", a, true, stream);
}
