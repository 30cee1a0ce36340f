// Stationary Gram pass and its reverse mode for wide inputs, 16 < Q <= MXF_GW_MAX_Q (gfx950): mxf_gram_wide, mxf_gram_wide_bwd, and the
// route by which mxf_gram_internal / mxf_gram_bwd_internal hand such calls over (mxf_gram_wide_configure).
//
// Every other Gram kernel of the library keeps a point's Q coordinates in registers and stops at Q = 16.  Here the coordinates pass through
// LDS one chunk of QC = gw_qc() of them at a time, so Q is bounded by index width alone.  The launch shape and the LDS layout are
// gram_wide_plan.h.
//
// Mapping (wave64, both passes): a workgroup of 256 lanes owns a tile of 64 rows x 64 columns; lane (ty, tx) = (tid / 16, tid % 16) owns
// the 4 x 4 pairs of rows 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3, whose r^2 live in 16 registers.  A lane writes 4 consecutive
// elements of a row of K (reads them of dK) as 16-byte pieces, the 16 lanes of a DPP row cover 64 consecutive elements of that row.
// A chunk of the tile's raw rows and columns is staged TRANSPOSED, xs[q][row] and zs[q][column], zero-padded beyond N, N2 and Q, next to
// the chunk's (c / l_q)^2 and 1 / l_q: per coordinate a lane reads its 4 rows and its 4 columns as two 16-byte LDS loads for 16 pairs.
// The next chunk's global loads are issued before the current chunk's arithmetic and land in the other LDS buffer after it: one barrier
// per chunk.
// The distance is formed from the raw coordinates, d = x - z first, r2 = sum_q d_q^2 (c / l_q)^2 after (gram2.hip's order): coincident
// points give r2 = 0 exactly, and no product x . z is ever formed -- so this is a register-blocked VALU design; the matrix pipe would need
// the expansion |x|^2 + |z|^2 - 2 x.z, whose cancellation on near pairs misses the project's bars by many orders.
//
// Reverse: sweep one rebuilds r2; the lane forms W = 2 dK var f'(r2) for its 16 pairs (registers) and adds dK f to its dvar partial.
// Sweep two walks the chunks again, four coordinates at a time; per coordinate and pair u = W d, and
//   row side    sum_j u : summed in the lane, then over the 16 lanes of the DPP row that share the rows (row_reduce_scatter, 16 values --
//               4 rows x 4 coordinates -- at a time): complete for the tile, one plain LDS word per (row, q);
//   column side sum_i u : summed in the lane, then over the wave's four DPP rows by a halving exchange on v_permlane16_swap /
//               v_permlane32_swap (8 + 4 swaps: a lane ends with ONE of the four coordinates for its 4 columns, summed over the wave),
//               then over the four waves by LDS atomics;
//   dls         sum u d per coordinate: summed in the lane, over the DPP row by a 4-value reduce-scatter, then in double in LDS.
// After the chunk's barrier the sums leave with one global atomic per value and workgroup, scaled by (c / l_q)^2 beforehand.  The sums'
// LDS words are double-buffered like the chunks, so the flush of chunk c runs next to the arithmetic of chunk c + 1.  dvar is block-reduced
// in double.  Nothing of size N x N2 is stored; dK is read once.
#include "common.h"
#include "internal.h"
#include "kmv.h"          // coord_scale, cov_from, cov_slope
#include "gram_wide_plan.h"

namespace {

constexpr int TILE = MXF_GW_TILE, MT = MXF_GW_MICRO, LANES = MXF_GW_LANES, RS = MXF_GW_RS;

template <typename T>
struct GwArgs {
    const T* X; const T* X2; const T* ls; const T* var; const T* diag;
    T* K; const T* dK;
    T* dX; T* dXc; T* dls; T* dvar;          // dXc: where the column side goes (dX2, or dX on a square Gram)
    int64_t N, N2, ldk, sX, sX2, sXc, sls, svar, sdiag, sK;
    int Q, ard, square, vec;                 // vec: rows of K / dK may be accessed in 16-byte pieces
    T jitter;
};

// four consecutive elements, 16-byte aligned, from LDS or global memory
template <typename T> __device__ __forceinline__ void gw_ld4(const T* p, T (&v)[MT]) {
    if constexpr (sizeof(T) == 4) {
        const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        const f64x2_t t = *reinterpret_cast<const f64x2_t*>(p), u = *reinterpret_cast<const f64x2_t*>(p + 2);
        v[0] = t.x; v[1] = t.y; v[2] = u.x; v[3] = u.y;
    }
}
template <typename T> __device__ __forceinline__ void gw_st4(T* p, const T (&v)[MT]) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<f32x4_t*>(p) = f32x4_t{v[0], v[1], v[2], v[3]};
    } else {
        *reinterpret_cast<f64x2_t*>(p) = f64x2_t{v[0], v[1]};
        *reinterpret_cast<f64x2_t*>(p + 2) = f64x2_t{v[2], v[3]};
    }
}

// a <- (own a | a of the partner), b <- (b of the partner | own b), partner = the lane 16 (32) further in the even | odd 16-lane (32-lane) row
__device__ __forceinline__ void gw_swap16(unsigned& a, unsigned& b) { asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void gw_swap32(unsigned& a, unsigned& b) { asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b)); }
template <int WIDTH> __device__ __forceinline__ void gw_swap(unsigned& a, unsigned& b) { if (WIDTH == 16) gw_swap16(a, b); else gw_swap32(a, b); }
// a + b after the swap: the sum over the two rows of a's value (even row) or of b's value (odd row)
template <int WIDTH> __device__ __forceinline__ float gw_pair_sum(float a, float b) {
    unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
    gw_swap<WIDTH>(ua, ub);
    return __builtin_bit_cast(float, ua) + __builtin_bit_cast(float, ub);
}
template <int WIDTH> __device__ __forceinline__ double gw_pair_sum(double a, double b) {
    const unsigned long long qa = __builtin_bit_cast(unsigned long long, a), qb = __builtin_bit_cast(unsigned long long, b);
    unsigned al = (unsigned)qa, ah = (unsigned)(qa >> 32), bl = (unsigned)qb, bh = (unsigned)(qb >> 32);
    gw_swap<WIDTH>(al, bl);
    gw_swap<WIDTH>(ah, bh);
    return __builtin_bit_cast(double, ((unsigned long long)ah << 32) | al) + __builtin_bit_cast(double, ((unsigned long long)bh << 32) | bl);
}

// What a workgroup knows of its tile, and the staging of its chunks.
template <typename T, int KIND>
struct GwTile {
    static constexpr int QC = gw_qc(sizeof(T)), LD = gw_ld(sizeof(T)), EP = TILE * QC / LANES;
    const T* X; const T* X2; const T* ls;      // of this sample
    int64_t r0, c0, N, N2;
    int Q, ard, tid;
    T* xs; T* zs; T* m2; T* il;                // LDS
    T gx[EP], gz[EP], gm2, gil;                // a chunk on its way from global memory to LDS

    __device__ __forceinline__ void load(int q0) {
#pragma unroll
        for (int k = 0; k < EP; ++k) {
            const int i = tid + k * LANES, r = i / QC, q = q0 + i % QC;
            gx[k] = (r0 + r < N && q < Q) ? X[(r0 + r) * Q + q] : (T)0;
            gz[k] = (c0 + r < N2 && q < Q) ? X2[(c0 + r) * Q + q] : (T)0;
        }
        if (tid < QC) {
            const int q = q0 + tid;
            gil = q < Q ? (T)1 / ls[ard ? q : 0] : (T)0;
            const T m = gil * coord_scale<T, KIND>();
            gm2 = m * m;
        }
    }
    __device__ __forceinline__ void store(int buf) {
#pragma unroll
        for (int k = 0; k < EP; ++k) {
            const int i = tid + k * LANES, r = i / QC, q = i % QC;
            xs[(buf * QC + q) * LD + r] = gx[k];
            zs[(buf * QC + q) * LD + r] = gz[k];
        }
        if (tid < QC) { m2[buf * QC + tid] = gm2; il[buf * QC + tid] = gil; }
    }
    // body(c, buf) on every chunk c, staged in buffer buf; after(c, buf) once the whole workgroup has run body(c, buf)
    template <typename F, typename G>
    __device__ __forceinline__ void sweep(F&& body, G&& after) {
        const int nc = (Q + QC - 1) / QC;
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
    // r2[i][j] += sum over the chunk's coordinates of ((x_i - z_j) c / l)^2
    __device__ __forceinline__ void add_r2(int buf, int tx, int ty, T (&r2)[MT][MT]) const {
#pragma unroll 4
        for (int q = 0; q < QC; ++q) {
            T xv[MT], zv[MT];
            gw_ld4<T>(xs + (buf * QC + q) * LD + ty * MT, xv);
            gw_ld4<T>(zs + (buf * QC + q) * LD + tx * MT, zv);
            const T s = m2[buf * QC + q];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j) { const T d = xv[i] - zv[j]; r2[i][j] = fma(d * d, s, r2[i][j]); }
        }
    }
};

template <typename T, int KIND>
__device__ __forceinline__ GwTile<T, KIND> gw_tile(const GwArgs<T>& a, char* smem, const GwLds& l) {
    GwTile<T, KIND> t;
    const int s = blockIdx.z;
    t.X = a.X + (int64_t)s * a.sX; t.X2 = a.X2 + (int64_t)s * a.sX2; t.ls = a.ls + (int64_t)s * a.sls;
    t.r0 = (int64_t)blockIdx.y * TILE; t.c0 = (int64_t)blockIdx.x * TILE; t.N = a.N; t.N2 = a.N2;
    t.Q = a.Q; t.ard = a.ard; t.tid = threadIdx.x;
    t.xs = reinterpret_cast<T*>(smem + l.xs); t.zs = reinterpret_cast<T*>(smem + l.zs);
    t.m2 = reinterpret_cast<T*>(smem + l.m2); t.il = reinterpret_cast<T*>(smem + l.il);
    return t;
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void gram_wide_kernel(GwArgs<T> a) {
    constexpr GwLds L = gw_lds(sizeof(T), false);
    __shared__ __attribute__((aligned(16))) char smem[L.bytes];
    GwTile<T, KIND> t = gw_tile<T, KIND>(a, smem, L);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, s = blockIdx.z;
    T r2[MT][MT] = {};
    t.sweep([&](int, int buf) { t.add_r2(buf, tx, ty, r2); }, [](int, int) {});
    const T variance = a.var[(int64_t)s * a.svar];
    const T dadd = a.square ? (a.diag ? a.diag[(int64_t)s * a.sdiag] : (T)0) + a.jitter : (T)0;
    T* __restrict__ K = a.K + (int64_t)s * a.sK;
    const int64_t col = t.c0 + tx * MT;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int64_t row = t.r0 + ty * MT + i;
        if (row >= a.N) break;
        T k[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            k[j] = cov_from<T, KIND>(r2[i][j], variance);
            if (a.square && row == col + j) k[j] += dadd;
        }
        if (a.vec && col + MT <= a.N2) gw_st4<T>(K + row * a.ldk + col, k);
        else {
#pragma unroll
            for (int j = 0; j < MT; ++j) if (col + j < a.N2) K[row * a.ldk + col + j] = k[j];
        }
    }
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void gram_wide_bwd_kernel(GwArgs<T> a) {
    constexpr GwLds L = gw_lds(sizeof(T), true);
    constexpr int QC = gw_qc(sizeof(T));
    __shared__ __attribute__((aligned(16))) char smem[L.bytes];
    GwTile<T, KIND> t = gw_tile<T, KIND>(a, smem, L);
    T* racc = reinterpret_cast<T*>(smem + L.racc);                 // [2][QC][RS]
    T* cacc = reinterpret_cast<T*>(smem + L.cacc);                 // [2][QC][RS]
    double* dlsacc = reinterpret_cast<double*>(smem + L.dls);      // [2][QC]
    double* iso = reinterpret_cast<double*>(smem + L.iso);
    double* red = reinterpret_cast<double*>(smem + L.red);
    const int tid = threadIdx.x, lane = tid & 63, tx = tid & 15, ty = tid >> 4, s = blockIdx.z;
    const bool rowside = a.dX != nullptr, colside = a.dXc != nullptr, wantls = a.dls != nullptr;
    for (int i = tid; i < 2 * QC * RS; i += LANES) cacc[i] = (T)0;
    if (tid < 2 * QC) dlsacc[tid] = 0.0;
    if (tid == 0) *iso = 0.0;

    T w[MT][MT] = {};
    t.sweep([&](int, int buf) { t.add_r2(buf, tx, ty, w); }, [](int, int) {});      // r2, for now

    // W = 2 dK var f'(r2) in place of r2; pairs beyond N or N2 read dK = 0 and so weigh nothing below
    const T variance = a.var[(int64_t)s * a.svar];
    const T* __restrict__ dK = a.dK + (int64_t)s * a.sK;
    const int64_t col = t.c0 + tx * MT;
    T gvar = 0;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int64_t row = t.r0 + ty * MT + i;
        T g[MT] = {};
        if (row < a.N) {
            if (a.vec && col + MT <= a.N2) gw_ld4<T>(dK + row * a.ldk + col, g);
            else {
#pragma unroll
                for (int j = 0; j < MT; ++j) if (col + j < a.N2) g[j] = dK[row * a.ldk + col + j];
            }
        }
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            T f, df;
            cov_slope<T, KIND>(w[i][j], f, df);
            gvar = fma(g[j], f, gvar);
            w[i][j] = (T)2 * g[j] * variance * df;
        }
    }

    if (rowside || colside || wantls) {
        T* dXr = rowside ? a.dX + (int64_t)s * a.sX : nullptr;
        T* dXc = colside ? a.dXc + (int64_t)s * a.sXc : nullptr;
        T* dl = wantls ? a.dls + (int64_t)s * a.sls : nullptr;
        t.sweep(
            [&](int, int buf) {
                const T* m2 = t.m2 + buf * QC;
#pragma unroll 1
                for (int g4 = 0; g4 < QC / 4; ++g4) {      // four coordinates at a time: 16 row-side, 16 column-side and 4 length-scale sums in registers
                    T rs[16], cs[16], gl[4];
#pragma unroll
                    for (int v = 0; v < 16; ++v) { rs[v] = 0; cs[v] = 0; }
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int q = g4 * 4 + qq;
                        T xv[MT], zv[MT], glq = 0;
                        gw_ld4<T>(t.xs + (buf * QC + q) * t.LD + ty * MT, xv);
                        gw_ld4<T>(t.zs + (buf * QC + q) * t.LD + tx * MT, zv);
#pragma unroll
                        for (int i = 0; i < MT; ++i)
#pragma unroll
                            for (int j = 0; j < MT; ++j) {
                                const T d = xv[i] - zv[j], u = w[i][j] * d;
                                rs[qq * 4 + i] += u;
                                cs[qq * 4 + j] += u;
                                glq = fma(u, d, glq);
                            }
                        gl[qq] = glq;
                    }
                    if (rowside) {      // lane tx of the DPP row ends with the tile's sum for row 4 ty + tx % 4, coordinate 4 g4 + tx / 4
                        const T v = row_reduce_scatter<T, 16>(rs, lane);
                        const int q = g4 * 4 + (tx >> 2);
                        racc[(buf * QC + q) * RS + ty * MT + (tx & 3)] = v * m2[q];
                    }
                    if (colside) {      // halve twice: the lane keeps ONE of the four coordinates, for its 4 columns, summed over the wave's four DPP rows
#pragma unroll
                        for (int v = 0; v < 8; ++v) cs[v] = gw_pair_sum<16>(cs[v], cs[v + 8]);
#pragma unroll
                        for (int v = 0; v < 4; ++v) cs[v] = gw_pair_sum<32>(cs[v], cs[v + 4]);
                        const int q = g4 * 4 + ((lane >> 5) & 1) + 2 * ((lane >> 4) & 1);
#pragma unroll
                        for (int j = 0; j < MT; ++j) lds_add(cacc + (buf * QC + q) * RS + tx * MT + j, -cs[j] * m2[q]);
                    }
                    if (wantls) {       // dL / dl_q = -sum W d^2 (c / l_q)^2 / l_q
                        const T v = row_reduce_scatter<T, 4>(gl, lane);
                        const int q = g4 * 4 + tx;
                        if (tx < 4) lds_add(dlsacc + buf * QC + q, -(double)v * (double)m2[q] * (double)t.il[buf * QC + q]);
                    }
                }
            },
            [&](int c, int buf) {
                const int q0 = c * QC;
#pragma unroll
                for (int k = 0; k < t.EP; ++k) {
                    const int i = tid + k * LANES, r = i / QC, q = i % QC;
                    const bool qok = q0 + q < a.Q;
                    if (rowside && qok && t.r0 + r < a.N) atomic_add(dXr + (t.r0 + r) * a.Q + q0 + q, racc[(buf * QC + q) * RS + r]);
                    if (colside) {
                        T* cw = cacc + (buf * QC + q) * RS + r;
                        const T v = *cw;
                        *cw = (T)0;
                        if (qok && t.c0 + r < a.N2) atomic_add(dXc + (t.c0 + r) * a.Q + q0 + q, v);
                    }
                }
                if (wantls && tid < QC) {
                    const double v = dlsacc[buf * QC + tid];
                    dlsacc[buf * QC + tid] = 0.0;
                    if (!a.ard) lds_add(iso, v);
                    else if (q0 + tid < a.Q) atomic_add(dl + q0 + tid, (T)v);
                }
            });
        if (wantls && !a.ard) {
            __syncthreads();
            if (tid == 0) atomic_add(dl, (T)*iso);
        }
    }
    if (a.dvar) {
        const double v = block_sum<double>((double)gvar, red);
        if (tid == 0) atomic_add(a.dvar + (int64_t)s * a.svar, (T)v);
    }
}

struct GwCall {
    int kind, dtype, S; int64_t N, N2; int Q;
    const void* X; int64_t sX; const void* X2; int64_t sX2;
    const void* ls; int ard; int64_t sls; const void* var; int64_t svar;
    const void* diag; int64_t sdiag; double jitter;
    void* K; const void* dK; int64_t ldk, sK;
    void* dX; void* dX2; void* dls; void* dvar;
    bool bwd;
};

GramWidePlan gw_plan(const GwCall& d) {
    GramWideRequest r;
    r.kind = d.kind; r.elem_size = mxf_esize(d.dtype); r.bwd = d.bwd; r.S = d.S; r.N = d.N; r.N2 = d.N2; r.Q = d.Q; r.square = d.X2 == nullptr;
    r.has_X = d.X != nullptr; r.has_ls = d.ls != nullptr; r.has_var = d.var != nullptr; r.has_K = d.bwd ? d.dK != nullptr : d.K != nullptr;
    r.sX = d.sX; r.sX2 = d.sX2; r.sls = d.sls; r.svar = d.svar; r.sdiag = d.sdiag; r.ldk = d.ldk; r.sK = d.sK;
    return gram_wide_plan(r);
}

template <typename T, int KIND>
int gw_launch(const GwCall& d, const GramWidePlan& p, hipStream_t st) {
    constexpr int64_t VEC = 16 / sizeof(T);
    GwArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.square = d.X2 == nullptr;
    a.X = (const T*)d.X; a.sX = d.sX; a.X2 = a.square ? a.X : (const T*)d.X2; a.sX2 = a.square ? d.sX : d.sX2;
    a.ls = (const T*)d.ls; a.sls = d.sls; a.var = (const T*)d.var; a.svar = d.svar;
    a.diag = (const T*)d.diag; a.sdiag = d.sdiag; a.jitter = (T)d.jitter;
    a.K = (T*)d.K; a.dK = (const T*)d.dK; a.ldk = d.ldk; a.sK = d.sK;
    a.dX = (T*)d.dX; a.dXc = a.square ? (T*)d.dX : (T*)d.dX2; a.sXc = a.sX2; a.dls = (T*)d.dls; a.dvar = (T*)d.dvar;
    a.N = d.N; a.N2 = a.square ? d.N : d.N2; a.Q = d.Q; a.ard = d.ard;
    a.vec = d.ldk % VEC == 0 && d.sK % VEC == 0 && (uintptr_t)(d.bwd ? d.dK : (const void*)d.K) % 16 == 0;
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    if (d.bwd) hipLaunchKernelGGL((gram_wide_bwd_kernel<T, KIND>), grid, dim3(LANES), 0, st, a);
    else hipLaunchKernelGGL((gram_wide_kernel<T, KIND>), grid, dim3(LANES), 0, st, a);
    return 0;
}

// p: the accepted plan of d
int gw_run(mxf_ctx* h, const GwCall& d, const GramWidePlan& p, hipStream_t st) {
    if (d.bwd && !d.dX && !d.dls && !d.dvar && (d.X2 == nullptr || !d.dX2)) return 0;      // nothing is asked for
    const int rc = dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52>(d.kind, [&](auto kd) {
        return d.dtype == MXF_F32 ? gw_launch<float, decltype(kd)::value>(d, p, st) : gw_launch<double, decltype(kd)::value>(d, p, st);
    });
    if (rc) return rc;
    MXF_LAUNCH_CHECK(h);
    return 0;
}

int gw_call(mxf_ctx* h, const char* name, const GwCall& d, hipStream_t st) {
    if (d.dtype != MXF_F32 && d.dtype != MXF_F64) return mxf_bad_dtype(h, name, d.dtype);
    const GramWidePlan p = gw_plan(d);
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    return gw_run(h, d, p, st);
}

bool gw_switched_on(const mxf_ctx* h, int dtype, int Q) { return Q >= MXF_GW_MIN_Q && (dtype == MXF_F32 || dtype == MXF_F64) && h->gram_wide[dtype == MXF_F64]; }

}  // namespace

// The routes of mxf_gram_internal and mxf_gram_bwd_internal: *taken says whether the call was this file's to run (the handle's switch is on
// and the plan accepts it); if not, nothing has happened -- no launch, no message -- and the caller goes on as it always did.
int mxf_gram_wide_route(mxf_ctx* h, hipStream_t st, const MxfGram& d, bool* taken) {
    *taken = false;
    if (d.mode != MXF_WRITE || !gw_switched_on(h, d.dtype, d.Q)) return 0;
    const GwCall c = {.kind = d.kind, .dtype = d.dtype, .S = d.S, .N = d.N, .N2 = d.N2, .Q = d.Q, .X = d.X, .sX = d.sX, .X2 = d.X2, .sX2 = d.sX2,
                      .ls = d.ls, .ard = d.ard, .sls = d.sls, .var = d.var, .svar = d.svar, .diag = d.X2 ? nullptr : d.diag_add, .sdiag = d.sdiag,
                      .jitter = d.X2 ? 0.0 : d.jitter, .K = d.K.p, .dK = nullptr, .ldk = d.K.ld, .sK = d.K.stride,
                      .dX = nullptr, .dX2 = nullptr, .dls = nullptr, .dvar = nullptr, .bwd = false};
    const GramWidePlan p = gw_plan(c);
    if (p.rc) return 0;
    *taken = true;
    return gw_run(h, c, p, st);
}

int mxf_gram_wide_bwd_route(mxf_ctx* h, hipStream_t st, const MxfGramBwd& d, bool* taken) {
    *taken = false;
    if (!gw_switched_on(h, d.dtype, d.Q)) return 0;
    const GwCall c = {.kind = d.kind, .dtype = d.dtype, .S = d.S, .N = d.N, .N2 = d.N2, .Q = d.Q, .X = d.X, .sX = d.sX, .X2 = d.X2, .sX2 = d.sX2,
                      .ls = d.ls, .ard = d.ard, .sls = d.sls, .var = d.var, .svar = d.svar, .diag = nullptr, .sdiag = 0, .jitter = 0.0,
                      .K = nullptr, .dK = d.dK, .ldk = d.lddk, .sK = d.sdK, .dX = d.dX, .dX2 = d.dX2, .dls = d.dls, .dvar = d.dvar, .bwd = true};
    const GramWidePlan p = gw_plan(c);
    if (p.rc) return 0;
    *taken = true;
    return gw_run(h, c, p, st);
}

extern "C" int mxf_gram_wide_configure(mxf_handle h, int dtype, int on) {
    if (!h) return -1;
    if (dtype != MXF_F32 && dtype != MXF_F64) return mxf_bad_dtype(h, "mxf_gram_wide_configure", dtype);
    h->gram_wide[dtype == MXF_F64] = on != 0;
    return 0;
}

extern "C" int mxf_gram_wide(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q,
                             const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                             const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                             const void* diag_add, int64_t strideS_diag, double jitter, int mode,
                             void* K_out, int64_t ldk, int64_t strideS_K, void* stream) {
    if (!h) return -1;
    if (mode != MXF_WRITE) MXF_FAIL(h, -2, "mxf_gram_wide: MXF_WRITE only (mode %d)", mode);
    return gw_call(h, "mxf_gram_wide",
                   {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .X = X, .sX = strideS_X, .X2 = X2, .sX2 = strideS_X2,
                    .ls = lengthscale, .ard = ard, .sls = strideS_ls, .var = variance, .svar = strideS_var,
                    .diag = X2 ? nullptr : diag_add, .sdiag = strideS_diag, .jitter = X2 ? 0.0 : jitter,
                    .K = K_out, .dK = nullptr, .ldk = ldk, .sK = strideS_K, .dX = nullptr, .dX2 = nullptr, .dls = nullptr, .dvar = nullptr, .bwd = false},
                   (hipStream_t)stream);
}

extern "C" int mxf_gram_wide_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q,
                                 const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                                 const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                                 const void* dK, int64_t lddk, int64_t strideS_dK,
                                 void* dX, void* dX2, void* dls, void* dvar, void* stream) {
    if (!h) return -1;
    return gw_call(h, "mxf_gram_wide_bwd",
                   {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .X = X, .sX = strideS_X, .X2 = X2, .sX2 = strideS_X2,
                    .ls = lengthscale, .ard = ard, .sls = strideS_ls, .var = variance, .svar = strideS_var, .diag = nullptr, .sdiag = 0, .jitter = 0.0,
                    .K = nullptr, .dK = dK, .ldk = lddk, .sK = strideS_dK, .dX = dX, .dX2 = dX2, .dls = dls, .dvar = dvar, .bwd = true},
                   (hipStream_t)stream);
}
