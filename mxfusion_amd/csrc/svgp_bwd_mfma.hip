// SVGP-fused reverse pass on the matrix pipe (gfx950): RBF, float32, P = 1, Q <= 8 (mxf_svgp_bwd_is_mfma); every other case: gram_bwd.hip.
#include "common.h"
#include "internal.h"
#include "gram_bwd_plan.h"

namespace {

// Distances and all cross-lane sums on the matrix pipe.  The difference-form pass spends its 93 VALU instructions per pair on the distance (16), the sums over rows (dZ, R: reduce-scatter across the
// wave + an LDS atomic per row) and over columns (dX, dl: 24 multiply-adds).  With W_mn = 2 g w variance (the per-pair weight) and
// scaled coordinates z_m, x_n every one of them is a skinny matrix product:
//   r2_mn = |z_m|^2 + |x_n|^2 - 2 (X Z^T)_nm                                            (stationary.py:98-107, the reference's own form)
//   dZ_mq = (z_mq S_m - B_mq) / l_q,   [B | S] = W   (M x N) . [X | 1] (N x 9)          (S_m = sum_n W_mn)
//   dX_nq = (x_nq C_n - D_nq) / l_q,   [D | C] = W^T (N x M) . [Z | 1] (M x 9)          (C_n = sum_m W_mn)
//   dl_q  = -(sum_m z_mq^2 S_m - 2 sum_m z_mq B_mq + sum_n x_nq^2 C_n) / l_q
// A wave walks 16 (m) x 16 (n) tiles.  Two v_mfma_f32_16x16x4_f32 (true float32) give the tile of dot products in the accumulator layout
// -- lane = (m = l % 16, columns 4 (l / 16) .. + 3) --, which is at once the layout of the T loads (16 bytes per lane) and the A-operand
// layout of the product that contracts over n: [B | S] of the tile's 16 rows accumulates in 4 registers per lane over ALL the columns
// the wave visits.  The tile of W is transposed through 1 KB of LDS (one ds_write_b128 + four ds_read_b32 per lane) and fed to the
// product that contracts over m: [D | C] of the tile's 16 columns, accumulated over the band's rows and flushed per column tile.
// ~15 VALU instructions per pair; ten MFMAs per 256 pairs.
struct BwdMfmaArgs {
    const float* Zs; const float* Xs;    // coordinates / lengthscale, zero-padded to 8 per point (bwd_prescale_kernel)
    const float* Xn;                     // |x_n|^2 of the scaled coordinates
    const float* ls; const float* var; const float* T; const float* U; const float* Y; const float* w;
    const float* noise;
    float* dX; float* dY; double* zacc;  // zacc [M][16]: 0..7 B_mq, 8 S_m, 9 R_m (zeroed by the launcher); float64: ~10^3 workgroups add into it
    double* dls3;                        // [8]: sum_n x_nq^2 C_n
    float* unread; double* scal;         // (unread: keeps the argument offsets, and with them the pass's machine code, as they were)
    int64_t M, SB, B, sY;
    int Q, ard, CT, dY_shared, tblk;     // tblk: T in 16-column blocks, element (m, n) at ((n / 16) * M + m) * 16 + n % 16
    double a1;
    // F16 accumulation: bit patterns of max |H0| (the T product's A operand), max |w_m|, max |y_n - U_n| -- the bound that scales the weights
    const unsigned* h0max; const unsigned* mx; const unsigned* tmax;     // tmax: max |T| itself when the GEMM reported it (word != 0)
};

constexpr int MF_MT = MXF_MF_MT;             // (gram_bwd_plan.h) row tiles of 16 per band: 4 accumulator registers each (16 tiles spill: the allocator chains each
                                     // accumulating MFMA through a second register quad)
constexpr int MF_RB = MXF_MF_RB;     // rows per band
// sqrt(log2(e) / 2), the extra scale of the pass's coordinates (bwd_prescale_kernel; taken out again where the sums are flushed): exp(-r2 / 2) = 2^-(BWD_CS^2 r2)
constexpr float BWD_CS = 0.84932180028801904272f;
// MFMA chains as ONE inline-asm statement each.  (1) A chain on one accumulator must issue back to back: a single foreign instruction
// between two dependent v_mfma_f32_16x16x4_f32 costs ~43 cycles (MI355X_MICROARCH.md), and the scheduler happily puts v_exp_f32 there.
// (2) In place ("+v"): through the builtin the register allocator chains every accumulation through a second register quad.
// The hazard recogniser does not see these, so every block is hazard-complete by itself: s_nop 4 in front (VALU write -> MFMA read of a
// source register) and s_nop 11 behind (12 wait states >= the 10 an 8-pass MFMA result needs before ANY instruction may touch it -- the
// compiler is free to spill or copy an accumulator right after the block, and did so in the Matern-5/2 instance: wrong dZ until this).
#define MF_DOT2(d, a0, b0, a1, b1)                                                                                      \
    asm volatile("s_nop 4\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, 0\n\tv_mfma_f32_16x16x4_f32 %0, %3, %4, %0\n\ts_nop 11"       \
                 : "=&v"(d) : "v"(a0), "v"(b0), "v"(a1), "v"(b1))
// the ten MFMAs of a pipeline stage in ONE block, the three chains (dots of the next tile, row side of this tile, column side of the
// previous tile) interleaved so that no two neighbours share an accumulator: they issue every 32 cycles (a dependent neighbour waits 40)
#define MF_STAGE(d, xa0_, zb0_, xa1_, zb1_, c1, w0, x0, w1, x1, w2, x2, w3, x3, c2, t0, z0, t1, z1, t2, z2, t3, z3)      \
    asm volatile("s_nop 4\n\t"          /* VALU write -> MFMA read of the same VGPR needs wait states the compiler only inserts for builtins */ \
                 "v_mfma_f32_16x16x4_f32 %0, %3, %4, 0\n\t"                                                             \
                 "v_mfma_f32_16x16x4_f32 %1, %7, %8, %1\n\t"                                                            \
                 "v_mfma_f32_16x16x4_f32 %2, %15, %16, %2\n\t"                                                          \
                 "v_mfma_f32_16x16x4_f32 %0, %5, %6, %0\n\t"                                                            \
                 "v_mfma_f32_16x16x4_f32 %1, %9, %10, %1\n\t"                                                           \
                 "v_mfma_f32_16x16x4_f32 %2, %17, %18, %2\n\t"                                                          \
                 "v_mfma_f32_16x16x4_f32 %1, %11, %12, %1\n\t"                                                          \
                 "v_mfma_f32_16x16x4_f32 %2, %19, %20, %2\n\t"                                                          \
                 "v_mfma_f32_16x16x4_f32 %1, %13, %14, %1\n\t"                                                          \
                 "v_mfma_f32_16x16x4_f32 %2, %21, %22, %2\n\ts_nop 11"                                                    \
                 : "=&v"(d), "+v"(c1), "+v"(c2)                                                                          \
                 : "v"(xa0_), "v"(zb0_), "v"(xa1_), "v"(zb1_), "v"(w0), "v"(x0), "v"(w1), "v"(x1), "v"(w2), "v"(x2), "v"(w3), "v"(x3),   \
                   "v"(t0), "v"(z0), "v"(t1), "v"(z1), "v"(t2), "v"(z2), "v"(t3), "v"(z3))
#define MF_ACC4(c, a0, b0, a1, b1, a2, b2, a3, b3)                                                                      \
    asm volatile("s_nop 4\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, %0\n\tv_mfma_f32_16x16x4_f32 %0, %3, %4, %0\n\t"           \
                 "v_mfma_f32_16x16x4_f32 %0, %5, %6, %0\n\tv_mfma_f32_16x16x4_f32 %0, %7, %8, %0\n\ts_nop 11"               \
                 : "+v"(c) : "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2), "v"(a3), "v"(b3))

// F16 form of a stage (r03): the two ACCUMULATING products contract over the tile's 16 columns / 16 rows, which is exactly the K of one
// v_mfma_f32_16x16x16_f16 -- with the weights and the coordinates split into hi + lo f16 (three products, f32-equivalent as in gemm_split.hip)
// they take 3 + 3 half-length instructions instead of 4 + 4 full-length float32 ones; the dot products stay true float32.
// Chains: d (dots of the next tile), c1 (row side, this tile), c2 (column side, previous tile), interleaved.
#define MF_STAGE16(d, xa0_, zb0_, xa1_, zb1_, c1, wh, wl, xh, xl, c2, th, tl, zh, zl)                                     \
    asm volatile("s_nop 4\n\t"                                                                                            \
                 "v_mfma_f32_16x16x4_f32 %0, %3, %4, 0\n\t"                                                               \
                 "v_mfma_f32_16x16x16_f16 %1, %7, %9, %1\n\t"                                                             \
                 "v_mfma_f32_16x16x16_f16 %2, %11, %13, %2\n\t"                                                           \
                 "v_mfma_f32_16x16x4_f32 %0, %5, %6, %0\n\t"                                                              \
                 "v_mfma_f32_16x16x16_f16 %1, %7, %10, %1\n\t"                                                            \
                 "v_mfma_f32_16x16x16_f16 %2, %11, %14, %2\n\t"                                                           \
                 "v_mfma_f32_16x16x16_f16 %1, %8, %9, %1\n\t"                                                             \
                 "v_mfma_f32_16x16x16_f16 %2, %12, %13, %2\n\ts_nop 11"                                                    \
                 : "=&v"(d), "+v"(c1), "+v"(c2)                                                                            \
                 : "v"(xa0_), "v"(zb0_), "v"(xa1_), "v"(zb1_), "v"(wh), "v"(wl), "v"(xh), "v"(xl), "v"(th), "v"(tl), "v"(zh), "v"(zl))
#define MF_ACC16(c, ah, al, bh, bl)                                                                                       \
    asm volatile("s_nop 4\n\tv_mfma_f32_16x16x16_f16 %0, %1, %3, %0\n\tv_mfma_f32_16x16x16_f16 %0, %1, %4, %0\n\t"        \
                 "v_mfma_f32_16x16x16_f16 %0, %2, %3, %0\n\ts_nop 11"                                                      \
                 : "+v"(c) : "v"(ah), "v"(al), "v"(bh), "v"(bl))

#ifdef MXF_BWD_TRACE
// probe build only (tests/probes/bwd_trace.py): shader-clock stamps of the stages of one wave's row tiles, [column tile it < 8][row tile][stage]
__device__ unsigned bwd_trace_buf[8 * 8 * 8];
extern "C" int mxf_debug_bwd_trace(unsigned* host_out) { return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(bwd_trace_buf), sizeof(bwd_trace_buf)); }
#define BT_STAMP2(mtv, k, dep)                                                                                            \
    do {                                                                                                                  \
        unsigned long long t_;                                                                                            \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep) : "memory");                            \
        if (traced && it < 8 && lane == 0) bwd_trace_buf[(it * 8 + (mtv)) * 8 + (k)] = (unsigned)t_;                      \
    } while (0)
#define BT_STAMP(k, dep)                                                                                                  \
    do {                                                                                                                  \
        unsigned long long t_;                                                                                            \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep) : "memory");                            \
        if (traced && it < 8 && lane == 0) bwd_trace_buf[(it * 8 + mt) * 8 + (k)] = (unsigned)t_;                         \
    } while (0)
#else
#define BT_STAMP(k, dep) do { } while (0)
#define BT_STAMP2(mtv, k, dep) do { } while (0)
#endif
typedef _Float16 bw_f16x4 __attribute__((ext_vector_type(4)));
// x (4 floats) = hi + lo, f16 each (hi = round(x), lo = round(x - hi)): the A / B operand of v_mfma_f32_16x16x16_f16 (k = 4 (lane / 16) + i)
__device__ __forceinline__ void split4(const float (&x)[4], bw_f16x4& hi, bw_f16x4& lo) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 v = {x[0], x[1], x[2], x[3]};
    hi = __builtin_convertvector(v, bw_f16x4);
    lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x4), bw_f16x4);
}

template <bool FULL, bool F16>       // FULL: M % MF_RB == 0 and SB % 64 == 0 (no ragged tiles: no masks); F16: weights accumulated as hi + lo f16
__global__ __launch_bounds__(256, MXF_MF_MT <= 4 ? 3 : 2) void svgp_bwd_mfma_kernel(BwdMfmaArgs a) {
    constexpr int QT = 8;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    // LDS tables of the band (bank-conflict free for the access patterns below: PMC showed half of the LDS cycles in conflicts before)
    __shared__ __attribute__((aligned(16))) float za[F16 ? 1 : MF_RB][16];     // [z (scaled, 8) | 1 | 0 ...]: B operand of the column-side product (row-contiguous reads)
    // F16: the same table as hi / lo f16, four consecutive rows of one entry j in 8 bytes: [row / 4][j][row % 4] -- the B operand of the 16 x 16 x 16 product
    __shared__ __attribute__((aligned(16))) bw_f16x4 zah[F16 ? MF_RB / 4 : 1][16], zal[F16 ? MF_RB / 4 : 1][16];
    __shared__ __attribute__((aligned(16))) float zd[MF_RB][12];     // [z (8) | |z|^2 | w | - | -]: lanes read (row li, word lq): 12-word rows keep 16 rows x 4 words apart
    __shared__ float rowacc[MF_RB][10];
    __shared__ __attribute__((aligned(16))) float wt[4][2][16][20];  // per wave, double-buffered: the W tile, transposed on the way through (20-word rows)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int64_t band0 = (int64_t)blockIdx.y * MF_RB;
    const int Q = a.Q;
    const float* __restrict__ Xs = a.Xs;
    const float* __restrict__ Tm = a.T;
    const float ilj = (li < Q) ? 1.f / a.ls[a.ard ? li : 0] : 0.f;                 // 1 / l of coordinate j = li (column flush)
    const float variance = a.var[0];
    const float c1 = (float)a.a1 / a.noise[0];
    const float kc = -c1 * variance;
    if constexpr (F16) {
        for (int i = tid; i < (MF_RB / 4) * 16; i += 256) {
            const int g4 = i / 16, j = i % 16;
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t r = band0 + 4 * g4 + t;
                v[t] = (r < a.M) ? ((j < QT) ? a.Zs[r * QT + j] : (j == 8 ? 1.f : 0.f)) : 0.f;
            }
            split4(v, zah[g4][j], zal[g4][j]);
        }
    } else {
        for (int i = tid; i < MF_RB * 16; i += 256) {
            const int r = i / 16, j = i % 16;
            za[r][j] = (band0 + r < a.M) ? ((j < QT) ? a.Zs[(band0 + r) * QT + j] : (j == 8 ? 1.f : 0.f)) : 0.f;
        }
    }
    // F16: weights are accumulated as (u k) 2^esc, |u k| 2^esc <= 2^14 from max |T| (reported by the split GEMM; else the bound
    // variance M max|H0|) and |w e| <= max|w| max|e|
    // (k <= 1 up to rounding); -(c1 variance) 2^-esc is applied when the sums are flushed.  f16 subnormals are kept by the matrix pipe
    // (tests/probes/probe_mfma_overlap.hip), so a loose bound costs absolute, not relative, precision: 2^-25 / 2^14 of the bound.
    float escf = 0.f, unsc = 1.f, fl = 1.f;     // fl: what the f16 sums still lack, -(c1 variance) 2^-esc
    if constexpr (F16) {
        const unsigned tb = a.tmax ? a.tmax[0] : 0u;
        const float bnd = (tb ? __builtin_bit_cast(float, tb) : variance * (float)a.M * __builtin_bit_cast(float, a.h0max[0])) +
                          __builtin_bit_cast(float, a.mx[0]) * __builtin_bit_cast(float, a.mx[1]);
        const unsigned bb = __builtin_bit_cast(unsigned, bnd);
        const int ex = (int)((bb >> 23) & 0xff);
        int esc = (ex == 0 || ex == 0xff) ? 0 : 13 - (ex - 127);          // bnd < 2^(ex - 126): bnd 2^esc < 2^14
        esc = esc > 60 ? 60 : (esc < -60 ? -60 : esc);
        escf = (float)esc;
        unsc = __builtin_bit_cast(float, (unsigned)(127 - esc) << 23);    // 2^-esc
        fl = kc * unsc;
    }
    for (int r = tid; r < MF_RB; r += 256) {
        float n2 = 0.f;
        const bool ok = band0 + r < a.M;
#pragma unroll
        for (int q = 0; q < QT; ++q) { const float v = ok ? a.Zs[(band0 + r) * QT + q] : 0.f; zd[r][q] = v; n2 = fmaf(v, v, n2); }
        zd[r][8] = n2;
        zd[r][9] = ok ? a.w[band0 + r] : 0.f;
        zd[r][10] = 0.f; zd[r][11] = 0.f;
    }
    for (int i = tid; i < MF_RB * 10; i += 256) (&rowacc[0][0])[i] = 0.f;
    __syncthreads();

    f32x4 C1[MF_MT];
    float racc[MF_MT];
#pragma unroll
    for (int mt = 0; mt < MF_MT; ++mt) { C1[mt] = f32x4{0.f, 0.f, 0.f, 0.f}; racc[mt] = 0.f; }
    float dl3 = 0.f;
    double qsum = 0.0, esum = 0.0;
    int cur_s = -1;
    auto flush_scal = [&]() {       // wave-uniform call: per-sample sums of q_n (and |e_n|^2 from the first band)
        const double qs = wave_sum(qsum), es = wave_sum(esum);
        if (lane == 0 && cur_s >= 0) { atomic_add(a.scal + 2 * cur_s, qs); if (blockIdx.y == 0) atomic_add(a.scal + 2 * cur_s + 1, es); }
        qsum = 0.0; esum = 0.0;
    };
    float* wtw = &wt[wave][0][0][0];
    constexpr int WTB = 16 * 20;      // words per transpose buffer
    _Float16* const wth = reinterpret_cast<_Float16*>(wtw);      // F16: the same space as two planes of 16 x 20 halves per buffer
    constexpr int WTB16 = 2 * WTB;    // halves per transpose buffer
    // row of T this lane reads in row tile mt: band0 + 16 mt + li (clamped: ragged rows are masked, not skipped -- no branches around loads)
    const int64_t rowl = band0 + li;

    // Loads run AHEAD of their use across the column tiles (r03): the raw column-side values of tile it + 1 are requested at the top of
    // tile it, and the T tiles PD row tiles ahead -- from tile it + 1's first rows while tile it works on its last ones.  (Before, every
    // column tile began with a round of loads that were used at once and with T only two row tiles ahead: PMC had the waves waiting on
    // memory for 42 % of their cycles.)
    constexpr int PD = 4;                                  // T tiles in flight per lane (MF_MT % PD == 0: a tile's slot is its index mod PD)
    static_assert(MF_MT % PD == 0, "slot = row tile % PD needs MF_MT % PD == 0");
    const int64_t tstep = a.tblk ? 256 : 16 * a.SB;       // blocked: a wave's 16 x 16 tile is ONE contiguous KB, the next row tile the next KB
    const int sb = (int)a.SB, bsz = (int)a.B;
    struct Cols { float xa0, xa1; f32x4 xx, uu, yy; float xv[4]; int smp; };
    auto col_nt0 = [&](int it_) -> int { return ((int)blockIdx.x * a.CT + it_) * 64 + wave * 16; };   // (SB < 2^31: the launcher checks)   // the wave's 16 columns (the block's four waves side by side)
    // (the sample of a column tile, nt0 / B, is walked along: a wave's tiles are 64 columns apart, and a 64-bit division per tile is ~100 instructions)
    auto load_cols = [&](int nt0_, int smp_) -> Cols {
        Cols c;
        c.smp = smp_;                                                                // B % 16 == 0: a tile lies inside one sample
        const int n0_ = nt0_ + 4 * lq;
        const int64_t n0c_ = (FULL || n0_ < sb) ? n0_ : sb - 4;
        const int64_t nac_ = (FULL || nt0_ + li < sb) ? nt0_ + li : sb - 1;     // column of the dot product's A operand
        c.xa0 = Xs[nac_ * QT + lq]; c.xa1 = Xs[nac_ * QT + 4 + lq];
        c.xx = *reinterpret_cast<const f32x4*>(a.Xn + n0c_);
        c.uu = *reinterpret_cast<const f32x4*>(a.U + n0c_);
        c.yy = *reinterpret_cast<const f32x4*>(a.Y + (int64_t)c.smp * a.sY + (n0c_ - (int64_t)c.smp * a.B));     // (16-byte aligned: B % 16 == 0, sY = 0 or B)
#pragma unroll
        for (int t = 0; t < 4; ++t) c.xv[t] = Xs[(n0c_ + t) * QT + (li & 7)];
        return c;
    };
    // T rows of this lane: band0 + li + 16 mt; ragged bands clamp to the last row and mask the value instead of branching
    auto tbase = [&](int nt0_, const float*& tl_) -> const float* {
        const int n0_ = nt0_ + 4 * lq;
        const int64_t n0c_ = (FULL || n0_ < sb) ? n0_ : sb - 4;
        tl_ = a.tblk ? Tm + ((int64_t)(nt0_ >> 4) * a.M + a.M - 1) * 16 + 4 * lq : Tm + n0c_ + (a.M - 1) * a.SB;
        return a.tblk ? Tm + ((int64_t)(nt0_ >> 4) * a.M + rowl) * 16 + 4 * lq : Tm + n0c_ + rowl * a.SB;
    };
    auto tget = [&](const float* base_, const float* tl_, int j) -> f32x4 {
        const float* q = base_ + (int64_t)j * tstep;
        if (!FULL) q = q <= tl_ ? q : tl_;
        return *reinterpret_cast<const f32x4*>(q);
    };
    int nt0 = col_nt0(0);
#ifdef MXF_BWD_TRACE
    const bool traced = blockIdx.x == gridDim.x / 2 && blockIdx.y == 3 && wave == 1;
#endif
    if (nt0 < sb) {
    Cols cur;
    const float* tl_c = nullptr;
    const float* tb_c = nullptr;
    f32x4 tq[PD];
    int smp_w = nt0 / bsz, smp_end = (smp_w + 1) * bsz;       // sample of the tile at nt0 and the first column behind it (< 2^31 + B: unsigned compare)
    auto advance_smp = [&](int nt0_) { while ((unsigned)nt0_ >= (unsigned)smp_end) { ++smp_w; smp_end += bsz; } return smp_w; };
    cur = load_cols(nt0, smp_w);
    tb_c = tbase(nt0, tl_c);
#pragma unroll
    for (int j = 0; j < PD; ++j) tq[j] = tget(tb_c, tl_c, j);
    for (int it = 0; it < a.CT; ++it) {
        int nt0n = col_nt0(it + 1);
        const bool has_next = it + 1 < a.CT && nt0n < sb;
        if (!has_next) nt0n = nt0;                        // (no next tile: harmless re-loads of this one)
        const Cols nxt = load_cols(nt0n, has_next ? advance_smp(nt0n) : cur.smp);
        const float* tl_n = tl_c;
        const float* const tb_n = tbase(nt0n, tl_n);
        BT_STAMP2(0, 6, tb_n);
        const int smp = cur.smp;
        if (smp != cur_s) { flush_scal(); cur_s = smp; }
        const int n0 = nt0 + 4 * lq;                                                 // this lane's 4 consecutive columns
        const bool cval = FULL || n0 < sb;                                         // SB % 4 == 0: all four or none
        const float xa0 = cur.xa0, xa1 = cur.xa1;
        const f32x4 xx = cur.xx;
        float e[4], bx[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            bx[t] = cval ? ((li < QT) ? cur.xv[t] : (li == 8 ? 1.f : 0.f)) : 0.f;
            e[t] = cval ? cur.yy[t] - cur.uu[t] : 0.f;
        }
        if (blockIdx.y == 0 && li == 0 && cval) {          // one lane per column, first band only: dY and |e|^2
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                esum += (double)e[t] * (double)e[t];
                if (a.dY) {
                    const float g = -c1 * e[t];
                    const int64_t n = n0 + t;
                    if (a.dY_shared) atomic_add(a.dY + (n - (int64_t)smp * a.B), g); else a.dY[n] = g;
                }
            }
        }
        bw_f16x4 bxh, bxl;
        f32x4 xxs = xx;
        if constexpr (F16) { split4(bx, bxh, bxl); xxs = xx - escf; }       // r2 - esc: k comes out as k 2^esc
        BT_STAMP2(0, 7, xxs[0]);
        float qn = 0.f;
        f32x4 C2 = f32x4{0.f, 0.f, 0.f, 0.f};
        // software pipeline over the row tiles: the dot products of tile mt + 1 are issued BEFORE the arithmetic of tile mt (whose dots were
        // issued one iteration earlier), and the accumulating products of tile mt / the transposed product of tile mt - 1 AFTER it -- so the
        // matrix pipe works on ten MFMAs while the VALU does the next tile, instead of the two taking turns
        // (tile 0's dots through the builtin: their first use follows at once, and only the builtin tells the hazard recogniser)
        f32x4 dotc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa0, zd[li][lq], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        dotc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa1, zd[li][4 + lq], dotc, 0, 0, 0);
        f32x2 zwc = *reinterpret_cast<const f32x2*>(&zd[li][8]);
        float zbn0 = zd[(1 < MF_MT ? 16 : 0) + li][lq], zbn1 = zd[(1 < MF_MT ? 16 : 0) + li][4 + lq];
        f32x2 zwn = *reinterpret_cast<const f32x2*>(&zd[(1 < MF_MT ? 16 : 0) + li][8]);
#pragma unroll
        for (int mt = 0; mt < MF_MT; ++mt) {
            const int rl = mt * 16 + li;
            asm volatile("" ::: "memory");
            BT_STAMP(0, rl);
            f32x4 tv;
            tv = tq[mt % PD];
            BT_STAMP(1, tv[0]);
            if (mt + PD < MF_MT) tq[mt % PD] = tget(tb_c, tl_c, mt + PD);                               // PD row tiles ahead
            else tq[mt % PD] = tget(tb_n, tl_n, mt + PD - MF_MT);                                       // ... into the next column tile
            if (!FULL) { const bool ok = cval && rowl + 16 * mt < a.M; tv = ok ? tv : f32x4{0.f, 0.f, 0.f, 0.f}; }
            f32x4 dotn = dotc;
            const f32x2 zwv = zwc;
            zwc = zwn;
            const float zbc0 = zbn0, zbc1 = zbn1;                   // operands of the NEXT tile's dot products (this stage's MFMA block)
            if (mt + 2 < MF_MT) {                                   // ... and those two tiles ahead, |z|^2 and w
                zbn0 = zd[rl + 32][lq]; zbn1 = zd[rl + 32][4 + lq];
                zwn = *reinterpret_cast<const f32x2*>(&zd[rl + 32][8]);
            }
            // the transposed copy of the PREVIOUS row tile (written one iteration ago)
            float wtr[4], zb2[4];
            bw_f16x4 th, tl, zh, zl;
            if (mt > 0) {
                if constexpr (F16) {        // the product's k index is the row 4 lq + t: four consecutive rows of column li, 8 bytes per plane
                    th = *reinterpret_cast<const bw_f16x4*>(wth + ((mt - 1) & 1) * WTB16 + li * 20 + 4 * lq);
                    tl = *reinterpret_cast<const bw_f16x4*>(wth + ((mt - 1) & 1) * WTB16 + 320 + li * 20 + 4 * lq);
                    zh = zah[(mt - 1) * 4 + lq][li]; zl = zal[(mt - 1) * 4 + lq][li];
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        wtr[t] = wtw[((mt - 1) & 1) * WTB + (lq + 4 * t) * 20 + li];
                        zb2[t] = za[(mt - 1) * 16 + lq + 4 * t][li];
                    }
                }
            }
            const float wm = zwv[1];
            f32x4 W;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float r2 = fmaf(-2.f, dotc[t], zwv[0] + xxs[t]);
                if constexpr (F16) {
                    const float k = __builtin_amdgcn_exp2f(-r2);          // k 2^esc
                    const float u = fmaf(wm, e[t], tv[t]);
                    W[t] = u * k;
                    qn = fmaf(k, tv[t], qn);
                    racc[mt] = fmaf(k, e[t], racc[mt]);
                } else {
                    // k = 2^-r2 is the bare v_exp_f32 (BWD_CS); the weight is W = 2 g w variance = -(c1 variance) (T + w e) k; variance and the sum over pairs of g k are applied once, at the flush
                    const float k = __builtin_amdgcn_exp2f(-r2);          // (r2 may round a few ulps below 0 for coincident points: k = 1 + O(1e-6))
                    const float u = fmaf(wm, e[t], tv[t]);
                    W[t] = kc * (u * k);
                    qn = fmaf(k, tv[t], qn);
                    racc[mt] = fmaf(k, e[t], racc[mt]);
                }
            }
            // this stage's MFMAs: dots of tile mt + 1, [B | S] += W . [X | 1] of tile mt, [D | C] += W^T . [Z | 1] of tile mt - 1
            bw_f16x4 wh16, wl16;
            BT_STAMP(2, W[3]);
            if constexpr (F16) {
                const float wf[4] = {W[0], W[1], W[2], W[3]};
                split4(wf, wh16, wl16);
                BT_STAMP(3, wl16);
                const bw_f16x4 wh = wh16, wl = wl16;
                if (mt > 0 && mt + 1 < MF_MT) {
                    MF_STAGE16(dotn, xa0, zbc0, xa1, zbc1, C1[mt], wh, wl, bxh, bxl, C2, th, tl, zh, zl);
                } else {
                    if (mt + 1 < MF_MT) MF_DOT2(dotn, xa0, zbc0, xa1, zbc1);
                    MF_ACC16(C1[mt], wh, wl, bxh, bxl);
                    if (mt > 0) MF_ACC16(C2, th, tl, zh, zl);
                }
            } else if (mt > 0 && mt + 1 < MF_MT) {
                MF_STAGE(dotn, xa0, zbc0, xa1, zbc1, C1[mt], W[0], bx[0], W[1], bx[1], W[2], bx[2], W[3], bx[3],
                         C2, wtr[0], zb2[0], wtr[1], zb2[1], wtr[2], zb2[2], wtr[3], zb2[3]);
            } else {
                if (mt + 1 < MF_MT) MF_DOT2(dotn, xa0, zbc0, xa1, zbc1);
                MF_ACC4(C1[mt], W[0], bx[0], W[1], bx[1], W[2], bx[2], W[3], bx[3]);
                if (mt > 0) MF_ACC4(C2, wtr[0], zb2[0], wtr[1], zb2[1], wtr[2], zb2[2], wtr[3], zb2[3]);
            }
            BT_STAMP(4, C1[mt][0]);
            // transpose the tile through LDS: written as (m = li, n = 4 lq .. + 3), read (next iteration) as (n = li, m = lq + 4 t)
            __builtin_amdgcn_wave_barrier();
            if constexpr (F16) {
                // the hi / lo planes go through LDS already split, element (m = li, n = 4 lq + t) to [n][m]: eight 2-byte stores (20-half rows:
                // the four column groups of one store land 32 bytes apart, conflict-free), read back as 8 bytes per plane -- the weights are
                // converted once for both products
                _Float16* const wb = wth + (mt & 1) * WTB16;
#pragma unroll
                for (int t = 0; t < 4; ++t) { wb[(4 * lq + t) * 20 + li] = wh16[t]; wb[320 + (4 * lq + t) * 20 + li] = wl16[t]; }
            } else {
                *reinterpret_cast<f32x4*>(wtw + (mt & 1) * WTB + li * 20 + 4 * lq) = W;
            }
            __builtin_amdgcn_wave_barrier();
            dotc = dotn;
            BT_STAMP(5, dotc[0]);
            __builtin_amdgcn_sched_barrier(0);      // keep the unrolled row tiles apart
        }
        {   // the last row tile's transposed product
            float wtr[4], zb2[4];
            if constexpr (F16) {
                const bw_f16x4 th = *reinterpret_cast<const bw_f16x4*>(wth + ((MF_MT - 1) & 1) * WTB16 + li * 20 + 4 * lq);
                const bw_f16x4 tl = *reinterpret_cast<const bw_f16x4*>(wth + ((MF_MT - 1) & 1) * WTB16 + 320 + li * 20 + 4 * lq);
                const bw_f16x4 zh = zah[(MF_MT - 1) * 4 + lq][li], zl = zal[(MF_MT - 1) * 4 + lq][li];
                MF_ACC16(C2, th, tl, zh, zl);
            } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                wtr[t] = wtw[((MF_MT - 1) & 1) * WTB + (lq + 4 * t) * 20 + li];
                zb2[t] = za[(MF_MT - 1) * 16 + lq + 4 * t][li];
            }
            MF_ACC4(C2, wtr[0], zb2[0], wtr[1], zb2[1], wtr[2], zb2[2], wtr[3], zb2[3]);
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");      // inline-asm MFMA result -> VALU read: the hazard recogniser does not see it
        }
        BT_STAMP2(7, 6, C2[0]);
        qsum += (double)(qn * (variance * unsc));
        // column side: C2[r] = [D | C] of column nt0 + 4 lq + r (= this lane's column n0 + r), entry j = li
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float Cn = __shfl(C2[r], (lane & 48) | 8, 64);
            const float pr = bx[r] * Cn;                       // x_nq C_n (q = li; bx is x of column n0 + r at coordinate li)
            if (li < Q) {
                dl3 = fmaf(bx[r], pr, dl3);
                if (a.dX && cval) atomic_add(a.dX + (int64_t)(n0 + r) * Q + li, (pr - C2[r]) * (ilj * (1.f / BWD_CS) * fl));
            }
        }
        BT_STAMP2(7, 7, dl3);
        if (!has_next) break;
        cur = nxt; nt0 = nt0n; tb_c = tb_n; tl_c = tl_n;
    }
    }
    flush_scal();
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    // row side: C1[mt][r] = [B | S] of row band0 + 16 mt + 4 lq + r, column li; the block's four waves are combined in LDS first
#pragma unroll
    for (int mt = 0; mt < MF_MT; ++mt) {
        if (li < 9) {
#pragma unroll
            for (int r = 0; r < 4; ++r) lds_add(&rowacc[mt * 16 + 4 * lq + r][li], C1[mt][r] * fl);
        }
        float rr = racc[mt];                                   // R partials of row 16 mt + li: fold the four column groups
        rr += __shfl_xor(rr, 16, 64);
        rr += __shfl_xor(rr, 32, 64);
        if (lane < 16) lds_add(&rowacc[mt * 16 + li][9], rr * (variance * unsc));
    }
    __syncthreads();
    for (int i = tid; i < MF_RB * 10; i += 256) {
        const int r = i / 10, c = i % 10;
        if (band0 + r < a.M) atomic_add(a.zacc + (band0 + r) * 16 + c, (double)rowacc[r][c]);
    }
    // (dvar = -(sum of S) / variance: by the finishing kernel)
    {   // sum_n x_nq^2 C_n: lane (q = li) holds its share
        float v = (li < Q) ? dl3 * fl : 0.f;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16 && li < Q) atomic_add(a.dls3 + li, (double)v);       // in the kernel's coordinates: the finishing kernel divides by BWD_CS^2
    }
}

// dZ, dls, R from the row-side sums of svgp_bwd_mfma_kernel (one row per thread; float64: z^2 S - 2 z B + x^2 C cancels a digit or two)
// and dvar = -(sum_m S_m) / variance: the pass's weights carry k
__global__ __launch_bounds__(256) void svgp_bwd_finish_kernel(int64_t M, int Q, int ard, const float* __restrict__ Z /* prescaled: Zs */, const float* __restrict__ ls,
                                                              const double* __restrict__ zacc, const double* __restrict__ dls3,
                                                              float* __restrict__ dZ, float* __restrict__ dls, float* __restrict__ R,
                                                              const float* __restrict__ var, float* __restrict__ dvar) {
    __shared__ double red[16];
    constexpr double cs = (double)BWD_CS;
    const int tid = threadIdx.x;
    const int64_t m = (int64_t)blockIdx.x * 256 + tid;
    double g12[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) g12[q] = 0.0;
    double Srow = 0.0;
    if (m < M) {
        const double S = zacc[m * 16 + 8];
        Srow = S;
        if (R) R[m] += (float)zacc[m * 16 + 9];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q < Q) {
                const double ilq = 1.0 / (double)ls[ard ? q : 0];
                const double z = (double)Z[m * 8 + q], Bq = zacc[m * 16 + q];      // the pass's own scaled, centred coordinate (bwd_prescale_kernel's output: 8 per row)
                if (dZ) dZ[m * Q + q] += (float)((z * S - Bq) * ilq / cs);
                g12[q] = z * (z * S - 2.0 * Bq);
            }
        }
    }
    if (dvar) { const double v = block_sum<double>(Srow, red); if (tid == 0) atomic_add(dvar, (float)(-v / (double)var[0])); }
    if (!dls) return;
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        if (q >= Q) break;
        const double v = block_sum<double>(g12[q], red);
        if (tid == 0) {
            const double glq = -(v + (blockIdx.x == 0 ? dls3[q] : 0.0)) / (cs * cs);   // sum over pairs of -W d_q^2 (this block's rows; block 0 adds the column term)
            if (ard) atomic_add(dls + q, (float)(glq / (double)ls[q])); else tot += glq;
        }
    }
    if (tid == 0 && !ard) atomic_add(dls, (float)(tot / (double)ls[0]));
}

// dst[i][0..7] = cs * src[i][0..Q-1] / l_q, zero padded; norms[i] = |dst[i]|^2 (optional).  Rows i = blockIdx.y * B + (row inside the
// sample), blockIdx.y = sample (the coordinates of the M inducing points: one "sample" of B = M rows).
// mx (optional; zeroed by the caller): bit pattern of max_i |aux[i]| (yv == nullptr: the row w) or of max_i |yv[s * sY + i % B] - aux[i]| (the
// residual y_n - U_n) -- the bound behind the f16 accumulation of the matrix-pipe pass.  One atomic per workgroup, and only if it can raise
// the word (non-negative floats order as their bit patterns).
// centre[q] = mean of Z[m][q] over the FIRST 64 inducing inputs (rows the caller appended to pad M -- far-away decoupled points, svgp_regression.py
// _pad_inducing -- come last and must not drag the centre away): the matrix-pipe pass forms r2 = |x|^2 + |z|^2 - 2 x.z in float32, whose absolute error grows with the NORMS of
// the scaled coordinates -- distances are translation invariant, so both operands are centred on the inducing inputs first (r04: inputs at an
// offset of 100 / 1000 units -- years, raw sensor readings -- gave 1e-2 / 98 % gradient errors and 1e-5 / 2e-2 on the bound un-centred)
__global__ __launch_bounds__(256) void bwd_centre_kernel(int64_t M, int Q, const float* __restrict__ Z, float* __restrict__ centre) {
    __shared__ double red[4];
    const int q = blockIdx.x;
    double s = 0.0;
    for (int64_t m = threadIdx.x; m < M; m += 256) s += (double)Z[m * Q + q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) centre[q] = (float)((red[0] + red[1] + red[2] + red[3]) / (double)M);
}

__global__ __launch_bounds__(256) void bwd_prescale_kernel(const float* __restrict__ src, int64_t B, int Q, const float* __restrict__ ls, int ard,
                                                           const float* __restrict__ centre, float* __restrict__ dst, float* __restrict__ norms, float cs,
                                                           const float* __restrict__ aux, const float* __restrict__ yv, int64_t sY,
                                                           unsigned* __restrict__ mx) {
    __shared__ float smax[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = (int64_t)blockIdx.y * B + i;
    if (mx) {
        float m = 0.f;
        if (i < B) m = fabsf(yv ? yv[(int64_t)blockIdx.y * sY + i] - aux[r] : aux[r]);
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
            if (__builtin_bit_cast(unsigned, m) > *(volatile unsigned*)mx) atomicMax(mx, __builtin_bit_cast(unsigned, m));
        }
    }
    if (i >= B) return;
    float v[8], n2 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { v[q] = (q < Q) ? (src[r * Q + q] - centre[q]) / ls[ard ? q : 0] * cs : 0.f; n2 = fmaf(v[q], v[q], n2); }
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<f32x4*>(dst + r * 8) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + r * 8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
    if (norms) norms[r] = n2;
}

}  // namespace

// RBF only (r04): the pass forms r2 = |x|^2 + |z|^2 - 2 x.z in float32 -- absolute error ~1e-7 (|x|^2 + |z|^2).  The RBF weight is
// smooth in r2; the Matern slopes are not (dk/dr2 = -k / 2r for Matern12): with inducing inputs next to data points -- Z = X[:M] is the
// usual initialisation -- its dX / dZ came out 10-20 % off for Matern12 and 1e-3 off for Matern32 / 52 at Q = 3 ... 8, against 1e-6 ... 5e-5 from the
// difference-form pass (tests/probes/bwd_form_accuracy.py).
bool mxf_svgp_bwd_is_mfma(int kind, int dtype, int64_t SB, int64_t B, int Q, int P, const void* Text) {
    return svgp_bwd_mfma_shape(kind == MXF_K_RBF, dtype == MXF_F32, SB, B, Q, P) && ((uintptr_t)Text % 16) == 0;
}

int mxf_svgp_bwd_mfma_internal(mxf_ctx* h, hipStream_t st, const MxfSvgpBwd& d) {
    if (d.kind != MXF_K_RBF) MXF_FAIL(h, -2, "svgp reverse pass: the matrix-pipe form is RBF only (kind %d)", d.kind);
    static const int64_t grid_target = MXF_KNOB("MXF_BWD_MFMA_GRID", 1024);      // (probe build's knob)
    const int64_t M = d.M, SB = d.SB;
    const SvgpBwdMfmaPlan p = svgp_bwd_mfma_plan(M, SB, d.B, grid_target);
    if (p.refusal) MXF_FAIL(h, -3, "svgp reverse pass: %s (SB %lld, B %lld)", p.refusal, (long long)SB, (long long)d.B);
    if (p.total_bytes > h->bwd_acc.bytes) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cap);
        if (cap != hipStreamCaptureStatusNone) MXF_FAIL(h, -4, "svgp reverse pass: scratch must be allocated before a stream capture (run one eager step first)");
        if (!mxf_grow(h, h->bwd_acc, p.total_bytes, p.total_bytes)) MXF_FAIL(h, -4, "svgp reverse pass: cannot allocate %zu bytes", p.total_bytes);
    }
    char* const base = reinterpret_cast<char*>(h->bwd_acc.p);
    MXF_HIP(h, hipMemsetAsync(base, 0, p.zero_bytes, st));
    BwdMfmaArgs a = {};
    float* const centre = reinterpret_cast<float*>(base + p.centre);
    float* const Zs = reinterpret_cast<float*>(base + p.Zs);
    float* const Xs = reinterpret_cast<float*>(base + p.Xs);
    float* const Xn = reinterpret_cast<float*>(base + p.Xn);
    unsigned* const mx = reinterpret_cast<unsigned*>(base + p.mx);
    a.Zs = Zs; a.Xs = Xs; a.Xn = Xn; a.ls = (const float*)d.ls; a.var = (const float*)d.var; a.T = (const float*)d.Text; a.U = a.T + M * SB; a.Y = (const float*)d.Y;
    a.w = (const float*)d.w; a.noise = (const float*)d.noise; a.dX = (float*)d.dXall; a.dY = (float*)d.dY; a.scal = d.scal;
    a.zacc = reinterpret_cast<double*>(base + p.zacc); a.dls3 = reinterpret_cast<double*>(base + p.dls3);
    a.M = M; a.SB = SB; a.B = d.B; a.sY = d.sY; a.Q = d.Q; a.ard = d.ard; a.CT = p.ct; a.dY_shared = d.dY_shared; a.tblk = d.t_blocked; a.a1 = d.a1;
    a.h0max = d.h0max; a.mx = mx; a.tmax = d.tmax;
    const bool f16 = d.h0max != nullptr;      // f16 accumulation: the T product's operand bound must be known (the split GEMM's max |H0| word)
    hipLaunchKernelGGL(bwd_centre_kernel, dim3((unsigned)d.Q), dim3(256), 0, st, M < 64 ? M : (int64_t)64, d.Q, (const float*)d.Z, centre);
    hipLaunchKernelGGL(bwd_prescale_kernel, dim3((unsigned)((M + 255) / 256), 1), dim3(256), 0, st, (const float*)d.Z, M, d.Q, a.ls, d.ard, (const float*)centre, Zs, (float*)nullptr, BWD_CS,
                       a.w, (const float*)nullptr, (int64_t)0, f16 ? mx : (unsigned*)nullptr);
    hipLaunchKernelGGL(bwd_prescale_kernel, dim3((unsigned)((d.B + 255) / 256), (unsigned)(SB / d.B)), dim3(256), 0, st, (const float*)d.Xall, d.B, d.Q, a.ls, d.ard, (const float*)centre, Xs, Xn, BWD_CS,
                       a.U, a.Y, d.sY, f16 ? mx + 1 : (unsigned*)nullptr);
    const dim3 g(p.grid[0], p.grid[1], p.grid[2]);
    if (f16 && p.full) hipLaunchKernelGGL((svgp_bwd_mfma_kernel<true, true>), g, dim3(256), 0, st, a);
    else if (f16) hipLaunchKernelGGL((svgp_bwd_mfma_kernel<false, true>), g, dim3(256), 0, st, a);
    else if (p.full) hipLaunchKernelGGL((svgp_bwd_mfma_kernel<true, false>), g, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((svgp_bwd_mfma_kernel<false, false>), g, dim3(256), 0, st, a);
    hipLaunchKernelGGL(svgp_bwd_finish_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, M, d.Q, d.ard, (const float*)Zs, a.ls, (const double*)a.zacc, (const double*)a.dls3,
                       (float*)d.dZ, (float*)d.dls, (float*)d.R, a.var, (float*)d.dvar);
    MXF_LAUNCH_CHECK(h);
    return 0;
}
