// Blocked Cholesky, triangular solves, triangular inverse and log-det for gfx950, built on the MFMA GEMM.
//
// Replaces MXNet linalg.potrf / trsm / sumlogdiag call sites of the reference
// (gp_regression.py:61-67,172; svgp_regression.py:83-94,151-164; sparsegp_regression.py:77-89).
//
// potrf: two-level blocking.  Outer panels of NBO columns get ONE trailing syrk-style MFMA update
// (K = NBO, lower blocks only) so the trailing matrix is re-read N/NBO times instead of N/64 times;
// inside a panel 64-wide block columns are updated left-looking (MFMA GEMM), their 64x64 diagonal
// block is factored in LDS by one workgroup, and the rows below are solved against it row-per-lane
// (L11 broadcast from LDS, the row held in VGPRs).  Roofline: MFMA bound for the trailing update
// (N^3/3 flops), latency bound on the 64-wide critical path.
#include "common.h"
#include "internal.h"
#include "chol_plan.h"

namespace {

using namespace mxf_chol_tiles;      // NB = 64 (inner block), NBO = 512 (outer panel), TRI_MIN

// 1/sqrt(d) to full precision: hardware v_rsq estimate + Newton steps (cheaper than a correctly-rounded sqrt AND a division)
__device__ __forceinline__ float inv_sqrt(float d) { float r = rsqrtf(d); r = r * (1.5f - 0.5f * d * r * r); return r; }
__device__ __forceinline__ double inv_sqrt(double d) {
    // (the pivots of a positive-definite matrix that is worth factoring are normal numbers: no scaling of the argument; the hardware
    //  estimate is good to ~2^-26, one third-order correction y (1 + e/2 + 3 e^2/8), e = 1 - d y^2, leaves < 1 ulp -- five dependent
    //  operations on the critical path of every column instead of the library routine's special-case handling plus a Newton step)
    const double y = __builtin_amdgcn_rsq(d);
    const double e = fma(-(d * y), y, 1.0);
    return fma(y * e, fma(e, 0.375, 0.5), y);
}

__device__ __forceinline__ float readlane_t(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ double readlane_t(double v, int l) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffull), l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// ---- fused panel step: every workgroup re-factors the 64x64 diagonal block in LDS (rank-4 blocked: 16 barrier pairs instead of
// 64) and then solves its own 128 rows against it; workgroup 0 owns the diagonal block itself.  One launch per 64-wide block column
// instead of two (diag + solve), and no dependent launch gap between them.
template <typename T>
__global__ __launch_bounds__(128) void potrf_panel_kernel(T* __restrict__ A, int64_t lda, int64_t sA, int64_t k0, int nb, int64_t n,
                                                           int* __restrict__ info, int* __restrict__ arrived) {
    __shared__ T a[NB][NB + 1];
    __shared__ T invd[NB];
    __shared__ T t[128][NB + 1];
    const int tid = threadIdx.x, b = blockIdx.y;
    T* Ab = A + (int64_t)b * sA;
    T* D = Ab + k0 * lda + k0;
    {   // all 32 loads of a thread are issued before the first LDS store: one memory round trip instead of one per unrolled batch
        // (timestamps: 11.5 us for this 32 KB block and 19 us for the 64 KB row tile below, of a 64 us panel step, before)
        T va[NB * NB / 128];
#pragma unroll
        for (int it = 0; it < NB * NB / 128; ++it) {
            const int e = tid + it * 128, i = e / NB, c = e % NB;
            T v = (T)0;
            if (i < nb && c < nb) { if (c <= i) v = D[(int64_t)i * lda + c]; }
            else if (i == c) v = (T)1;          // identity padding of a ragged last block
            va[it] = v;
        }
#pragma unroll
        for (int it = 0; it < NB * NB / 128; ++it) { const int e = tid + it * 128; a[e / NB][e % NB] = va[it]; }
    }
    __syncthreads();
    // Every workgroup re-factors the diagonal block from the UNFACTORED values in global memory, and workgroup 0 writes the factor back
    // in place: it may do so only after all the others have taken their copy (they can start arbitrarily late when other kernels hold
    // the CUs).  Arrival counter: one per batch item, zero on entry, reset to zero by workgroup 0.
    if (blockIdx.x != 0 && tid == 0) { __threadfence(); atomicAdd(arrived + b, 1); }
    // 64 x 64 diagonal block, 16 columns at a time: (1) the 16 x 16 sub-block by ONE wave with a row per lane in registers (pivots and
    // columns travel by v_readlane: no LDS round trip, no barrier), (2) the rows below it by substitution (one row per thread, x[16]),
    // (3) the trailing lower triangle by MFMA:  A22 -= X X^T.  (The rank-4 LDS version it replaces spent ~40 us in 32 barriers and
    // dependent LDS round trips.)
    {
        const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
        for (int blk = 0; blk < NB; blk += 16) {
            if (wave == 0) {                                   // (1)
                T r[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) r[c] = a[blk + li][blk + c];       // lanes 16..63 mirror lanes 0..15 (harmless)
                int bad = -1;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    T d = readlane_t(r[j], j);
                    if (!(d > (T)0)) { if (bad < 0) bad = j; d = (T)1; }        // not positive definite (or NaN): record, keep going finite
                    const T inv = inv_sqrt(d);
                    const T l = (li == j) ? d * inv : r[j] * inv;
                    r[j] = l;
                    if (lane == 0) invd[blk + j] = inv;
#pragma unroll
                    for (int c = j + 1; c < 16; ++c) r[c] = fma(-l, readlane_t(l, c), r[c]);
                }
                if (bad >= 0 && lane == 0 && blockIdx.x == 0 && blk + bad < nb && info && info[b] == 0) info[b] = (int)(k0 + blk + bad + 1);
                if (lane < 16) {
#pragma unroll
                    for (int c = 0; c < 16; ++c) a[blk + lane][blk + c] = (c <= lane) ? r[c] : (T)0;
                }
            }
            __syncthreads();
            if (blk + 16 < NB) {
                const int i = blk + 16 + tid;                   // (2) rows below the sub-block: X L_bb^T = A_ib
                if (i < NB) {
                    T x[16];
#pragma unroll
                    for (int c = 0; c < 16; ++c) {
                        T s0 = a[i][blk + c], s1 = (T)0;
#pragma unroll
                        for (int k = 0; k + 1 < c; k += 2) { s0 = fma(-x[k], a[blk + c][blk + k], s0); s1 = fma(-x[k + 1], a[blk + c][blk + k + 1], s1); }
                        if (c & 1) s0 = fma(-x[c - 1], a[blk + c][blk + c - 1], s0);
                        x[c] = (s0 + s1) * invd[blk + c];
                    }
#pragma unroll
                    for (int c = 0; c < 16; ++c) a[i][blk + c] = x[c];
                }
                __syncthreads();
                // (3) trailing update, lower tiles (I0 >= J0) of 16 x 16, dealt to the two waves
                int tix = 0;
                for (int I0 = blk + 16; I0 < NB; I0 += 16)
                    for (int J0 = blk + 16; J0 <= I0; J0 += 16, ++tix) {
                        if ((tix & 1) != wave) continue;
                        T af[4], bf[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) { af[q] = -a[I0 + li][blk + 4 * q + lq]; bf[q] = a[J0 + li][blk + 4 * q + lq]; }
                        if constexpr (sizeof(T) == 8) {
                            typedef double f64x4_ __attribute__((ext_vector_type(4)));
                            f64x4_ cf;
#pragma unroll
                            for (int r = 0; r < 4; ++r) cf[r] = a[I0 + lq + 4 * r][J0 + li];
#pragma unroll
                            for (int q = 0; q < 4; ++q) cf = __builtin_amdgcn_mfma_f64_16x16x4f64(af[q], bf[q], cf, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 4; ++r) a[I0 + lq + 4 * r][J0 + li] = cf[r];
                        } else {
                            typedef float f32x4_ __attribute__((ext_vector_type(4)));
                            f32x4_ cf;
#pragma unroll
                            for (int r = 0; r < 4; ++r) cf[r] = a[I0 + lq * 4 + r][J0 + li];
#pragma unroll
                            for (int q = 0; q < 4; ++q) cf = __builtin_amdgcn_mfma_f32_16x16x4f32(af[q], bf[q], cf, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 4; ++r) a[I0 + lq * 4 + r][J0 + li] = cf[r];
                        }
                    }
                __syncthreads();
            }
        }
    }
    if (blockIdx.x == 0) {
        if (tid == 0) {
            const int others = (int)gridDim.x - 1;
            while (__hip_atomic_load(arrived + b, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < others) __builtin_amdgcn_s_sleep(2);
            __hip_atomic_store(arrived + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        for (int e = tid; e < nb * nb; e += 128) {
            const int i = e / nb, c = e % nb;
            D[(int64_t)i * lda + c] = (c <= i) ? a[i][c] : (T)0;     // MXNet potrf zeroes the strict upper part
        }
        return;
    }
    // rows below: X L11^T = A21, one row per lane
    const int64_t r0 = k0 + nb, nrows = n - r0;
    const int64_t rb = r0 + (int64_t)(blockIdx.x - 1) * 128;
#pragma unroll
    for (int half = 0; half < 2; ++half) {       // two batches of 32 loads per thread, each issued back to back
        T vt[NB / 2];
#pragma unroll
        for (int it = 0; it < NB / 2; ++it) {
            const int e = tid + (half * (NB / 2) + it) * 128, r = e / NB, c = e % NB;
            vt[it] = (rb + r < r0 + nrows && c < nb) ? Ab[(rb + r) * lda + k0 + c] : (T)0;
        }
#pragma unroll
        for (int it = 0; it < NB / 2; ++it) { const int e = tid + (half * (NB / 2) + it) * 128; t[e / NB][e % NB] = vt[it]; }
    }
    __syncthreads();
    // Blocked substitution: 16 columns at a time by plain substitution (one row per lane, x[16] in registers), then the remaining columns of
    // the tile are updated with MFMA:  T[:, J] -= X[:, blk] L11[J, blk]^T.  The un-blocked form (one row per lane, 64 dependent steps,
    // 2016 broadcast LDS reads with x[64] pinning 128 VGPRs) kept only two LDS reads in flight and took ~40 us of the 84 us kernel.
    {
        const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
        for (int blk = 0; blk < NB; blk += 16) {
            T x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                T s0 = t[tid][blk + c], s1 = (T)0;          // two accumulators: halves the dependent-FMA chain
#pragma unroll
                for (int k = 0; k + 1 < c; k += 2) { s0 = fma(-x[k], a[blk + c][blk + k], s0); s1 = fma(-x[k + 1], a[blk + c][blk + k + 1], s1); }
                if (c & 1) s0 = fma(-x[c - 1], a[blk + c][blk + c - 1], s0);
                x[c] = (s0 + s1) * invd[blk + c];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) t[tid][blk + c] = x[c];
            __syncthreads();
            if (blk + 16 < NB) {
                for (int rt = wave * 4; rt < wave * 4 + 4; ++rt) {          // 8 row tiles of 16 rows, 4 per wave
                    const int rr = rt * 16;
                    T af[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) af[q] = -t[rr + li][blk + 4 * q + lq];
                    for (int J0 = blk + 16; J0 < NB; J0 += 16) {
                        if constexpr (sizeof(T) == 8) {
                            typedef double f64x4_ __attribute__((ext_vector_type(4)));
                            f64x4_ cf;
#pragma unroll
                            for (int r = 0; r < 4; ++r) cf[r] = t[rr + lq + 4 * r][J0 + li];
#pragma unroll
                            for (int q = 0; q < 4; ++q) cf = __builtin_amdgcn_mfma_f64_16x16x4f64(af[q], a[J0 + li][blk + 4 * q + lq], cf, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 4; ++r) t[rr + lq + 4 * r][J0 + li] = cf[r];
                        } else {
                            typedef float f32x4_ __attribute__((ext_vector_type(4)));
                            f32x4_ cf;
#pragma unroll
                            for (int r = 0; r < 4; ++r) cf[r] = t[rr + lq * 4 + r][J0 + li];
#pragma unroll
                            for (int q = 0; q < 4; ++q) cf = __builtin_amdgcn_mfma_f32_16x16x4f32(af[q], a[J0 + li][blk + 4 * q + lq], cf, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 4; ++r) t[rr + lq * 4 + r][J0 + li] = cf[r];
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
#pragma unroll 8
    for (int e = tid; e < 128 * NB; e += 128) {
        const int r = e / NB, c = e % NB;
        if (rb + r < r0 + nrows && c < nb) Ab[(rb + r) * lda + k0 + c] = t[r][c];
    }
}

// ---- tile-dataflow Cholesky (float64, n a multiple of 64): one workgroup per 64-row block row -----------------------------------------
// n <= 512 in ONE launch; larger n one launch per 512-column outer panel (below).  The launch-per-panel form above costs 16 x (panel
// kernel ~45 us + left-looking GEMM + two dependent-launch gaps) at n = 1024: 0.86 ms, every one of them on the critical path of the SVGP
// step when few samples are left per GPU.  Here workgroup i owns block row i and walks its tiles j = 0 .. i
// left-looking:
//     C = A[i][j] - sum_{k<j} L[i][k] L[j][k]^T      (ONE k loop of length 64 j over two contiguous row panels, f64 MFMA, software-pipelined)
//     j < i :  L[i][j] = C L[j][j]^-T                 (with the inverses of L[j][j]'s four 16 x 16 diagonal blocks, which its owner publishes)
//     j = i :  L[i][i] = chol(C)                      (16 x 16 sub-blocks as rank-1 MFMA steps in one accumulator)
// and hands tiles on through a progress counter per block row (release store after the tile is in memory; readers acquire): tile (i, j)
// needs progress[j] >= j before its k loop and progress[j] == j + 1 before its solve.  The diagonal tile's update is accumulated
// incrementally (one 64^3 product after every solve), so the critical path per block column is factor -> solve of the next row's tile ->
// one product -> factor: 23 us (DESIGN.md section 4 has the stage table; tests/probes/potrf_trace.py measures it).  Every workgroup
// must be resident at once (<= 256 workgroups); spins are bounded (a lost hand-off reports info = -1 instead of hanging the queue).
#ifdef MXF_POTRF_TRACE
// probe build only (tests/probes/potrf_trace.py): 100 MHz timestamps of the stages of block rows 0 .. 15, [row][column j][stage]
__device__ long long potrf_trace_buf[16 * 17 * 16];
#define PT_STAMP(k) do { if (tid == 0 && i < 16) potrf_trace_buf[(i * 17 + jt) * 16 + (k)] = wall_clock64(); } while (0)
extern "C" int mxf_debug_potrf_trace(long long* host_out) { return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(potrf_trace_buf), sizeof(long long) * 16 * 17 * 16); }
#else
#define PT_STAMP(k) do { } while (0)
#endif
constexpr int PT_SLD = 66;      // LDS row stride of the staged k chunks (as the small GEMM)
typedef double pt_f64x4 __attribute__((ext_vector_type(4)));

// Panel mode (large n): the same kernel factors ONE outer panel -- columns [c0, c0 + 64 npt), rows c0 .. n, one workgroup per block row
// below c0 -- left-looking INSIDE the panel (columns left of c0 were applied by the trailing updates of the earlier panels): block rows
// i < npt end with their diagonal tile, the others only solve.  nbr = block rows, counters: nbr progress words + one completion word.
__global__ __launch_bounds__(256) void potrf_tiles_kernel(double* __restrict__ A, int64_t lda, int64_t sA, int64_t c0, int npt, int* __restrict__ info,
                                                          int* __restrict__ progress_all, double* __restrict__ inv_all, int row0, int nowait) {
    __shared__ double a[NB][NB + 1];          // diagonal factor L[j][j] (or, for j == i, the tile being factored)
    __shared__ double invd[NB];
    __shared__ double minv[4][16][17];       // the arrived diagonal factor's four inverse blocks
    // the tile being solved, and (never at the same time) the k chunks of the two row panels of the left-looking product: 70 KB of LDS in
    // all, so that a 64 KB float64 GEMM workgroup of the look-ahead trailing update still fits on the same CU
    __shared__ double tsm[(2 * 2 * 16 * PT_SLD > NB * (NB + 1)) ? 2 * 2 * 16 * PT_SLD : NB * (NB + 1)];
    double (*t)[NB + 1] = reinterpret_cast<double (*)[NB + 1]>(tsm);
    double (*sm)[2][16 * PT_SLD] = reinterpret_cast<double (*)[2][16 * PT_SLD]>(tsm);
    __shared__ int sflag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    // row0 / nowait: the SECOND launch of a split outer panel -- block rows row0 .. below an already factored diagonal block: every tile
    // they need is final (stream order), nothing is waited for or published
    const int i = row0 + (int)blockIdx.x, b = blockIdx.y, nbk = (int)gridDim.x;
    double* Ab = A + (int64_t)b * sA;
    int* progress = progress_all + (int64_t)b * (nbk + 1);
    double* invs = inv_all + (int64_t)b * npt * 1024;     // [block row][16-column block][row][column] inverses of the diagonal factors' 16 x 16 diagonal blocks
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    bool lost = false;

    // all threads: block until progress[row] >= need; returns the value seen (progress only grows: the caller skips later waits it covers)
    auto wait_for = [&](int row, int need) -> int {
        if (nowait) return 1 << 30;
        if (tid == 0) {
            int spins = 0, v;
            while ((v = __hip_atomic_load(progress + row, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) < need) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (1 << 26)) { v = -1; break; }
            }
            sflag = v;
        }
        __syncthreads();
        const int v = sflag;
        if (v < 0) lost = true;
        __atomic_thread_fence(__ATOMIC_ACQUIRE);         // every wave: drop stale lines before reading the published tiles
        __syncthreads();                                  // (sflag is rewritten by the next wait)
        return v < 0 ? (1 << 30) : v;
    };
    // C (this wave's 32 x 32 quadrant, accumulator layout) += P[rows r0 ..][k0 .. k1) . Q[rows q0 ..][k0 .. k1)^T, both row panels of A;
    // k0, k1 multiples of 64.  One wave per SIMD: nothing hides a latency unless the code does.  Chunks of 16 columns; FOUR chunks of
    // global loads in flight (the tiles come from other CUs' stores, ~2 us away); two LDS buffers and two operand register sets: while
    // the 16 MFMAs of chunk c issue, chunk c + 1 goes registers -> LDS -> barrier -> operand registers in between them.
    auto panel_product = [&](pt_f64x4 (&c)[2][2], int64_t r0, int64_t q0, int64_t k0, int64_t k1, int gate_row) {
        const int qmn = tid >> 2, qk0 = (tid & 3) * 4;
        double ra[4][4], rb[4][4], oa[2][4][2], ob[2][4][2];
        if (k0 >= k1) return;
        int seen = 0;
        auto gate = [&](int64_t k) {                       // the 64-column tile of row gate_row that starts at column k
            if (gate_row < 0 || k >= k1) return;
            const int need = (int)((k - c0) / NB) + 1;
            if (seen < need) seen = wait_for(gate_row, need);
        };
        const double* pa = Ab + (r0 + qmn) * lda + qk0;
        const double* pb = Ab + (q0 + qmn) * lda + qk0;
        const int64_t C = (k1 - k0) / 16;
#define PT_LOAD(s, k) do { _Pragma("unroll") for (int j = 0; j < 4; ++j) { ra[s][j] = pa[(k) + j]; rb[s][j] = pb[(k) + j]; } } while (0)
#define PT_STORE(s, b) do { _Pragma("unroll") for (int j = 0; j < 4; ++j) { sm[b][0][(qk0 + j) * PT_SLD + qmn] = ra[s][j]; sm[b][1][(qk0 + j) * PT_SLD + qmn] = rb[s][j]; } } while (0)
#define PT_READ(b, o) do { _Pragma("unroll") for (int q = 0; q < 4; ++q) _Pragma("unroll") for (int x = 0; x < 2; ++x) {                     \
            oa[o][q][x] = sm[b][0][(4 * q + lq) * PT_SLD + wm + 16 * x + li]; ob[o][q][x] = sm[b][1][(4 * q + lq) * PT_SLD + wn + 16 * x + li]; } } while (0)
#define PT_MMA(o, q0_, q1_) do { _Pragma("unroll") for (int q = (q0_); q < (q1_); ++q) _Pragma("unroll") for (int x = 0; x < 2; ++x)          \
            _Pragma("unroll") for (int y = 0; y < 2; ++y) c[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(oa[o][q][x], ob[o][q][y], c[x][y], 0, 0, 0); } while (0)
        gate(k0);
        PT_LOAD(0, k0); PT_LOAD(1, k0 + 16); PT_LOAD(2, k0 + 32); PT_LOAD(3, k0 + 48);
        gate(k0 + 64);
        PT_STORE(0, 0);
        __syncthreads();
        if (C > 4) PT_LOAD(0, k0 + 64);
        PT_READ(0, 0);
        for (int64_t m = 0; m < C; m += 4) {
            gate(k0 + 16 * (m + 8));
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int64_t cc = m + s;
                const bool nxt = cc + 1 < C;
                if (nxt) PT_STORE((s + 1) & 3, (s + 1) & 1);
                PT_MMA(s & 1, 0, 2);
                if (nxt) {
                    __syncthreads();
                    if (cc + 5 < C) PT_LOAD((s + 1) & 3, k0 + 16 * (cc + 5));
                    PT_READ((s + 1) & 1, (s + 1) & 1);
                }
                PT_MMA(s & 1, 2, 4);
            }
        }
#undef PT_LOAD
#undef PT_STORE
#undef PT_READ
#undef PT_MMA
    };
    auto zero = [&](pt_f64x4 (&c)[2][2]) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) c[x][y] = pt_f64x4{0.0, 0.0, 0.0, 0.0};
    };
    // accumulator element (x, y, r) <-> tile element (row wm + 16 x + lq + 4 r, column wn + 16 y + li)
    const int64_t ri = c0 + (int64_t)i * NB;
    pt_f64x4 cd[2][2];          // running sum_k L[i][k] L[i][k]^T of the diagonal tile
    zero(cd);
    const int jend = i < npt ? i : npt;
    pt_f64x4 dg[2][2];          // A[i][i] itself, fetched now: the factorisation of the diagonal tile is the critical path of its block column
    if (i < npt) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) dg[x][y][r] = Ab[(ri + wm + 16 * x + lq + 4 * r) * lda + ri + wn + 16 * y + li];
    }

    for (int j = 0; j < jend; ++j) {
        const int64_t rj = c0 + (int64_t)j * NB;
        pt_f64x4 c[2][2];
        zero(c);
        [[maybe_unused]] const int jt = j;
        PT_STAMP(0);
        panel_product(c, ri, rj, c0, rj, j);                      // sum_{k<j} L[i][k] L[j][k]^T  (row j's tiles k < j: gated on progress[j])
        PT_STAMP(1);
        __syncthreads();                                           // (the product's last chunk has been read: its LDS becomes the tile)
        // (the tile's own entries do not depend on L[j][j]: they are in LDS before it arrives)
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = wm + 16 * x + lq + 4 * r, cc = wn + 16 * y + li;
                    t[rr][cc] = Ab[(ri + rr) * lda + rj + cc] - c[x][y][r];
                }
        wait_for(j, j + 1);                                        // L[j][j] and the inverses of its four 16 x 16 diagonal blocks
        PT_STAMP(2);
        pt_f64x4 mreg[4];                                          // this lane's entries of the inverses, as MFMA A operands: M_b[li][4 r + lq]
        {
            double lv[16];                                         // 16 independent loads in flight, then LDS
            const int r0 = tid >> 6, cc = tid & 63;
#pragma unroll
            for (int u = 0; u < 16; ++u) lv[u] = Ab[(rj + r0 + 4 * u) * lda + rj + cc];
            double mvv[4];                                         // the four inverses: 1024 contiguous values, through LDS as well
#pragma unroll
            for (int u = 0; u < 4; ++u) mvv[u] = invs[(int64_t)j * 1024 + tid + 256 * u];
#pragma unroll
            for (int u = 0; u < 16; ++u) a[r0 + 4 * u][cc] = (cc <= r0 + 4 * u) ? lv[u] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) minv[u][tid >> 4][tid & 15] = mvv[u];
        }
        __syncthreads();
#pragma unroll
        for (int bb = 0; bb < 4; ++bb)
#pragma unroll
            for (int r = 0; r < 4; ++r) mreg[bb][r] = minv[bb][li][4 * r + lq];
        PT_STAMP(3);
        // X L[j][j]^T = T, one 16-row tile per wave, entirely in registers (accumulator layout of the TRANSPOSED tile: lane (li, lq),
        // register r = element (row li, column lq + 4 r) of a 16 x 16 block): X_b = Y_b M_b^T with the published inverse M_b of the
        // diagonal block (4 MFMAs) instead of 16 dependent substitution steps, then Y_b'' -= X_b L_b''b^T for the blocks to the right.
        {
            pt_f64x4 tacc[4];
            const int rw = wave * 16;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb)
#pragma unroll
                for (int r = 0; r < 4; ++r) tacc[bb][r] = t[rw + li][16 * bb + lq + 4 * r];
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                pt_f64x4 xs = pt_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r) xs = __builtin_amdgcn_mfma_f64_16x16x4f64(mreg[bb][r], tacc[bb][r], xs, 0, 0, 0);
#pragma unroll
                for (int b2 = bb + 1; b2 < 4; ++b2)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        tacc[b2] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[16 * b2 + li][16 * bb + 4 * r + lq], xs[r], tacc[b2], 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) t[rw + li][16 * bb + lq + 4 * r] = xs[r];
            }
        }
        __syncthreads();
        PT_STAMP(4);
        {
            const int r0 = tid >> 6, cc = tid & 63;
#pragma unroll
            for (int u = 0; u < 16; ++u) Ab[(ri + r0 + 4 * u) * lda + rj + cc] = t[r0 + 4 * u][cc];
        }
        // the diagonal tile's share of this column, straight from the solved tile in LDS: cd += L[i][j] L[i][j]^T (the stores above drain
        // meanwhile; the tile is published after it -- the rows below need it for their NEXT column's product only)
        if (i < npt) {
#pragma unroll 4
            for (int ks = 0; ks < NB; ks += 4) {
                double av[2], bv[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) { av[x] = t[wm + 16 * x + li][ks + lq]; bv[x] = t[wn + 16 * x + li][ks + lq]; }
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) cd[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], cd[x][y], 0, 0, 0);
            }
        }
        PT_STAMP(5);
        __threadfence();
        __syncthreads();                                           // (also: t is rewritten by the next tile)
        if (tid == 0 && !nowait) __hip_atomic_store(progress + i, j + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        PT_STAMP(6);
    }
    // M_b = L_bb^-1 of the 16 x 16 block at a[blk ..][blk ..] (one wave; straight to the hand-off scratch): row by row, M[c][:] = W[c][:] / l_cc,
    // then W[R][:] -= L[R][c] M[c][:] for the rows below as ONE rank-1 MFMA; accumulator lane (li, lq), register r = element (lq + 4 r, li).
    auto inverse16 = [&](int blk) {
        pt_f64x4 lb, wv, mv = pt_f64x4{0.0, 0.0, 0.0, 0.0};
        double iv[16];
#pragma unroll
        for (int r = 0; r < 4; ++r) { lb[r] = a[blk + li][blk + lq + 4 * r]; wv[r] = (lq + 4 * r == li) ? 1.0 : 0.0; }
#pragma unroll
        for (int c = 0; c < 16; ++c) iv[c] = invd[blk + c];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int p = c >> 2, sg = c & 3;
            const double msel = (lq == sg) ? 1.0 : 0.0;
            const double mrow = (wv[p] * iv[c]) * msel;
            mv[p] += mrow;
            if (c < 15) wv = __builtin_amdgcn_mfma_f64_16x16x4f64(-lb[p] * msel, mrow, wv, 0, 0, 0);
        }
        double* dst = invs + (int64_t)i * 1024 + (blk >> 4) * 256 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(lq + 4 * r) * 16] = mv[r];
    };
    if (i < npt) {
    [[maybe_unused]] const int jt = i;
    PT_STAMP(7);
    // diagonal tile: factor A[i][i] - cd
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = wm + 16 * x + lq + 4 * r, cc = wn + 16 * y + li;
                a[rr][cc] = (cc <= rr) ? dg[x][y][r] - cd[x][y][r] : 0.0;
            }
    __syncthreads();
    PT_STAMP(8);
    for (int blk = 0; blk < NB; blk += 16) {
        if (wave == 0) {
            // 16 x 16 sub-block on the matrix pipe: the block sits in ONE MFMA accumulator (lane (li, lq), register r = element
            // (row li, column lq + 4 r), valid for column <= row), and every column step is d -> 1/sqrt(d) -> scale -> ONE rank-1 MFMA
            // (operand: the scaled column in the lanes lq == c % 4, zero elsewhere) instead of 15 readlane + FMA column updates:
            // ~15 instructions on the serial chain of a column instead of ~55.
            pt_f64x4 cv, lv = pt_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r) cv[r] = a[blk + li][blk + lq + 4 * r];
            int bad = 99;
            double myinv = 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int p = c >> 2, sg = c & 3;
                // (branch-free; a non-positive pivot is reported below and its column left unscaled: the factor stays finite)
                const double d = readlane_t(cv[p], sg * 16 + c);
                bad = (!(d > 0.0) && bad > c) ? c : bad;
                const double rs = inv_sqrt(d);
                const double inv = (d > 0.0) ? rs : 1.0;
                const double m = (lq == sg && li >= c) ? 1.0 : 0.0;       // this column's lanes: rows c .. 15 in lane group c % 4
                const double l = (cv[p] * inv) * m;
                lv[p] += l;                                                // (exactly one non-zero contribution per lane and register)
                myinv = (lane == c) ? inv : myinv;
                if (c < 15) cv = __builtin_amdgcn_mfma_f64_16x16x4f64(-l, l, cv, 0, 0, 0);
            }
            if (bad < 16 && lane == 0 && info && info[b] == 0) info[b] = (int)(ri + blk + bad + 1);
            if (lane < 16) invd[blk + lane] = myinv;
#pragma unroll
            for (int r = 0; r < 4; ++r) a[blk + li][blk + lq + 4 * r] = (lq + 4 * r <= li) ? lv[r] : 0.0;
        }
        __syncthreads();
        if (blk == 0) PT_STAMP(11);
        if (wave == 1) inverse16(blk);                     // M_b for the solving workgroups, next to wave 0's substitution below
        if (blk + 16 < NB) {
            const int rr = blk + 16 + tid;                 // rows below the sub-block: X L_bb^T = A_ib
            if (rr < NB) {
                double x[16];
#pragma unroll
                for (int c2 = 0; c2 < 16; ++c2) {
                    double s0 = a[rr][blk + c2], s1 = 0.0;
#pragma unroll
                    for (int k = 0; k + 1 < c2; k += 2) { s0 = fma(-x[k], a[blk + c2][blk + k], s0); s1 = fma(-x[k + 1], a[blk + c2][blk + k + 1], s1); }
                    if (c2 & 1) s0 = fma(-x[c2 - 1], a[blk + c2][blk + c2 - 1], s0);
                    x[c2] = (s0 + s1) * invd[blk + c2];
                }
#pragma unroll
                for (int c2 = 0; c2 < 16; ++c2) a[rr][blk + c2] = x[c2];
            }
            __syncthreads();
            if (blk == 0) PT_STAMP(12);
            int tix = 0;                                   // trailing lower tiles of 16 x 16, dealt to the four waves
            for (int I0 = blk + 16; I0 < NB; I0 += 16)
                for (int J0 = blk + 16; J0 <= I0; J0 += 16, ++tix) {
                    if ((tix & 3) != wave) continue;
                    double af[4], bf[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { af[q] = -a[I0 + li][blk + 4 * q + lq]; bf[q] = a[J0 + li][blk + 4 * q + lq]; }
                    pt_f64x4 cf;
#pragma unroll
                    for (int r = 0; r < 4; ++r) cf[r] = a[I0 + lq + 4 * r][J0 + li];
#pragma unroll
                    for (int q = 0; q < 4; ++q) cf = __builtin_amdgcn_mfma_f64_16x16x4f64(af[q], bf[q], cf, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[I0 + lq + 4 * r][J0 + li] = cf[r];
                }
            __syncthreads();
            if (blk == 0) PT_STAMP(13);
        }
    }
    PT_STAMP(9);
    if (wave != 1) {                                       // (wave 1 is still busy with the last block's inverse)
        const int t3 = (wave == 0 ? 0 : wave - 1) * 64 + lane;
        for (int e = t3; e < NB * NB; e += 192) { const int r = e >> 6, cc = e & 63; Ab[(ri + r) * lda + ri + cc] = (cc <= r) ? a[r][cc] : 0.0; }
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(progress + i, i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    PT_STAMP(10);
    }
    if (tid == 0 && !nowait) {
        if (lost && info) info[b] = -1;
        // the workgroup that completes last leaves the counters at zero for the next launch (every poll of a counter precedes the poller's own completion)
        if (__hip_atomic_fetch_add(progress + nbk, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nbk - 1)
            for (int r = 0; r <= nbk; ++r) __hip_atomic_store(progress + r, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- op(L_kk) X = B_k (X overwrites B_k): one right-hand-side column per lane ------------------------------
// TRANS: solve L_kk^T X = B_k by index reversal (P L^T P is lower triangular)
template <typename T, bool TRANS>
__global__ __launch_bounds__(256) void solve_cols_kernel(const T* __restrict__ L, int64_t ldl, int64_t sL, T* __restrict__ B,
                                                          int64_t ldb, int64_t sB, int64_t k0, int nb, int64_t c0, int64_t ncols) {
    __shared__ T l[NB][NB + 1];
    const int tid = threadIdx.x, b = blockIdx.y;
    const T* Lkk = L + (int64_t)b * sL + k0 * ldl + k0;
    T* Bk = B + (int64_t)b * sB + k0 * ldb;
    {   // 16 loads per thread, issued back to back before the LDS stores (see potrf_panel_kernel)
        T vl[NB * NB / 256];
#pragma unroll
        for (int it = 0; it < NB * NB / 256; ++it) {
            const int e = tid + it * 256, i = e / NB, m = e % NB;
            T v = (T)0;
            if (i < nb && m < nb) {
                if (m <= i) v = TRANS ? Lkk[(int64_t)(nb - 1 - m) * ldl + (nb - 1 - i)] : Lkk[(int64_t)i * ldl + m];
            } else if (i == m) v = (T)1;
            vl[it] = v;
        }
#pragma unroll
        for (int it = 0; it < NB * NB / 256; ++it) { const int e = tid + it * 256; l[e / NB][e % NB] = vl[it]; }
    }
    __syncthreads();
    const int64_t c = c0 + (int64_t)blockIdx.x * 256 + tid;
    if (c >= c0 + ncols) return;
    // forward substitution in chunks of 8 rows: solved rows are written back to B (in place) and re-read from
    // L1/L2 by later chunks (coalesced across lanes), so only 8 values are live in registers at a time
    constexpr int CH = 8;
    for (int ib = 0; ib < nb; ib += CH) {
        T sacc[CH];
#pragma unroll
        for (int r = 0; r < CH; ++r) {
            const int i = ib + r;
            const int gi = TRANS ? nb - 1 - i : i;
            sacc[r] = (i < nb) ? Bk[(int64_t)gi * ldb + c] : (T)0;
        }
        for (int m = 0; m < ib; ++m) {
            const int gm = TRANS ? nb - 1 - m : m;
            const T xm = Bk[(int64_t)gm * ldb + c];
#pragma unroll
            for (int r = 0; r < CH; ++r) sacc[r] = fma(-xm, l[ib + r][m], sacc[r]);
        }
#pragma unroll
        for (int r = 0; r < CH; ++r) {
#pragma unroll
            for (int m = 0; m < r; ++m) sacc[r] = fma(-sacc[m], l[ib + r][ib + m], sacc[r]);
            sacc[r] = sacc[r] / l[ib + r][ib + r];
        }
#pragma unroll
        for (int r = 0; r < CH; ++r) {
            const int i = ib + r;
            const int gi = TRANS ? nb - 1 - i : i;
            if (i < nb) Bk[(int64_t)gi * ldb + c] = sacc[r];
        }
    }
}

// ---- inverse of every 64x64 diagonal block of L in ONE launch (one wave per block) -----------------------------------------------------
// Blocked: the four 16 x 16 diagonal sub-blocks by substitution (16 lanes per sub-block, one column of the inverse per lane, the column in
// registers), then two merge levels  inv([A 0; B C]) = [A^-1 0; -C^-1 B A^-1, C^-1]  as 16 x 16 MFMA products on the LDS image.
// (The un-blocked form -- one column per lane, 64 dependent steps through LDS -- took ~120 us.)
template <typename T> struct Mfma16;
template <> struct Mfma16<double> {
    typedef double vec __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ vec mma(double a, double b, vec c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lq, int r) { return lq + 4 * r; }       // C/D: row = (lane >> 4) + 4 r
};
template <> struct Mfma16<float> {
    typedef float vec __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ vec mma(float a, float b, vec c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lq, int r) { return lq * 4 + r; }       // C/D: row = (lane >> 4) * 4 + r
};
// D (16 x 16 at Dst[d0r.., d0c..]) = sgn * A (16 x K16) * B (K16 x 16), A at As[a0r.., a0c..], B at Bs[b0r.., b0c..]; K16 = 16 * kt
template <typename T>
__device__ __forceinline__ void lds_mm16(T (*Dst)[NB + 1], int d0r, int d0c, T (*As)[NB + 1], int a0r, int a0c, T (*Bs)[NB + 1], int b0r, int b0c,
                                         int kt, T sgn, int lane) {
    const int li = lane & 15, lq = lane >> 4;
    typename Mfma16<T>::vec c;
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = (T)0;
    for (int k = 0; k < 16 * kt; k += 4) c = Mfma16<T>::mma(sgn * As[a0r + li][a0c + k + lq], Bs[b0r + k + lq][b0c + li], c);
#pragma unroll
    for (int r = 0; r < 4; ++r) Dst[d0r + Mfma16<T>::row(lq, r)][d0c + li] = c[r];
}
template <typename T>
__global__ __launch_bounds__(64) void trtri_diag_kernel(const T* __restrict__ L, int64_t ldl, int64_t sL, T* __restrict__ Li, int64_t ldi,
                                                        int64_t sI, int64_t n) {
    __shared__ T l[NB][NB + 1];
    __shared__ T x[NB][NB + 1];
    __shared__ T w[NB][NB + 1];              // products L21 I11 of the merge levels
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * NB;
    const int nb = (int)((k0 + NB < n) ? NB : n - k0);
    const T* Lkk = L + (int64_t)b * sL + k0 * ldl + k0;
    T* Ikk = Li + (int64_t)b * sI + k0 * ldi + k0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {       // 2 x 32 loads per lane, each batch issued back to back (see potrf_panel_kernel)
        T vl[NB / 2];
#pragma unroll
        for (int it = 0; it < NB / 2; ++it) {
            const int e = tid + (half * (NB / 2) + it) * 64, i = e / NB, m = e % NB;
            T v = (T)0;
            if (i < nb && m < nb) { if (m <= i) v = Lkk[(int64_t)i * ldl + m]; }
            else if (i == m) v = (T)1;          // identity padding of a ragged last block
            vl[it] = v;
        }
#pragma unroll
        for (int it = 0; it < NB / 2; ++it) {
            const int e = tid + (half * (NB / 2) + it) * 64;
            l[e / NB][e % NB] = vl[it];
            x[e / NB][e % NB] = (T)0;
        }
    }
    __syncthreads();
    {   // 16 x 16 diagonal sub-blocks: lane group g = tid / 16 owns sub-block g, lane c = tid % 16 column c of its inverse
        const int g0 = (tid >> 4) * 16, c = tid & 15;
        T xc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            T sacc = (i == c) ? (T)1 : (T)0;
#pragma unroll
            for (int m = 0; m < i; ++m) sacc = fma(-l[g0 + i][g0 + m], (m >= c) ? xc[m] : (T)0, sacc);
            xc[i] = (i >= c) ? sacc / l[g0 + i][g0 + i] : (T)0;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) x[g0 + i][g0 + c] = xc[i];
    }
    __syncthreads();
    // merge 16 -> 32: pairs (0,1) and (2,3):  X21 = -I22 (L21 I11)
    for (int p = 0; p < 2; ++p) {
        const int o = 32 * p;
        lds_mm16<T>(w, o + 16, o, l, o + 16, o, x, o, o, 1, (T)1, tid);                 // W = L21 I11
    }
    __syncthreads();
    for (int p = 0; p < 2; ++p) {
        const int o = 32 * p;
        lds_mm16<T>(x, o + 16, o, x, o + 16, o + 16, w, o + 16, o, 1, (T)-1, tid);      // X21 = -I22 W
    }
    __syncthreads();
    // merge 32 -> 64: L21 = l[32:64][0:32], I11 = x[0:32][0:32], I22 = x[32:64][32:64] (both lower triangular, explicit zeros above)
    for (int ti = 0; ti < 2; ++ti)
        for (int tj = 0; tj < 2; ++tj) lds_mm16<T>(w, 32 + 16 * ti, 16 * tj, l, 32 + 16 * ti, 0, x, 0, 16 * tj, 2, (T)1, tid);
    __syncthreads();
    for (int ti = 0; ti < 2; ++ti)
        for (int tj = 0; tj < 2; ++tj) lds_mm16<T>(x, 32 + 16 * ti, 16 * tj, x, 32 + 16 * ti, 32, w, 32, 16 * tj, 2, (T)-1, tid);
    __syncthreads();
    for (int e = tid; e < nb * nb; e += 64) {
        const int i = e / nb, m = e % nb;
        Ikk[(int64_t)i * ldi + m] = x[i][m];
    }
}

template <typename T>
__global__ void zero_upper_kernel(T* A, int64_t n, int64_t lda, int64_t sA) {
    T* a = A + (int64_t)blockIdx.z * sA;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col < n && col > row) a[row * lda + col] = (T)0;
}

template <typename T>
__global__ void set_identity_kernel(T* A, int64_t n, int64_t lda, int64_t sA) {
    T* a = A + (int64_t)blockIdx.z * sA;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (col < n) a[row * lda + col] = (col == row) ? (T)1 : (T)0;
}

template <typename T>
__global__ __launch_bounds__(256) void sumlogdiag_kernel(const T* __restrict__ L, int64_t n, int64_t ldl, int64_t sL, T* __restrict__ out) {
    __shared__ T red[16];
    const T* l = L + (int64_t)blockIdx.x * sL;
    T s = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += log(fabs(l[i * ldl + i]));
    s = block_sum<T>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- the block rows BELOW an outer panel (r03) ------------------------------------------------------------------------------------------
// After the panel's own block rows are factored (potrf_tiles_kernel, the latency chain), every row below solves  L[i][0..npt) L11^T = A[i][0..npt)
// against the FINISHED diagonal block L11.  potrf_tiles_kernel did that one 64 x 64 tile at a time, left-looking, the whole workgroup on one
// tile: ~37 us per tile, 0.3 ms per outer panel at n = 8192 although a block row's matrix work is 25 us (these launches were 2.5 of
// potrf(8192)'s 7.3 ms, and only rows / 64 <= 120 of the 256 CUs had a workgroup).  Here a workgroup of EIGHT waves keeps the block row's eight
// tiles in registers, one per wave (64 x 64 float64 = 128 VGPRs in the accumulator layout), and goes RIGHT-looking:
//   step k: the owner of tile k puts it into LDS (two buffers, alternating);  waves 0..3 solve  X L[k][k]^T = T  in place, 16 rows each, with
//   the published inverses of L[k][k]'s four 16 x 16 diagonal blocks (the substitution of potrf_tiles_kernel);  X goes to global memory (it is
//   L[i][k]);  every wave j > k updates its tile in place,  A[i][j] -= X L[j][k]^T,  the L[j][k] operand straight from global memory (L11 is
//   2 MB: L2-resident, every workgroup reads the same tiles) three 16-column groups ahead of the MFMAs that use them.
// Two barriers per step; the critical chain of a block row is npt x (solve + one tile update by one wave, 256 MFMAs).
// (Measured and dropped: this launch NEXT TO the panel's chain on a second auxiliary stream, following the chain's progress counters column
//  by column -- it then ends 17 us after the chain, but the chain itself takes 0.30 - 0.36 instead of 0.19 ms (the followers' acquire fences
//  and tile reads share its L2) and 120 mostly waiting workgroups hold CUs the look-ahead GEMM wants: potrf(8192) 7.18 vs 6.72 ms.)
// MFMA conventions as potrf_tiles_kernel: A operand lane (li, lq) = P[m = li][k = lq], B operand = Q[n = li][k = lq], accumulator register r of
// lane (li, lq) = element (row lq + 4 r, column li).
// RH (r06): rows per workgroup.  A block row's critical chain is npt x (solve + ONE wave's tile update): at 64 rows that update is 256 float64
// MFMAs of 64 cycles each, 7.8 us, i.e. >= 62 us per outer panel on <= 120 of the 256 CUs.  32 rows halve the chain and double the workgroup
// count (each re-reads the L2-resident diagonal block L11: 1.2 MB per workgroup).
static_assert(NBO / NB <= 8, "potrf_rows_kernel: one wave per tile of the panel, eight waves");
__global__ __launch_bounds__(512) void potrf_rows_kernel(double* __restrict__ A, int64_t lda, int64_t sA, int64_t c0, int npt, int row0,
                                                         const double* __restrict__ inv_all) {
    constexpr int RH = 32;
    constexpr int XR = RH / 16;
    __shared__ double Tb[2][RH][NB + 1];
    __shared__ double a[NB][NB + 1];          // L[k][k]
    __shared__ double minv[4][16][17];        // the inverses of its four 16 x 16 diagonal blocks
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int b = blockIdx.y;
    double* Ab = A + (int64_t)b * sA;
    const double* invs = inv_all + (int64_t)b * npt * 1024;
    const int64_t ri = c0 + (int64_t)row0 * NB + (int64_t)blockIdx.x * RH;      // (row0 in units of NB rows)
    const bool own = wave < npt;
    const int64_t rjw = c0 + (int64_t)wave * NB;
    pt_f64x4 acc[XR][4];
    if (own) {
#pragma unroll
        for (int x = 0; x < XR; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[x][y][r] = Ab[(ri + 16 * x + lq + 4 * r) * lda + rjw + 16 * y + li];
    }
    for (int k = 0; k < npt; ++k) {
        const int64_t rk = c0 + (int64_t)k * NB;
        double (*T)[NB + 1] = Tb[k & 1];
        // operands that do not depend on this step's tile: requested in front of the barriers
        double lv[8];                           // L[k][k], element e = tid + 512 u <-> (row e / 64, column e % 64); lower triangle
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 512 * u, rr = e >> 6, cc = e & 63;
            lv[u] = (cc <= rr) ? Ab[(rk + rr) * lda + rk + cc] : 0.0;
        }
        const double mv0 = invs[(int64_t)k * 1024 + tid], mv1 = invs[(int64_t)k * 1024 + 512 + tid];
        const bool upd = own && wave > k;
        const double* lj = Ab + (rjw + li) * lda + rk + lq;            // L[j = wave][k][n = li + 16 y][c = lq + 4 q]
        // the update's B operand in groups of four k steps (16 columns of L[j][k]), three groups ahead of the MFMAs that use them
        auto lgroup = [&](int g, double (&d)[4]) {           // group g = 4 y + qq: rows 16 y + li, columns 16 qq + 4 t + lq
            const double* p = lj + (int64_t)16 * (g >> 2) * lda + 16 * (g & 3);
#pragma unroll
            for (int t = 0; t < 4; ++t) d[t] = p[4 * t];
        };
        double b0[4], b1[4], b2[4], b3[4];
        if (upd) { lgroup(0, b0); lgroup(1, b1); lgroup(2, b2); }
        if (wave == k) {
#pragma unroll
            for (int x = 0; x < XR; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y)
#pragma unroll
                    for (int r = 0; r < 4; ++r) T[16 * x + lq + 4 * r][16 * y + li] = acc[x][y][r];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = tid + 512 * u; a[e >> 6][e & 63] = lv[u]; }
        minv[tid >> 8][(tid >> 4) & 15][tid & 15] = mv0;
        minv[2 + (tid >> 8)][(tid >> 4) & 15][tid & 15] = mv1;
        __syncthreads();
        if (wave < XR) {
            // X L[k][k]^T = T, 16 rows per wave, in registers (accumulator layout of the TRANSPOSED tile: lane (li, lq), register r = element
            // (row li, column lq + 4 r) of a 16 x 16 block): X_b = Y_b M_b^T with the published inverse M_b (4 MFMAs), then
            // Y_b'' -= X_b L_b''b^T for the blocks to the right -- as potrf_tiles_kernel
            pt_f64x4 mreg[4], tacc[4];
            const int rw = wave * 16;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb)
#pragma unroll
                for (int r = 0; r < 4; ++r) { mreg[bb][r] = minv[bb][li][4 * r + lq]; tacc[bb][r] = T[rw + li][16 * bb + lq + 4 * r]; }
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                pt_f64x4 xs = pt_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < 4; ++r) xs = __builtin_amdgcn_mfma_f64_16x16x4f64(mreg[bb][r], tacc[bb][r], xs, 0, 0, 0);
#pragma unroll
                for (int b2i = bb + 1; b2i < 4; ++b2i)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        tacc[b2i] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[16 * b2i + li][16 * bb + 4 * r + lq], xs[r], tacc[b2i], 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) T[rw + li][16 * bb + lq + 4 * r] = xs[r];
            }
        }
        __syncthreads();
        {   // L[i][k] = X to global memory, coalesced
#pragma unroll
            for (int u = 0; u < RH / 8; ++u) { const int e = tid + 512 * u, rr = e >> 6, cc = e & 63; Ab[(ri + rr) * lda + rk + cc] = T[rr][cc]; }
        }
        if (upd) {
#pragma unroll
            for (int y = 0; y < 4; ++y) {
#pragma unroll 1
                for (int qq = 0; qq < 4; ++qq) {
                    const int g = 4 * y + qq;
                    if (g + 3 < 16) lgroup(g + 3, b3);
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int x = 0; x < XR; ++x)
                            acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(-T[16 * x + li][16 * qq + 4 * t + lq], b0[t], acc[x][y], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < 4; ++t) { b0[t] = b1[t]; b1[t] = b2[t]; b2[t] = b3[t]; }
                }
            }
        }
    }
}

template <typename T>
__global__ void zero_block_kernel(T* __restrict__ P, int64_t rows, int64_t cols, int64_t ld, int64_t stride) {
    T* p = P + (int64_t)blockIdx.y * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += (int64_t)gridDim.x * blockDim.x)
        p[(i / cols) * ld + (i % cols)] = (T)0;
}

// Kernel templates land in the code object in the order they are first used.  This list uses each instance once, in the order the code
// object has always had, so that host code below can be rearranged without moving device code (the device assembly of a host-only change
// then compares equal).  Host-side only; never read.
[[maybe_unused]] const void* const chol_kernel_order[] = {
    (const void*)potrf_panel_kernel<float>, (const void*)zero_upper_kernel<float>, (const void*)zero_upper_kernel<double>,
    (const void*)zero_block_kernel<double>, (const void*)potrf_panel_kernel<double>,
    (const void*)solve_cols_kernel<float, false>, (const void*)solve_cols_kernel<float, true>,
    (const void*)solve_cols_kernel<double, false>, (const void*)solve_cols_kernel<double, true>,
    (const void*)trtri_diag_kernel<float>, (const void*)zero_block_kernel<float>, (const void*)trtri_diag_kernel<double>,
    (const void*)sumlogdiag_kernel<float>, (const void*)sumlogdiag_kernel<double>};

// ---- triangular inverse ------------------------------------------------------------------------------------------------------------------
// The merge step:  inv([L11 0; L21 L22]) = [I11 0; -I22 L21 I11, I22]  for `batch` pairs of a b1-row first and a b2-row second block (Lp / Ip:
// the first pair's corner in the factor / the inverse, stL / stI: pair strides), given I11 and I22, in two MFMA GEMMs; the temporary
// (L21 I11)^T lives in the (unused, finally zeroed) upper-triangular mirror block of the output, so no extra workspace is needed.
// Both products have a triangular left operand: with `tri` only the non-zero k range of each row tile is multiplied.
//   p1: tmpT (b1 x b2, in the mirror block) = I11^T L21^T -- needs I11 and L21, NOT I22 (the bulk of the work);
//   p2: X21 = -I22 tmpT^T, then the mirror block zeroed again (it becomes part of the next level's I11 operand).
template <typename T>
int trtri_merge_p1(mxf_ctx* h, int dtype, int64_t b1, int64_t b2, const T* Lp, int64_t ldl, int64_t stL, T* Ip, int64_t ldi, int64_t stI, int batch,
                   bool tri, hipStream_t st) {
    return mxf_gemm_internal(h, st, {.dtype = dtype, .ta = 1, .tb = 1, .M = b1, .N = b2, .K = b1, .A = {Ip, ldi, stI}, .B = {Lp + b1 * ldl, ldl, stL},
                                     .C = {Ip + b1, ldi, stI}, .batch = batch, .tri = tri ? MXF_TRI_UPPER : MXF_TRI_NONE});
}
template <typename T>
int trtri_merge_p2(mxf_ctx* h, int dtype, int64_t b1, int64_t b2, T* Ip, int64_t ldi, int64_t stI, int batch, bool tri, hipStream_t st) {
    int rc = mxf_gemm_internal(h, st, {.dtype = dtype, .tb = 1, .M = b2, .N = b1, .K = b2, .alpha = -1.0, .A = {Ip + b1 * (ldi + 1), ldi, stI}, .B = {Ip + b1, ldi, stI},
                                       .C = {Ip + b1 * ldi, ldi, stI}, .batch = batch, .tri = tri ? MXF_TRI_LOWER : MXF_TRI_NONE});
    if (rc) return rc;
    hipLaunchKernelGGL((zero_block_kernel<T>), dim3((unsigned)((b1 * b2 + 255) / 256 > 1024 ? 1024 : (b1 * b2 + 255) / 256), (unsigned)batch), dim3(256), 0, st,
                       Ip + b1, b1, b2, ldi, stI);
    return 0;
}

// Log-depth blocked inverse of a lower-triangular matrix.  Level 0: all 64x64 diagonal blocks (one launch); then the merge levels of
// chol_plan.h (trtri_level).  From TRI_MIN-wide blocks on the products skip the zero k range -- trtri(8192) 6.9 -> 5.0 ms; the small levels
// keep the plain split-K products, which fill the chip better.
template <typename T>
int trtri_typed(mxf_ctx* h, hipStream_t st, const MxfTrtri& d) {
    const int64_t n = d.n, ldl = d.L.ld, sL = d.L.stride, ldi = d.Linv.ld, sI = d.Linv.stride;
    const T* L = (const T*)d.L.p; T* Li = (T*)d.Linv.p;
    const int dtype = d.dtype, S = d.S;
    if (const char* why = chol_rows_refusal(n)) MXF_FAIL(h, -3, "mxf_trtri: %s", why);
    const int64_t nblk = (n + NB - 1) / NB;
    hipLaunchKernelGGL((trtri_diag_kernel<T>), dim3((unsigned)nblk, S), dim3(64), 0, st, L, ldl, sL, Li, ldi, sI, n);
    for (int l = 0; l < trtri_levels(n); ++l) {
        const TrtriLevel v = trtri_level(n, l);
        for (int s = 0; s < S; ++s) {
            const T* Ls = L + (int64_t)s * sL;
            T* Is = Li + (int64_t)s * sI;
            if (v.pairs > 0) {
                const int64_t stL = 2 * v.bs * (ldl + 1), stI = 2 * v.bs * (ldi + 1);
                int rc = trtri_merge_p1<T>(h, dtype, v.bs, v.bs, Ls, ldl, stL, Is, ldi, stI, (int)v.pairs, v.tri, st);
                if (!rc) rc = trtri_merge_p2<T>(h, dtype, v.bs, v.bs, Is, ldi, stI, (int)v.pairs, v.tri, st);
                if (rc) return rc;
            }
            if (v.ragged_b2 > 0) {
                const int64_t r0 = v.ragged_at;
                int rc = trtri_merge_p1<T>(h, dtype, v.bs, v.ragged_b2, Ls + r0 * (ldl + 1), ldl, 0, Is + r0 * (ldi + 1), ldi, 0, 1, v.tri, st);
                if (!rc) rc = trtri_merge_p2<T>(h, dtype, v.bs, v.ragged_b2, Is + r0 * (ldi + 1), ldi, 0, 1, v.tri, st);
                if (rc) return rc;
            }
        }
    }
    if (n > 1) hipLaunchKernelGGL((zero_upper_kernel<T>), dim3((unsigned)((n + 255) / 256), (unsigned)n, S), dim3(256), 0, st, Li, n, ldi, sI);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

// ---- potrf: the plan's inputs ---------------------------------------------------------------------------------------------------------------
// Which form a factorisation takes is potrf_plan (chol_plan.h), decided once per call from this request: the shape, the CU count, the knobs and,
// only where look-ahead is possible at all, the capture state and the handle's auxiliary streams, created here on first use.
PotrfRequest potrf_request(mxf_ctx* h, size_t esize, int S, int64_t n, hipStream_t st, bool want_inverse, bool zero_upper) {
    static const int ncu = [] { int dev = 0, v = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 64; return v; }();
    static const int64_t one_max = MXF_KNOB("MXF_POTRF_ONE_MAX", 512), split_rows = MXF_KNOB("MXF_POTRF_SPLIT_ROWS", 64), eager_panels = MXF_KNOB("MXF_POTRF_EAGER_INV", 2);
    PotrfRequest r{.esize = esize, .S = S, .n = n, .ncu = ncu, .want_inverse = want_inverse, .zero_upper = zero_upper,
                   .one_max = one_max, .split_rows = split_rows, .eager_panels = eager_panels};
    if (potrf_may_look(r)) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cap);
        r.capturing = cap != hipStreamCaptureStatusNone;
        r.aux_streams = !r.capturing && mxf_potrf_aux_init(h);
    }
    return r;
}

// ---- potrf: one call and its stages ---------------------------------------------------------------------------------------------------------
// Events of potrf_aux that the caller's stream has not waited on yet.  Only trailing_update sets them, only wait_rest / wait_head clear them, and
// join clears whatever is left: every recorded auxiliary event is waited on by the caller's stream before the call returns.
struct PotrfPending {
    bool rest = false;     // ev_pb: the rest of a trailing update (everything right of the next outer panel)
    bool head = false;     // ev_ph: the update of the rows below the next outer panel's diagonal block
};

// One factorisation: its arguments, its plan and the stages that queue its launches, in enqueue order.  Streams: st (the caller's: the serial
// path), and with look-ahead h->potrf_aux; with the eager inverse also h->potrf_inv and h->potrf_inv_diag.
template <typename T>
struct PotrfCall : PotrfPlan {
    mxf_ctx* h; int dtype; T* A; int64_t lda, sA; int* info; hipStream_t st; T* Ie; int64_t ldie;
    PotrfPending pend;

    int wait_rest() { if (pend.rest) { MXF_HIP(h, hipStreamWaitEvent(st, h->ev_pb, 0)); pend.rest = false; } return 0; }
    int wait_head() { if (pend.head) { MXF_HIP(h, hipStreamWaitEvent(st, h->ev_ph, 0)); pend.head = false; } return 0; }

    // A[r0 : r0 + m, cc : cc + nc] -= A[r0 : r0 + m, k0 : k0 + K] A[cc : cc + nc, k0 : k0 + K]^T on stream q (lower: blocks on and below the diagonal only)
    int update(int64_t r0, int64_t m, int64_t cc, int64_t nc, int64_t k0, int64_t K, int lower, hipStream_t q) {
        return mxf_gemm_internal(h, q, {.dtype = dtype, .tb = 1, .M = m, .N = nc, .K = K, .alpha = -1.0, .A = {A + r0 * lda + k0, lda, sA}, .B = {A + cc * lda + k0, lda, sA},
                                        .beta = 1.0, .C = {A + r0 * lda + cc, lda, sA}, .batch = S, .lower_only = lower});
    }

    // Tile form (panel_tiles) of the outer panel at c0, on st.  Waits on ev_ph if pending.  One launch for all nbr block rows from c0 down, or
    // (split) two: the panel's own npt block rows (the latency chain), then the rows below against the finished diagonal block, right-looking
    // from registers in workgroups of 32 rows (potrf_rows_kernel; ~90 us of MFMA work each, nothing to wait for).  In one launch those rows sit
    // resident and mostly idle for the whole chain, one CU each, and the look-ahead GEMM next to them (whose 133 KB of LDS cannot share a CU with a
    // tile workgroup) runs on what is left.  The chain launch reads the diagonal block only, so in the split form the wait for the auxiliary
    // stream's update of the rows below it comes behind that launch (that update ran next to the chain); every other form waits first.
    int factor_panel_tiles(int64_t c0) {
        const unsigned nbr = (unsigned)((n - c0) / NB), npt = (unsigned)((panel_end(c0) - c0) / NB);
        const bool two = split(c0);
        const unsigned na = two ? npt : nbr;
        if (!two) { int rc = wait_head(); if (rc) return rc; }
        int* progress = mxf_flags(h, (na + 1) * (unsigned)S);
        if (!progress) MXF_FAIL(h, -4, "mxf_potrf: cannot allocate the workgroup hand-off counters");
        double* pinv = mxf_potrf_inv(h, (size_t)npt * S * 1024);
        if (!pinv) MXF_FAIL(h, -4, "mxf_potrf: cannot allocate the inverse-block scratch");
        hipLaunchKernelGGL(potrf_tiles_kernel, dim3(na, (unsigned)S), dim3(256), 0, st, (double*)A, lda, sA, c0, (int)npt, info, progress, pinv, 0, 0);
        int rc = wait_head();
        if (rc) return rc;
        if (two) hipLaunchKernelGGL(potrf_rows_kernel, dim3((nbr - npt) * 2, (unsigned)S), dim3(512), 0, st, (double*)A, lda, sA, c0, (int)npt, (int)npt, (const double*)pinv);
        return 0;
    }

    // Panel-kernel form (float32, ragged n, more block rows than CUs) of the outer panel at c0, on st: per 64-wide block column the left-looking
    // update with the panel's previous block columns, then one launch that factors the diagonal block and solves the rows below.  Waits on ev_ph
    // if pending (never today: only split panels get their head update on the auxiliary stream, and those take the tile form).
    int factor_panel_columns(int64_t c0) {
        int rc = wait_head();
        if (rc) return rc;
        for (int64_t j0 = c0; j0 < panel_end(c0); j0 += NB) {
            const int nb = (int)((j0 + NB < n) ? NB : n - j0);
            if (j0 > c0 && (rc = update(j0, n - j0, j0, nb, c0, j0 - c0, 0, st))) return rc;
            const int64_t below = n - (j0 + nb);
            int* arrived = mxf_flags(h, (unsigned)S);
            if (!arrived) MXF_FAIL(h, -4, "mxf_potrf: cannot allocate the workgroup hand-off counters");
            hipLaunchKernelGGL((potrf_panel_kernel<T>), dim3((unsigned)(1 + (below + 127) / 128), S), dim3(128), 0, st, A, lda, sA, j0, nb, n, info, arrived);
        }
        return 0;
    }

    // Eager inverse, when the panels of row block [rb0, pe) have been factored (fires_at(pe)): the block's pieces of the merge step with a first
    // block of rb0 rows, each queued as soon as ITS inputs exist.  Records ev_pi on st (L down to row pe and the rows below it are final).
    //   potrf_inv_diag: waits ev_pi; the inverse of the diagonal block L[rb0:pe, rb0:pe] (needs the block's own panels only); records ev_pc.
    //   potrf_inv: waits ev_pc; p2 of this block (its p1 was queued one firing earlier); waits ev_pi; p1 of the NEXT block, whose inputs -- the
    //     rows below the panel that just ended and the finished leading inverse -- are complete now, panels before that block is factored.
    // What is left behind the factorisation is the last block's diagonal inverse and p2.  join() brings potrf_inv back to st; potrf_inv_diag's
    // work always ends in an ev_pc that potrf_inv has waited on.
    int eager_row_block(int64_t pe) {
        const int64_t rb0 = row_block_start(pe);
        hipStream_t qd = h->potrf_inv_diag, qp = h->potrf_inv;
        MXF_HIP(h, hipEventRecord(h->ev_pi, st));
        MXF_HIP(h, hipStreamWaitEvent(qd, h->ev_pi, 0));
        int rc = trtri_typed<T>(h, qd, {.dtype = dtype, .n = pe - rb0, .L = {A + rb0 * (lda + 1), lda}, .Linv = {Ie + rb0 * (ldie + 1), ldie}});
        if (rc) return rc;
        MXF_HIP(h, hipEventRecord(h->ev_pc, qd));
        MXF_HIP(h, hipStreamWaitEvent(qp, h->ev_pc, 0));       // (block 0: p1 of block 1 reads this inverse)
        if (rb0 > 0 && (rc = trtri_merge_p2<T>(h, dtype, rb0, pe - rb0, Ie, ldie, 0, 1, true, qp))) return rc;
        if (pe < n) {
            MXF_HIP(h, hipStreamWaitEvent(qp, h->ev_pi, 0));   // the rows below the panel that just ended
            rc = trtri_merge_p1<T>(h, dtype, pe, next_fire(pe) - pe, (const T*)A, lda, 0, Ie, ldie, 0, 1, true, qp);
        }
        return rc;
    }

    // Trailing update after the outer panel [c0, pe), pe < n, lower blocks only: A22 -= L21 L21^T with K = the panel's width.  Waits on ev_pb if
    // pending (the previous rest update touched these columns).  Without look-ahead, or in front of the last panel: one product on st.
    // With look-ahead: the part that touches the NEXT outer panel's columns [pe, pe2) first, so that panel's latency-bound factorisation starts
    // right away, and the rest on potrf_aux next to that factorisation (records ev_pb, sets pend.rest):
    //   next panel not split: its diagonal block and the rows below it on st; ev_pa recorded on st behind them and waited on by potrf_aux (the
    //     rest starts behind the head products, not next to them);
    //   next panel split: only its diagonal block (what its chain launch reads) on st; the rows below it -- read by potrf_rows_kernel only,
    //     0.2 ms later -- on potrf_aux behind ev_pa, recorded on st in FRONT of the diagonal block's product (this panel's columns are final);
    //     records ev_ph, sets pend.head (0.09 ms per panel off the serial path at n = 8192).
    int trailing_update(int64_t c0) {
        const int64_t pe = panel_end(c0), pe2 = panel_end(pe), K = pe - c0;
        int rc = wait_rest();
        if (rc) return rc;
        if (!look || pe2 >= n) return update(pe, n - pe, pe, n - pe, c0, K, 1, st);
        hipStream_t ax = h->potrf_aux;
        const bool head_aux = split(pe);
        if (head_aux) MXF_HIP(h, hipEventRecord(h->ev_pa, st));
        if ((rc = update(pe, pe2 - pe, pe, pe2 - pe, c0, K, 1, st))) return rc;
        if (head_aux) {
            MXF_HIP(h, hipStreamWaitEvent(ax, h->ev_pa, 0));
            if ((rc = update(pe2, n - pe2, pe, pe2 - pe, c0, K, 0, ax))) return rc;
            MXF_HIP(h, hipEventRecord(h->ev_ph, ax));
            pend.head = true;
        } else {
            if ((rc = update(pe2, n - pe2, pe, pe2 - pe, c0, K, 0, st))) return rc;
            MXF_HIP(h, hipEventRecord(h->ev_pa, st));
            MXF_HIP(h, hipStreamWaitEvent(ax, h->ev_pa, 0));
        }
        if ((rc = update(pe2, n - pe2, pe2, n - pe2, c0, K, 1, ax))) return rc;
        MXF_HIP(h, hipEventRecord(h->ev_pb, ax));
        pend.rest = true;
        return 0;
    }

    // st waits for everything the call queued elsewhere: potrf_inv (records ev_pj there) and what is pending of potrf_aux.  (ev_ph is never
    // pending here today: the last panel has no successor.)
    int join() {
        if (eager) {
            MXF_HIP(h, hipEventRecord(h->ev_pj, h->potrf_inv));
            MXF_HIP(h, hipStreamWaitEvent(st, h->ev_pj, 0));
        }
        int rc = wait_rest();
        return rc ? rc : wait_head();
    }
};

// d.Linv.p (float64 only): L^-1 may be formed into it next to the factorisation (PotrfPlan::eager); *d.inv_done tells the caller whether it was
// (else: call trtri afterwards).
template <typename T>
int potrf_typed(mxf_ctx* h, hipStream_t st, const MxfPotrf& d) {
    const int64_t n = d.n;
    T* A = (T*)d.A.p; T* Ie = sizeof(T) == 8 ? (T*)d.Linv.p : nullptr;
    const PotrfPlan plan = potrf_plan(potrf_request(h, sizeof(T), d.S, n, st, Ie != nullptr, d.zero_upper));
    if (plan.refusal) MXF_FAIL(h, -3, "mxf_potrf: %s", plan.refusal);
    if (d.info && d.zero_info) MXF_HIP(h, hipMemsetAsync(d.info, 0, sizeof(int) * d.S, st));
    PotrfCall<T> c{plan, h, d.dtype, A, d.A.ld, d.A.stride, d.info, st, Ie, d.Linv.ld, {}};
    int rc = 0;
    for (int64_t c0 = 0, pe; c0 < n && !rc; c0 = pe) {
        pe = c.panel_end(c0);
        rc = c.panel_tiles ? c.factor_panel_tiles(c0) : c.factor_panel_columns(c0);
        if (!rc && c.eager && c.fires_at(pe)) rc = c.eager_row_block(pe);
        if (!rc && pe < n) rc = c.trailing_update(c0);
    }
    if (!rc) rc = c.join();
    if (rc) return rc;
    if (d.inv_done) *d.inv_done = c.eager;
    // (internal callers that only ever read the lower triangle skip this pass)
    if (n > 1 && d.zero_upper) hipLaunchKernelGGL((zero_upper_kernel<T>), dim3((unsigned)((n + 255) / 256), (unsigned)n, d.S), dim3(256), 0, st, A, n, d.A.ld, d.A.stride);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

// B <- op(L)^-1 B
template <typename T>
int trsm_typed(mxf_ctx* h, hipStream_t st, const MxfTrsm& d) {
    const int64_t n = d.n, nrhs = d.nrhs, ldl = d.L.ld, sL = d.L.stride, ldb = d.B.ld, sB = d.B.stride;
    const T* L = (const T*)d.L.p; T* B = (T*)d.B.p;
    const int dtype = d.dtype, S = d.S;
    const int64_t nblk = (n + NB - 1) / NB;
    if (!d.transpose) {
        for (int64_t kb = 0; kb < nblk; ++kb) {
            const int64_t k0 = kb * NB;
            const int nb = (int)((k0 + NB < n) ? NB : n - k0);
            if (k0 > 0) {
                int rc = mxf_gemm_internal(h, st, {.dtype = dtype, .M = nb, .N = nrhs, .K = k0, .alpha = -1.0, .A = {L + k0 * ldl, ldl, sL}, .B = {B, ldb, sB},
                                                   .beta = 1.0, .C = {B + k0 * ldb, ldb, sB}, .batch = S});
                if (rc) return rc;
            }
            hipLaunchKernelGGL((solve_cols_kernel<T, false>), dim3((unsigned)((nrhs + 255) / 256), S), dim3(256), 0, st, L, ldl, sL, B,
                               ldb, sB, k0, nb, (int64_t)0, nrhs);
        }
    } else {
        for (int64_t kb = nblk - 1; kb >= 0; --kb) {
            const int64_t k0 = kb * NB;
            const int nb = (int)((k0 + NB < n) ? NB : n - k0);
            const int64_t rem = n - (k0 + nb);
            if (rem > 0) {   // B_k -= L[k+1:, k]^T B[k+1:]
                int rc = mxf_gemm_internal(h, st, {.dtype = dtype, .ta = 1, .M = nb, .N = nrhs, .K = rem, .alpha = -1.0, .A = {L + (k0 + nb) * ldl + k0, ldl, sL},
                                                   .B = {B + (k0 + nb) * ldb, ldb, sB}, .beta = 1.0, .C = {B + k0 * ldb, ldb, sB}, .batch = S});
                if (rc) return rc;
            }
            hipLaunchKernelGGL((solve_cols_kernel<T, true>), dim3((unsigned)((nrhs + 255) / 256), S), dim3(256), 0, st, L, ldl, sL, B,
                               ldb, sB, k0, nb, (int64_t)0, nrhs);
        }
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

int mxf_potrf_internal(mxf_ctx* h, hipStream_t st, const MxfPotrf& d) {
    if (d.inv_done) *d.inv_done = false;
    if (d.n <= 0 || d.S <= 0) return 0;
    if (d.dtype == MXF_F32) return potrf_typed<float>(h, st, d);
    if (d.dtype == MXF_F64) return potrf_typed<double>(h, st, d);
    MXF_FAIL(h, -2, "mxf_potrf: bad dtype %d", d.dtype);
}

int mxf_trsm_internal(mxf_ctx* h, hipStream_t st, const MxfTrsm& d) {
    if (d.n <= 0 || d.nrhs <= 0 || d.S <= 0) return 0;
    if (d.dtype == MXF_F32) return trsm_typed<float>(h, st, d);
    if (d.dtype == MXF_F64) return trsm_typed<double>(h, st, d);
    MXF_FAIL(h, -2, "mxf_trsm: bad dtype %d", d.dtype);
}

int mxf_trtri_internal(mxf_ctx* h, hipStream_t st, const MxfTrtri& d) {
    if (d.n <= 0 || d.S <= 0) return 0;
    if (d.dtype == MXF_F32) return trtri_typed<float>(h, st, d);
    if (d.dtype == MXF_F64) return trtri_typed<double>(h, st, d);
    MXF_FAIL(h, -2, "mxf_trtri: bad dtype %d", d.dtype);
}

int mxf_sumlogdiag_internal(mxf_ctx* h, hipStream_t st, const MxfSumLogDiag& d) {
    if (d.S <= 0) return 0;
    if (d.dtype == MXF_F32) hipLaunchKernelGGL((sumlogdiag_kernel<float>), dim3(d.S), dim3(256), 0, st, (const float*)d.L.p, d.n, d.L.ld, d.L.stride, (float*)d.out);
    else if (d.dtype == MXF_F64) hipLaunchKernelGGL((sumlogdiag_kernel<double>), dim3(d.S), dim3(256), 0, st, (const double*)d.L.p, d.n, d.L.ld, d.L.stride, (double*)d.out);
    else MXF_FAIL(h, -2, "mxf_sumlogdiag: bad dtype %d", d.dtype);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

extern "C" int mxf_potrf(mxf_handle h, int dtype, int S, int64_t n, void* A, int64_t lda, int64_t strideS_A, int* info, void* stream) {
    if (!h) return -1;
    if (n < 0 || S < 0 || (n > 0 && (!A || lda < n))) MXF_FAIL(h, -2, "mxf_potrf: bad arguments");
    return mxf_potrf_internal(h, (hipStream_t)stream, {.dtype = dtype, .S = S, .n = n, .A = {A, lda, strideS_A}, .info = info});
}

extern "C" int mxf_trsm(mxf_handle h, int dtype, int transpose, int S, int64_t n, int64_t nrhs, const void* L, int64_t ldl,
                        int64_t strideS_L, void* B, int64_t ldb, int64_t strideS_B, void* stream) {
    if (!h) return -1;
    if (n < 0 || nrhs < 0 || S < 0 || (n > 0 && nrhs > 0 && (!L || !B || ldl < n || ldb < nrhs))) MXF_FAIL(h, -2, "mxf_trsm: bad arguments");
    return mxf_trsm_internal(h, (hipStream_t)stream, {.dtype = dtype, .transpose = transpose, .S = S, .n = n, .nrhs = nrhs, .L = {L, ldl, strideS_L},
                                                      .B = {B, ldb, strideS_B}});
}

extern "C" int mxf_trtri(mxf_handle h, int dtype, int S, int64_t n, const void* L, int64_t ldl, int64_t strideS_L, void* Linv,
                         int64_t ldi, int64_t strideS_I, void* stream) {
    if (!h) return -1;
    if (n < 0 || S < 0 || (n > 0 && (!L || !Linv || ldl < n || ldi < n))) MXF_FAIL(h, -2, "mxf_trtri: bad arguments");
    return mxf_trtri_internal(h, (hipStream_t)stream, {.dtype = dtype, .S = S, .n = n, .L = {L, ldl, strideS_L}, .Linv = {Linv, ldi, strideS_I}});
}

extern "C" int mxf_sumlogdiag(mxf_handle h, int dtype, int S, int64_t n, const void* L, int64_t ldl, int64_t strideS_L, void* out,
                              void* stream) {
    if (!h) return -1;
    if (n < 0 || S < 0 || (n > 0 && (!L || !out))) MXF_FAIL(h, -2, "mxf_sumlogdiag: bad arguments");
    return mxf_sumlogdiag_internal(h, (hipStream_t)stream, {.dtype = dtype, .S = S, .n = n, .L = {L, ldl, strideS_L}, .out = out});
}
