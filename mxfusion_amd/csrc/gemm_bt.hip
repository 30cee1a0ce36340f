// f16x2 split product whose second operand is stored K-MAJOR:  C (M x N) = alpha * A (M x K) * Bt (K x N),  f32-equivalent accuracy
// (two scaled f16 terms per operand and three f16 MFMA products per fragment pair -- hi' lo, lo' hi, hi' hi: gemm_split.hip's format; since r07
// on v_mfma_f32_16x16x32_f16, where gemm_split.hip multiplies with v_mfma_f32_32x32x16_f16: the 32 products of one instruction are summed inside
// the pipe, so the two kernels agree to rounding, not bit for bit).
//
// Why (r06): the SVGP training call (svgp_regression.py:85-90) needs Kuf twice -- as the (m, k = n) operand of Psi2 = Kuf Kuf^T and as the
// (n, k = m) operand of T = H0 Kuf -- and until r05 wrote it twice, 8.6 GB of planes each; the second pass (1.8 ms, HBM-write bound) sat
// between the two products with the matrix pipe idle.  This kernel reads T's second operand from the FIRST set of planes: the planes of
// the (R = K rows, k' = N) operand "Bt", element (k, n) at ((n / 16) * R + k) * 16 + n % 16 -- 16 x 16 tiles [k][n], n minor.  The MFMA
// wants, per lane, eight CONSECUTIVE k of one column n; the tile has them 32 bytes apart.  gfx950's transposing LDS read does the turn:
//   * LDS-DMA (global_load_lds_dwordx4, lane-linear destination, free per-lane source) builds an image of 128-byte chunks [4 k][16 n];
//   * ds_read_b64_tr_b16: within a 16-lane group lane p ADDRESSES row p / 4, columns 4 (p % 4) .. + 3 of a chunk and RECEIVES column p of
//     its four rows -- two reads give the lane its eight k.
// A (shared by the workgroup's eight waves) and Bt both go through LDS, every load an LDS-DMA request, as one stream ACROSS work items.
//
// Why the 16x16x32 shape (r07): on the 32x32x16 shape this kernel was bound by the clock the chip holds under the instruction mix (DESIGN.md
// section 4.2: busy x clock constant over three structures, all-zero operands 18.5 % faster on the same binary).  Same tiles, same request
// stream, same LDS bytes per flop (24 16-byte reads per wave and 32 k) on the K = 32 shape: 10.5 against 11.3 ms on the T shape, same box,
// alternating (profiles/r07_bt_shape_ab.txt).  What the instruction forces:
//   * an MFMA consumes TWO consecutive 16-k blocks (lane = column / row lane % 16, k group lane / 16: lanes 0-31 take the first block,
//     lanes 32-63 the second), so the ring is two PAIR slots of (2 blocks x (A 16 KB + Bt 16 KB)) and a stream position is a pair of blocks;
//   * A image: unit = 2 row + k half, NO swizzle (ds_read_b128 serves lanes {0-3, 12-15, 20-27} | {4-11, 16-19, 28-31} | the same + 32 in one
//     cycle each: with lane = 16 (k half) + row the plain image puts each group on 16 distinct units modulo 16; the XOR of gemm_split.hip's
//     32-row fragments would make it 2-way);
//   * Bt image: chunk c = (n16 block c >> 2, read h = (c >> 1) & 1, k half c & 1) holds k = 8 (c & 1) + 4 h + 0..3: the two chunks of a
//     32-lane half of one ds_read_b64_tr_b16 are neighbours (256 contiguous bytes: conflict free), lanes 32-63 read the same place of
//     the pair's second block;
//   * requests: a pair (8 per thread) goes out in the MIDDLE of a step, behind a barrier that follows the step's last fragment read, into
//     the slot that step is reading -- two slots hold up to two pairs (128 KB) in flight or unread, and a pair has the rest of that step and the
//     whole next one to land (the r06 ring of four 16-k slots: three blocks = 96 KB, three block times).  Two barriers per pair, as before;
//   * an item with an odd number of blocks ends in a PEELED step whose second block is a second request for its last block (nothing past
//     K16 is read, the request count per step stays 8) and whose Bt fragments are zeroed in lanes 32-63: those products add exactly 0.
//
// U (optional, P = 1 of the SVGP call): the row  U[n] = uscale * sum_k w[k] Bt[k][n]  rides on the fragments that are in registers anyway:
// for every column strip ONE of its tm row-tile workgroups (rotating) also forms v_dot2_f32_f16 sums of its Bt fragments with the f16
// hi / lo planes of w (three products, like the MFMAs), its two row halves taking alternate block pairs.  (Until r05 U was a by-product of the
// second planes pass; every other pass over Kuf happens before w exists.)
#include "common.h"
#include "internal.h"
#include "split_device.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));

struct BtArgs {
    const unsigned short* A; const unsigned short* Bt; float* C;
    int64_t M, N, K16;                   // K16 = number of 16-wide k blocks
    int64_t pA, pB, btR;                 // plane strides (elements); rows of the Bt operand (>= 16 K16)
    float alpha;
    int c_blk;                           // C in 16-column blocks: element (row, col) at ((col / 16) * M + row) * 16 + col % 16
    int64_t ldc;
    int64_t tm, tn, nwg;
    const float* ad0;                    // alpha *= ad0[0] (device scalar: the kernel variance of Gram planes)
    const unsigned* maxbits;             // alpha /= scale_from_maxbits(maxbits[0]) (the power-of-two scale of the A planes)
    const unsigned* maxbits2;            // the same for the Bt planes (nullptr: Gram planes, whose scale is known: alpha / ad0 carry it)
    unsigned* maxout;                    // atomicMax of the bit pattern of max |C| (nullptr: none)
    unsigned* sync; int sync_n;          // rendezvous of the tm row tiles of a column strip (split_device.h: wg_rendezvous)
    int sync_every;                      // ... in every sync_every-th persistent round only: bounds the drift of the tiles that share a strip's lines in L2
    // U row: w as two f16 planes [2][16 K16] (hi, lo of w * scale_from_maxbits(uwmax[0])), U[n] = uscale * ad0[0] / that scale * sum
    const unsigned short* uw; const unsigned* uwmax; float* uout; float uscale;
};

// one LDS-DMA request: 64 lanes x 16 bytes from per-lane global addresses to the 1 KB at LDS byte address `lds` (wave-uniform, in M0)
// (wave-uniform 64-bit base in SGPRs + a 32-bit per-lane byte offset: two address registers per thread for the whole kernel)
__device__ __forceinline__ void bt_dma16(const void* sbase, unsigned voff, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds) : "memory", "m0");
}

// acc + sum of the eight f16 products of two 16-byte fragments (four v_dot2_f32_f16)
__device__ __forceinline__ float bt_dot8(u32x4 a, u32x4 b, float acc) {
    const f16x8 av = __builtin_bit_cast(f16x8, a), bv = __builtin_bit_cast(f16x8, b);
    acc = __builtin_amdgcn_fdot2(f16x2{av[0], av[1]}, f16x2{bv[0], bv[1]}, acc, false);
    acc = __builtin_amdgcn_fdot2(f16x2{av[2], av[3]}, f16x2{bv[2], bv[3]}, acc, false);
    acc = __builtin_amdgcn_fdot2(f16x2{av[4], av[5]}, f16x2{bv[4], bv[5]}, acc, false);
    acc = __builtin_amdgcn_fdot2(f16x2{av[6], av[7]}, f16x2{bv[6], bv[7]}, acc, false);
    return acc;
}

constexpr int BT_KMAX16 = 128;           // U row: w planes of up to 2048 k live in LDS

// 256 x 256 tile, 512 threads: wave = 4 h + w owns rows [128 h, + 128) x columns [64 w, + 64) = 8 x 4 MFMA tiles of 16 x 16 (128 accumulators).
template <bool WU>
__global__ __launch_bounds__(512, 2) void gemm_f16x2_bt_kernel(BtArgs g) {
    constexpr int NU = 512;                          // 16-byte units of one plane's (256 x 16) slab
    __shared__ u32x4 sA[2][2][2][NU];                // [pair slot][block of the pair][plane][unit]: A rows, unit = 2 row + k half
    __shared__ u32x4 sB[2][2][2][NU];                // Bt: chunk c = (nb * 2 + h) * 2 + k half of 128 bytes [4 k][16 n]
    __shared__ u32x4 sW[WU ? 2 * BT_KMAX16 * 2 : 1]; // w planes [plane][16 K16 halves], zero up to a whole pair
    __shared__ float sU[WU ? 512 : 1];               // the two row halves' shares of U for the item's 256 columns
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave & 3, wh = wave >> 2;
    const int lj = lane & 15, lg = lane >> 4;        // row / column inside a 16 x 16 tile; k group (8 k) of the pair's 32
    int patience = 2;
    float cmax = 0.f;
    if constexpr (WU) {
        if (g.uout) {
            const int nunits = (int)(g.K16 * 2), npad = (nunits + 3) & ~3;          // 16-byte units per plane; a tail step reads units of the missing block
            for (int i = tid; i < 2 * npad; i += 512) {
                const int p = i / npad, u = i % npad;
                sW[p * (BT_KMAX16 * 2) + u] = u < nunits ? *reinterpret_cast<const u32x4*>(g.uw + (int64_t)p * g.K16 * 16 + u * 8) : u32x4{0u, 0u, 0u, 0u};
            }
        }
        __syncthreads();
    }
    float alpha = g.alpha;
    if (g.ad0) alpha *= g.ad0[0];
    if (g.maxbits) alpha /= scale_from_maxbits(g.maxbits[0]);
    if (g.maxbits2) alpha /= scale_from_maxbits(g.maxbits2[0]);

    // A: thread t fills unit t of each plane's slab = bytes [16 t, + 16) of the block's 8 KB in memory (row t >> 1, k half t & 1)
    // Bt: thread t fills unit t = 8 c + s of the image: chunk c, piece s = (row j = s >> 1 of the chunk, n half s & 1)
    const int bc = tid >> 3, bs = tid & 7;
    const int b_nb = bc >> 2;                                                     // n16 block inside the strip
    const int b_kl = 8 * (bc & 1) + 4 * ((bc >> 1) & 1) + (bs >> 1);              // k inside the block: 8 (k half) + 4 h + j
    const unsigned voff_b = (unsigned)((((int64_t)b_nb * g.btR + b_kl) * 16 + 8 * (bs & 1)) * 2);      // bytes (host checks 16 btR * 32 < 2^31)
    const unsigned voff_a = (unsigned)(tid * 16);
    // fragment reads, relative to a pair slot's plane 0: A unit of tile x = 0 (tile x: + 32 units, plane 1: + NU, lanes 32-63: the second block);
    // Bt byte offset of this lane (instruction (t, h) adds 512 t + 256 h; ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group addresses row q,
    // columns 4 p .. + 3 of its chunk)
    const int ua0_ = (128 * wh + lj) * 2 + (lg & 1) + (lg >> 1) * (2 * NU);
    const unsigned ldsA = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)&sA[0][0][0][wave * 64]);
    const unsigned ldsB = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) void*)&sB[0][0][0][wave * 64]);
    const unsigned toff_blk = (unsigned)((((int64_t)(4 * wq) * g.M + 128 * wh + lj) * 16 + 4 * lg) * 4);      // bytes (host: 16 M * 64 < 2^31)
    const int rb_h = (wq * 2048 + (lg >> 1) * 16384 + (lg & 1) * 128 + (lj >> 2) * 32 + (lj & 3) * 8) / 2;      // in halves

    // One STREAM of block pairs over all of this workgroup's items (blockIdx.x, + gridDim.x, ...): the requests run ahead of the multiplies
    // ACROSS item boundaries, so an item's first pairs arrive under the previous item's last multiplies and its epilogue -- a per-item
    // pipeline fill (two memory latencies with nothing in flight, ~3 % of a K = 1024 item) never happens.  Slot = stream position modulo 2.
    // (32-bit index arithmetic throughout: the 64-bit divisions of a first form expanded to branchy software routines in the per-item paths,
    //  with spill reloads whose compiler-inserted s_waitcnt vmcnt(0) drained the request stream once per item)
    const int nk = (int)g.K16, np = (nk + 1) / 2;
    const unsigned nwg = (unsigned)g.nwg, tmu = (unsigned)g.tm;
    const int nit = (int)((nwg - blockIdx.x + gridDim.x - 1) / gridDim.x);
    const int nsteps = nit * np;
    const unsigned q8 = nwg / 8, r8 = nwg % 8;
    auto item_of = [&](int i) -> unsigned { return xcd_run_item(blockIdx.x + (unsigned)i * gridDim.x, q8, r8); };
    int q_it = 0, q_p = 0;
    unsigned q_slot = 0;
    const unsigned short* qa = nullptr;
    const unsigned short* qb = nullptr;
    auto q_enter = [&]() {
        const unsigned wid = item_of(q_it);
        const unsigned tn_ = wid / tmu, tm_ = wid - tn_ * tmu;
        qa = g.A + (int64_t)tm_ * 256 * 16;
        qb = g.Bt + ((int64_t)tn_ * 16) * g.btR * 16;
    };
    // one pair: EIGHT requests per thread, always (an odd item's last pair asks for its one block twice)
    // (inline asm, not __builtin_amdgcn_global_load_lds: with the builtin the compiler tracks the LDS-DMA writes itself and puts an
    //  s_waitcnt vmcnt(0) in front of the fragment reads at the loop header -- it cannot see the counted waits below --, i.e. one full
    //  memory latency per trip with nothing in flight)
    auto q_issue = [&]() {
        const int kb0 = 2 * q_p, kb1 = kb0 + 1 < nk ? kb0 + 1 : kb0;
        const unsigned la = ldsA + q_slot * 32768, lb = ldsB + q_slot * 32768;
        bt_dma16(qa + (int64_t)kb0 * g.M * 16, voff_a, la);
        bt_dma16(qa + g.pA + (int64_t)kb0 * g.M * 16, voff_a, la + 8192);
        bt_dma16(qb + (int64_t)kb0 * 256, voff_b, lb);
        bt_dma16(qb + g.pB + (int64_t)kb0 * 256, voff_b, lb + 8192);
        bt_dma16(qa + (int64_t)kb1 * g.M * 16, voff_a, la + 16384);
        bt_dma16(qa + g.pA + (int64_t)kb1 * g.M * 16, voff_a, la + 16384 + 8192);
        bt_dma16(qb + (int64_t)kb1 * 256, voff_b, lb + 16384);
        bt_dma16(qb + g.pB + (int64_t)kb1 * 256, voff_b, lb + 16384 + 8192);
        q_slot ^= 1;
        if (++q_p == np) { q_p = 0; ++q_it; if (q_it < nit) q_enter(); }
    };
    // this wave's share of everything but the youngest NSTR requests has landed; the barrier extends it to the workgroup.  (vmcnt retires in
    // order and counts the epilogue's stores too: a wait behind an epilogue also drains that item's stores -- conservative.)
#define BT_WAIT(NSTR) do { asm volatile("s_waitcnt vmcnt(" NSTR ")" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)
#define HF(v) __builtin_bit_cast(f16x8, v)
#define BT_TR(ptr) __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ptr)))
    f32x4 c[8][4];
    float ua[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t m0 = 0, n0 = 0;
    unsigned c_slot = 0;
    bool uitem = false;
    u32x4 fb[4][2];
#define BT_A(x, p) sa_[(p) * NU + ua0_ + 32 * (x)]
#define BT_MM(x, AH, AL)                                                                                                           \
    do {                                                                                                                            \
        _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                                             \
            c[x][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(HF(fb[t][0]), HF(AL), c[x][t], 0, 0, 0);          /* hi' lo */         \
            c[x][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(HF(fb[t][1]), HF(AH), c[x][t], 0, 0, 0);          /* lo' hi */         \
            c[x][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(HF(fb[t][0]), HF(AH), c[x][t], 0, 0, 0);          /* hi' hi */         \
        }                                                                                                                           \
        __builtin_amdgcn_sched_barrier(0);           /* (pins the order: the scheduler otherwise hoists every read to the top) */    \
    } while (0)
    // One stream position = pair c_p of the current item, in slot c_slot.  On entry the pair has landed (workgroup-wide) and pair s_ + 1 is
    // requested; TAIL: the item's last, single block.
#define BT_STEP(TAIL)                                                                                                              \
    do {                                                                                                                            \
        const u32x4* const sa_ = &sA[c_slot][0][0][0];                                                                              \
        _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                                             \
            const unsigned short* sb_ = reinterpret_cast<const unsigned short*>(&sB[c_slot][0][p][0]) + rb_h;                       \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                                         \
                const u32x2 v0_ = BT_TR(sb_ + t * 256), v1_ = BT_TR(sb_ + t * 256 + 128);                                           \
                fb[t][p] = u32x4{v0_[0], v0_[1], v1_[0], v1_[1]};                                                                   \
                if (TAIL) fb[t][p] &= kmask;         /* lanes 32-63 hold the copy of the last block: their products must add 0 */   \
            }                                                                                                                       \
        }                                                                                                                           \
        u32x4 a0h = BT_A(0, 0), a0l = BT_A(0, 1), a1h = BT_A(1, 0), a1l = BT_A(1, 1);                                           \
        if constexpr (WU) {                                                                                                         \
            if (uitem && ((c_p & 1) == wh)) {        /* wave-uniform; FIRST: few registers are live here */                         \
                const u32x4 wh_ = sW[4 * c_p + lg], wl_ = sW[BT_KMAX16 * 2 + 4 * c_p + lg];                                         \
                _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                                     \
                    ua[t] = bt_dot8(fb[t][1], wh_, ua[t]); ua[t] = bt_dot8(fb[t][0], wl_, ua[t]); ua[t] = bt_dot8(fb[t][0], wh_, ua[t]); \
                }                                                                                                                   \
            }                                                                                                                       \
        }                                                                                                                           \
        /* the A fragments are requested two multiplies ahead of their use */                                                       \
        u32x4 a2h = BT_A(2, 0), a2l = BT_A(2, 1);                                                                                 \
        BT_MM(0, a0h, a0l);                                                                                                        \
        u32x4 a3h = BT_A(3, 0), a3l = BT_A(3, 1);                                                                                 \
        BT_MM(1, a1h, a1l);                                                                                                        \
        u32x4 a4h = BT_A(4, 0), a4l = BT_A(4, 1);                                                                                 \
        BT_MM(2, a2h, a2l);                                                                                                        \
        u32x4 a5h = BT_A(5, 0), a5l = BT_A(5, 1);                                                                                 \
        BT_MM(3, a3h, a3l);                                                                                                        \
        u32x4 a6h = BT_A(6, 0), a6l = BT_A(6, 1);                                                                                 \
        BT_MM(4, a4h, a4l);                                                                                                        \
        u32x4 a7h = BT_A(7, 0), a7l = BT_A(7, 1);                                                                                 \
        BT_MM(5, a5h, a5l);                                                                                                        \
        /* every fragment of this pair is read: once all eight waves' reads have returned, its slot takes pair s_ + 2 */             \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                          \
        __builtin_amdgcn_s_barrier();                                                                                               \
        asm volatile("" ::: "memory");                                                                                              \
        const bool more = s_ + 2 < nsteps;                                                                                          \
        if (more) q_issue();                                                                                                        \
        asm volatile("" ::: "memory");                                                                                              \
        BT_MM(6, a6h, a6l);                                                                                                        \
        BT_MM(7, a7h, a7l);                                                                                                        \
        /* pair s_ + 1 (requested in the middle of step s_ - 1, or in the prologue) must have landed.  Outstanding per thread, oldest first: \
           its 8 requests, the 32 stores of an epilogue that ran since (conservative: they are waited for too), the 8 requests of pair     \
           s_ + 2 if this step made them: all but the youngest 8, or all.  (Behind the last step nothing is outstanding but stores.) */    \
        if (more) BT_WAIT("8"); else BT_WAIT("0");                                                                                  \
        c_slot ^= 1; ++c_p; ++s_;                                                                                                   \
    } while (0)
    auto finish_item = [&]() {
        if constexpr (WU) {
            if (uitem) {          // workgroup-uniform
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    ua[t] += __shfl_xor(ua[t], 16, 64);      // the four k groups of the fragment
                    ua[t] += __shfl_xor(ua[t], 32, 64);
                    if (lane < 16) sU[256 * wh + 64 * wq + 16 * t + lj] = ua[t];
                }
                __syncthreads();
                if (tid < 256) {
                    float sc = g.uscale * (g.ad0 ? g.ad0[0] : 1.f) / scale_from_maxbits(g.uwmax[0]);
                    if (g.maxbits2) sc /= scale_from_maxbits(g.maxbits2[0]);
                    g.uout[n0 + tid] = (sU[tid] + sU[256 + tid]) * sc;
                }
            }
        }
        // D = Bt^T A^T: accumulator register r of tile (x, t) is C[m0 + 128 wh + 16 x + lj][n0 + 64 wq + 16 t + 4 lg + r]
        if (g.c_blk) {
            // blocked layout, element (row, col) at ((col / 16) * M + row) * 16 + col % 16: a 16 x 16 tile of C is one contiguous KB, the wave's
            // 64 stores of 16 bytes cover it; one 32-bit per-thread byte offset (toff_blk) + a wave-uniform base per (x, t)
            char* const cb = reinterpret_cast<char*>(g.C) + ((n0 >> 4) * g.M + m0) * 64;
#pragma unroll
            for (int x = 0; x < 8; ++x)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    char* const sb = cb + ((int64_t)t * g.M + 16 * x) * 64;      // wave-uniform
                    const f32x4 v = {alpha * c[x][t][0], alpha * c[x][t][1], alpha * c[x][t][2], alpha * c[x][t][3]};
                    *reinterpret_cast<f32x4*>(sb + toff_blk) = v;
                    if (g.maxout) cmax = fmaxf(fmaxf(cmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
                }
        } else {
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int64_t row = m0 + 128 * wh + 16 * x + lj;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int64_t col = n0 + 64 * wq + 16 * t + 4 * lg;
                    float* p = g.C + row * g.ldc + col;
                    const f32x4 v = {alpha * c[x][t][0], alpha * c[x][t][1], alpha * c[x][t][2], alpha * c[x][t][3]};
                    *reinterpret_cast<f32x4*>(p) = v;
                    if (g.maxout) cmax = fmaxf(fmaxf(cmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
                }
            }
        }
    };
    const unsigned kmask = lane < 32 ? ~0u : 0u;
    if (nsteps > 0) {
        q_enter();
        q_issue();
        // pair 0 landed: all but the 8 requests of pair 1, if there is one (K >= 48: every item has at least two pairs)
        if (nsteps > 1) { q_issue(); BT_WAIT("8"); } else BT_WAIT("0");
    }
    int s_ = 0;
    for (int c_it = 0; c_it < nit; ++c_it) {
        {                                            // a new item (workgroup-uniform)
            const unsigned wid = item_of(c_it);
            const unsigned tile_n = wid / tmu, tile_m = wid - tile_n * tmu;
            m0 = (int64_t)tile_m * 256; n0 = (int64_t)tile_n * 256;
            uitem = WU && g.uout != nullptr && ((tile_n + (tile_n >> 3) + (tile_n >> 6)) % tmu) == tile_m;
            if (g.sync && (c_it % g.sync_every) == 0) wg_rendezvous(g.sync + wid / g.sync_n, (unsigned)g.sync_n, patience);
#pragma unroll
            for (int x = 0; x < 8; ++x)
#pragma unroll
                for (int t = 0; t < 4; ++t) c[x][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 4; ++t) ua[t] = 0.f;
        }
        int c_p = 0;
        while (c_p < nk / 2) BT_STEP(false);
        if (nk & 1) BT_STEP(true);                  // the peeled tail: no branch sits in the steady-state loop
        finish_item();
    }
#undef BT_STEP
#undef BT_MM
#undef BT_A
#undef BT_TR
#undef HF
#undef BT_WAIT
    if (g.maxout) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, o, 64));
        if (lane == 0 && __builtin_bit_cast(unsigned, cmax) > *(volatile unsigned*)g.maxout) atomicMax(g.maxout, __builtin_bit_cast(unsigned, cmax));
    }
}

// w (K floats) -> two f16 planes of w * scale (scale from max |w|, which is also written to maxword); one workgroup
__global__ __launch_bounds__(256) void bt_wsplit_kernel(int64_t K, int64_t Kp, const float* __restrict__ w, unsigned short* __restrict__ planes,
                                                        unsigned* __restrict__ maxword) {
    __shared__ unsigned wm[4];
    unsigned m = 0;
    for (int64_t i = threadIdx.x; i < K; i += 256) { const unsigned b = __builtin_bit_cast(unsigned, w[i]) & 0x7fffffffu; m = b > m ? b : m; }
    for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    for (int i = 0; i < 4; ++i) m = wm[i] > m ? wm[i] : m;
    if (threadIdx.x == 0) maxword[0] = m;
    const float sc = scale_from_maxbits(m);
    for (int64_t i = threadIdx.x; i < Kp; i += 256) {
        const float x = i < K ? w[i] * sc : 0.f;
        const _Float16 fh = (_Float16)x;
        const _Float16 fl = (_Float16)(x - (float)fh);
        planes[i] = __builtin_bit_cast(unsigned short, fh);
        planes[Kp + i] = __builtin_bit_cast(unsigned short, fl);
    }
}

}  // namespace

bool mxf_gemm_bt_ok(int64_t M, int64_t N, int64_t K) { return gemm_bt_shape_ok(M, N, K); }

// C (M x N) = alpha * ad0[0] / scale(maxbits) * A (M x K) * Bt (K x N) from f16x2 planes: A planes as in gemm_split.hip ((m, k): ((k / 16) * M
// + m) * 16 + k % 16), Bt = the planes of the (btR >= K rows, k' = N) operand ((n / 16) * btR + k) * 16 + n % 16.  out.blocked: C in 16-column
// blocks (ldc == N).  u: w (K floats, device) + U (N floats), U[n] = uscale * ad0[0] * sum_k w[k] Bt[k][n] (Bt in the planes' units).
// sched.reserve_cus: workgroups = 256 - reserve_cus (one per CU).
namespace {

// What bt_plan decides (no HIP call) and bt_launch carries out; g.sync is the one field bt_launch fills.  The kernel relies on:
// M, N multiples of 256, K a multiple of 16 and >= 48 (every item has at least two block pairs), btR >= K, 32-bit byte offsets inside one k block of Bt
// and one 16-column block of C, C 16-byte aligned with ldc % 4 == 0; uout != nullptr => the <true> instantiation, K <= 16 BT_KMAX16;
// ncounters > 0 => a group is g.sync_n = tm consecutive items of one XCD's run taken in the same persistent round (strip_rendezvous_ok).
struct BtPlan { BtArgs g; unsigned grid; unsigned ncounters; const float* w; unsigned short* wplanes; unsigned* wmax; };      // w*: the U row's bt_wsplit_kernel launch

int bt_plan(mxf_ctx* h, int64_t M, int64_t N, int64_t K, const MxfSplitScale& sc, const MxfPlanes& A, const MxfPlanes& Bt, int64_t btR,
            const MxfSplitOut& o, const MxfBtURow& u, const MxfSplitSched& sched, BtPlan& p) {
    if (o.planes || o.planes_t || o.avec || o.a_lower || o.lower_only || o.beta != 0.0 || sc.pow0 < 0 || sc.pow0 > 1)
        MXF_FAIL(h, -2, "mxf_gemm_bt: the output is C or blocked C of a full product with beta == 0, and ad0 enters once");
    if (o.blocked && M * 16 * 64 >= (1ll << 31)) MXF_FAIL(h, -3, "mxf_gemm_bt: too many rows for the blocked output");
    if (btR * 16 * 32 >= (1ll << 31)) MXF_FAIL(h, -3, "mxf_gemm_bt: the K-major operand has too many rows");
    if (!mxf_gemm_bt_ok(M, N, K) || btR < K) MXF_FAIL(h, -2, "mxf_gemm_bt: needs M %% 256 == 0, N %% 256 == 0, K %% 16 == 0, K >= 48");
    if (o.blocked && o.ldc != N) MXF_FAIL(h, -2, "mxf_gemm_bt: the blocked output layout needs ldc == N");
    if ((o.ldc % 4) != 0 || (((uintptr_t)o.C) % 16) != 0) MXF_FAIL(h, -2, "mxf_gemm_bt: C must be 16-byte aligned with ldc %% 4 == 0");
    if (u.U && (!u.w || !u.wscratch || K / 16 > BT_KMAX16)) MXF_FAIL(h, -2, "mxf_gemm_bt: the U row needs w, scratch and K <= %d", BT_KMAX16 * 16);
    BtArgs& g = p.g;
    memset(&g, 0, sizeof(g));
    g.A = A.p; g.pA = A.stride; g.maxbits = A.maxbits; g.Bt = Bt.p; g.pB = Bt.stride; g.maxbits2 = Bt.maxbits; g.btR = btR;
    g.M = M; g.N = N; g.K16 = K / 16; g.tm = M / 256; g.tn = N / 256; g.nwg = g.tm * g.tn;
    g.alpha = (float)sc.alpha; g.ad0 = sc.pow0 ? sc.ad0 : nullptr;
    g.C = o.C; g.ldc = o.ldc; g.c_blk = o.blocked; g.maxout = o.maxout;
    p.w = u.w; p.wplanes = nullptr; p.wmax = nullptr;
    if (u.U) {          // caller's scratch: the two f16 planes of w (2 K halves), then its max-abs word
        p.wplanes = (unsigned short*)u.wscratch; p.wmax = (unsigned*)(p.wplanes + 2 * K);
        g.uw = p.wplanes; g.uwmax = p.wmax; g.uout = u.U; g.uscale = (float)u.uscale;
    }
    int64_t grid = (int64_t)(256 - (sched.reserve_cus > 0 ? sched.reserve_cus : 0)) / 8 * 8;
    if (grid < 8) grid = 8;
    if (g.nwg <= grid) grid = g.nwg;
    p.grid = (unsigned)grid;
    // The tm row tiles of a column strip share the strip's Bt lines in their XCD's L2 -- as long as they run in step.  Nothing keeps them
    // there: with no pacing at all they drift apart and every one fetches the strip from HBM itself (r06 PMC: 50 GB of traffic per launch
    // against 26 GB of operands + output).  A bounded rendezvous (wg_rendezvous) at the start of an item re-aligns them.  Same box, T shape, traffic per
    // launch | 32-sample step: never 49.9 GB | 22.04-22.09 ms; every item 23.1 GB | 22.31; every 4th round 32.1 GB | 22.07; 8th 33.0 | 22.02-22.06;
    // 16th 34.1 | 22.06 (tests/probes/r06_bt_sync.sh).  Every fourth round: two thirds of the avoidable traffic gone at no cost in time.
    // (MXF_BT_SYNC = rounds between two rendezvous, 0 = never; probe builds.)
    static const int sync_env = (int)MXF_KNOB("MXF_BT_SYNC", 4);
    p.ncounters = 0;
    if (sync_env && strip_rendezvous_ok(g.tm, g.nwg, grid)) {
        p.ncounters = (unsigned)(g.nwg / g.tm);
        g.sync_n = (int)g.tm; g.sync_every = sync_env > 0 ? sync_env : 1;
    }
    return 0;
}

int bt_launch(mxf_ctx* h, hipStream_t st, BtPlan& p) {
    BtArgs& g = p.g;
    if (g.uout) hipLaunchKernelGGL(bt_wsplit_kernel, dim3(1), dim3(256), 0, st, g.K16 * 16, g.K16 * 16, p.w, p.wplanes, p.wmax);
    if (p.ncounters) g.sync = mxf_gsync(h, p.ncounters);       // (nullptr: the kernel goes without the rendezvous)
    if (g.uout) hipLaunchKernelGGL((gemm_f16x2_bt_kernel<true>), dim3(p.grid), dim3(512), 0, st, g);
    else hipLaunchKernelGGL((gemm_f16x2_bt_kernel<false>), dim3(p.grid), dim3(512), 0, st, g);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

int mxf_gemm_bt_internal(mxf_ctx* h, hipStream_t st, int64_t M, int64_t N, int64_t K, MxfSplitScale scale, MxfPlanes A, MxfPlanes Bt, int64_t btR,
                         MxfSplitOut out, MxfBtURow u, MxfSplitSched sched) {
    BtPlan p;
    const int rc = bt_plan(h, M, N, K, scale, A, Bt, btR, out, u, sched, p);
    return rc ? rc : bt_launch(h, st, p);
}

// C ABI: C (M x N) = alpha * A (M x K) * Bt (K x N) from split operands -- A_planes = mxf_f16x2_split of A (M x K), Bt_planes = mxf_f16x2_split
// of the (K x N) matrix Bt ITSELF (its rows are the contraction index: no transposed copy of it is ever made).  blocked: C in 16-column
// blocks (mxf_gemm_f16x2_planes' lower_only = 2 layout).  w (K floats) and U (N floats), both or neither: U[n] = sum_k w[k] Bt[k][n].
extern "C" int mxf_gemm_f16x2_planes_kmajor(mxf_handle h, int64_t M, int64_t N, int64_t K, double alpha, const void* A_planes, const void* A_maxword,
                                            const void* Bt_planes, const void* Bt_maxword, void* C, int blocked, const void* w, void* U, void* stream) {
    if (!h) return -1;
    if (!A_planes || !Bt_planes || !A_maxword || !Bt_maxword || !C || ((w == nullptr) != (U == nullptr))) MXF_FAIL(h, -2, "mxf_gemm_f16x2_planes_kmajor: bad argument");
    if (!mxf_gemm_bt_ok(M, N, K)) MXF_FAIL(h, -3, "mxf_gemm_f16x2_planes_kmajor: needs M %% 256 == 0, N %% 256 == 0, K %% 16 == 0, K >= 48");
    void* ws = nullptr;
    if (U) {
        ws = mxf_ws(h, mxf_align((2 * (size_t)K + 8) * 2));
        if (!ws) MXF_FAIL(h, -4, "mxf_gemm_f16x2_planes_kmajor: cannot allocate scratch");
    }
    return mxf_gemm_bt_internal(h, (hipStream_t)stream, M, N, K, {.alpha = alpha},
                                {(const unsigned short*)A_planes, (int64_t)mxf_split_plane_elems(M, K), (const unsigned*)A_maxword},
                                {(const unsigned short*)Bt_planes, (int64_t)mxf_split_plane_elems(K, N), (const unsigned*)Bt_maxword}, K,
                                {.C = (float*)C, .ldc = N, .blocked = blocked ? 1 : 0}, {.w = (const float*)w, .U = (float*)U, .wscratch = ws});
}
