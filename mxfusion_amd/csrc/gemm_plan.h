// Kernel choice, tile grid and split-K of the dense GEMM (gemm.hip) as a pure function of the problem: plain C++, no HIP, checked on the
// host by tests/host/gemm_plan_check.cpp.  The launcher passes the probe-build knob in.  The tile sizes below are the kernels' own.
#pragma once
#include <stddef.h>
#include <stdint.h>

// what the caller vouches for about op(A): upper triangular (A^T of a lower-triangular A) / lower triangular (A itself, not transposed)
#define MXF_TRI_NONE 0
#define MXF_TRI_UPPER 1
#define MXF_TRI_LOWER 2

#ifndef MXF_GEMM_BK
#define MXF_GEMM_BK 32
#endif
#ifndef MXF_GEMM_WAVES
#define MXF_GEMM_WAVES 8
#endif
namespace mxf_gemm_tiles {
constexpr int BM = 128, BN = 128, BK = MXF_GEMM_BK;     // generic and LDS-DMA kernels: block tile; BK: the generic kernel's k tile
constexpr int NWAVE = MXF_GEMM_WAVES;                   // 4: 2x2 waves of 64x64;  8: 2x4 waves of 64x32 (half the accumulators -> 4 waves/SIMD)
constexpr int DBK = 16;                                 // LDS-DMA kernel: k tile
constexpr int SBM_ = 64, SBK_ = 16;                     // small-tile float64 kernel: block tile (square) and k tile
}  // namespace mxf_gemm_tiles

// The split GEMMs (gemm_split.hip, gemm_bt.hip): elements of ONE plane of an (R x K) operand, and the shapes the K-major product takes
// (whole 256 x 256 output tiles, k in steps of 16 and at least three of them)
inline size_t split_plane_elems(int64_t R, int64_t K) { return (size_t)((K + 15) / 16) * (size_t)R * 16; }
inline bool gemm_bt_shape_ok(int64_t M, int64_t N, int64_t K) { return M > 0 && N > 0 && K >= 48 && (M % 256) == 0 && (N % 256) == 0 && (K % 16) == 0; }

enum { MXF_GEMM_SMALL_F64 = 0, MXF_GEMM_DMA_F64 = 1, MXF_GEMM_GENERIC = 2 };
struct GemmPlan {
    const char* refusal = nullptr; int rc = 0;     // why the launcher cannot take this shape, and its error code (nothing below is valid then)
    int kernel = MXF_GEMM_GENERIC;
    int64_t tm = 0, tn = 0, ntiles = 0;            // tile grid; tiles per (batch, split)
    int splitk = 1; int64_t kchunk = 0; int atomic = 0;
    int64_t nwg = 0;                               // total workgroups
    int64_t xc_max = 0;                            // > 0: balanced triangular mapping, 8 * xc_max workgroups per batch entry
    int rev_m = 0;
    bool prescale = false;                         // C *= beta in a launch of its own ahead of the atomic epilogue
};

// the triangular hint counts only in the orientation it describes
inline int gemm_tri_normalise(int tri, int ta) { return (tri == MXF_TRI_UPPER && ta) ? MXF_TRI_UPPER : ((tri == MXF_TRI_LOWER && !ta) ? MXF_TRI_LOWER : MXF_TRI_NONE); }

// Split K when the output grid cannot fill `slots` resident workgroups and K is long: pick the split so that the grid is (just under) a whole
// number of rounds -- 576 workgroups on 512 slots would run a half-empty second round (measured: Psi2 33 ms -> 19 ms with 504).
struct GemmSplitRule {
    int64_t slots, tile_k, min_k, k_per_split;     // resident workgroups; the kernel's k tile; shortest K that splits; least K per split
    bool two_rounds;                               // one round would leave >25% of the slots idle: use two
};
inline void gemm_split_k(int64_t tiles, int64_t K, int tri, const GemmSplitRule& r, int& splitk, int64_t& kchunk) {
    int64_t sk = 1;
    if (tiles < r.slots && K >= r.min_k && !tri) {
        const int64_t maxsplit = K / r.k_per_split > 0 ? K / r.k_per_split : 1;     // small latency-bound GEMMs of the (M x M) core split too
        sk = r.slots / tiles;
        if (r.two_rounds && sk * tiles < (r.slots * 3) / 4) sk = (2 * r.slots) / tiles;
        if (sk > maxsplit) sk = maxsplit;
        if (sk < 1) sk = 1;
    }
    kchunk = r.tile_k;
    if (K > 0) {
        kchunk = (K + sk - 1) / sk;
        kchunk = (kchunk + r.tile_k - 1) / r.tile_k * r.tile_k;
        sk = (K + kchunk - 1) / kchunk;
    } else {
        sk = 1;      // empty contraction: C = beta C
    }
    splitk = (int)sk;
}

// tri: normalised (gemm_tri_normalise); vecA / vecB: the operand passed the 16-byte check; small_kmax: MXF_GEMM_SMALL_KMAX
inline GemmPlan gemm_plan(size_t elem_size, int64_t M, int64_t N, int64_t K, int batch, int lower_only, int reserve_cus, int tri, bool vecA, bool vecB,
                          double beta, int64_t small_kmax) {
    using namespace mxf_gemm_tiles;
    GemmPlan p;
    auto grid = [&](int64_t bm) {
        p.tm = (M + bm - 1) / bm; p.tn = (N + bm - 1) / bm;
        p.ntiles = lower_only ? p.tm * (p.tm + 1) / 2 : p.tm * p.tn;      // EXACT count (an estimate of 32 for 36 tiles cost 35 %)
    };
    auto split = [&](const GemmSplitRule& r) {
        gemm_split_k(p.ntiles * batch, K, tri, r, p.splitk, p.kchunk);
        p.atomic = p.splitk > 1;
        p.nwg = p.ntiles * batch * p.splitk;
        p.prescale = p.atomic && beta != 1.0;     // beta == 1 (the potrf / trsm updates): C is accumulated into as is, nothing to pre-scale
    };
    // latency-bound float64 products of the (M x M) core: small-tile variant
    const int64_t t128 = ((M + 127) / 128) * ((N + 127) / 128) * batch;
    bool small = elem_size == 8 && t128 <= 64 && M <= 65535;       // beyond that the big kernel fills at least a quarter of the chip: keep it
    // r06: a LONG contraction over a small output (the float64 step's Psi2 = Kuf Kuf^T: 1024 x 1024 x 2.1 M) is throughput-bound, not
    // latency-bound -- it belongs on the 128 x 128 LDS-DMA kernel with split-K (probe knob MXF_GEMM_SMALL_KMAX: contraction length above
    // which the small-tile kernel steps aside)
    if (K > small_kmax && !tri && M >= 512 && N >= 512) small = false;      // (skinny outputs -- K^T y, M x P -- stay: the 128 x 128 tiles would idle)
    if (small) {
        grid(SBM_);
        if (lower_only && p.tm != p.tn) small = false;
    }
    if (small) {
        p.kernel = MXF_GEMM_SMALL_F64;
        split({1024, SBK_, 128, 64, false});                        // 4 workgroups per CU
        return p;
    }
    grid(BM);
    // split K when the output grid cannot fill the chip.  Resident slots: 256 CUs x (2 workgroups f32 | 1 f64).
    // reserve_cus: leave that many CUs without a workgroup of this (register-saturating) kernel, so that latency-bound
    // kernels of a concurrent stream can still be scheduled (the split-K grid is sized to the remaining CUs)
    split({(256 - reserve_cus) * (elem_size == 4 ? 2 : 1), BK, 256, 128, true});
    p.rev_m = 1;
    if (lower_only && p.tm != p.tn) { p.refusal = "lower_only needs a square output"; p.rc = -2; return p; }
    if (lower_only && tri == MXF_TRI_UPPER && p.splitk == 1 && p.tm >= 16) {
        for (int64_t x = 0; x < 8; ++x) {
            int64_t cnt = 0;
            for (int64_t r = x; r < p.tm; r += 8) cnt += r + 1;
            if (cnt > p.xc_max) p.xc_max = cnt;
        }
        p.nwg = 8 * p.xc_max * batch;
    }
    if (p.nwg > 2147483647LL) { p.refusal = "grid too large"; p.rc = -3; return p; }
    if (p.prescale && M > 65535) { p.refusal = "split-K path needs M<=65535"; p.rc = -3; return p; }     // (the pre-scale grid has a row per block)
    if (elem_size == 8 && vecA && vecB && M % BM == 0 && N % BN == 0 && K % DBK == 0 && p.kchunk % DBK == 0 && NWAVE == 8) p.kernel = MXF_GEMM_DMA_F64;
    return p;
}
