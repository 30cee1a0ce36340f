// Launch shapes and scratch layout of the Gram reverse passes (gram_bwd.hip, svgp_bwd_mfma.hip) as pure functions of the problem sizes:
// plain C++, no HIP, checked on the host by tests/host/gram_bwd_plan_check.cpp.  The launchers pass the probe-build knobs in.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- difference-form pass (gram_bwd_kernel): a block owns ct column tiles of 256 columns and a band of rb rows ------------------------
constexpr int MXF_BWD_TRB = 64;          // rows staged in LDS at a time; rb is a multiple of it
struct GramBwdPlan {
    int64_t rb = 0;                      // rows per band
    int ct = 0;                          // column tiles per block
    unsigned grid[3] = {1, 1, 1};        // (groups of ct column tiles, bands, samples)
    size_t lds_bytes = 0;                // dynamic LDS: the band's accumulators rb * (QT + PT) * elem_size + the staged tile and the reduction words
    bool grid_too_large = false;
};
// QT: the kernel's coordinate tile (2, 4, 8, 16); PT: its output tile (0: plain pass); lds_kb: LDS budget per block (the row accumulators:
// 30 KB = five blocks per CU; 80 KB, two blocks and fewer row flushes, measured 1 % slower per step); grid_target: blocks wanted -- enough
// to fill the chip (~16 per CU at five resident blocks each) while keeping the per-block row flush amortised
inline GramBwdPlan gram_bwd_plan(int64_t N, int64_t N2, int S, int QT, int PT, size_t elem_size, int lds_kb, int64_t grid_target) {
    constexpr int64_t TRB = MXF_BWD_TRB;
    GramBwdPlan p;
    const size_t row = (size_t)(QT + PT) * elem_size, fixed = (size_t)(TRB * QT + TRB * PT + 16) * elem_size + 16 * sizeof(double) + 64;
    int64_t rb = (int64_t)(((size_t)lds_kb * 1024 - fixed) / row) / TRB * TRB;
    if (rb < TRB) rb = TRB;
    const int64_t npad = (N + TRB - 1) / TRB * TRB, tiles = (N2 + 255) / 256;
    if (rb > npad) rb = npad;
    // small problems (the M x M core Gram): split the rows into bands so that the grid still fills the chip
    while (rb > TRB && tiles * ((N + rb - 1) / rb) * S < 512) rb = (rb / 2 + TRB - 1) / TRB * TRB;
    const int64_t rblocks = (N + rb - 1) / rb, ct = (tiles * rblocks * S + grid_target - 1) / grid_target;
    p.rb = rb;
    p.ct = (int)(ct < 1 ? 1 : (ct > 64 ? 64 : ct));
    p.grid[0] = (unsigned)((tiles + p.ct - 1) / p.ct); p.grid[1] = (unsigned)rblocks; p.grid[2] = (unsigned)S;
    p.grid_too_large = p.grid[1] > 65535u || p.grid[2] > 65535u;
    p.lds_bytes = (size_t)rb * row + fixed;
    return p;
}

// ---- which pass the SVGP-fused reverse mode takes: the shape halves of mxf_svgp_bwd_is_mfma / mxf_svgp_bwd_reads_blocked (the other half is
// the 16-byte alignment of T, which the SVGP composite's scratch always has) -----------------------------------------------------------------
constexpr int MXF_BWD_PMAX_ALL = 8;      // output columns of the difference-form fused pass's widest kernel
inline bool svgp_bwd_mfma_shape(bool rbf, bool f32, int64_t SB, int64_t B, int Q, int P) {
    return rbf && f32 && P == 1 && Q <= 8 && SB % 4 == 0 && SB >= 16 && B % 16 == 0;
}
// the difference-form pass reads T in 16-column blocks as well as row-major for these shapes (the matrix-pipe pass reads blocks only)
inline bool svgp_bwd_diff_reads_blocked(bool f32, int64_t SB, int Q, int P) { return f32 && Q <= 16 && P <= MXF_BWD_PMAX_ALL && SB % 16 == 0; }

// ---- matrix-pipe pass (svgp_bwd_mfma_kernel): a block owns ct groups of 64 columns and a band of MXF_MF_RB rows ------------------------
#ifndef MXF_MF_MT
#define MXF_MF_MT 8
#endif
constexpr int MXF_MF_RB = 16 * MXF_MF_MT;    // rows per band: MXF_MF_MT row tiles of 16
struct SvgpBwdMfmaPlan {
    const char* refusal = nullptr;       // why the pass cannot take this shape (nothing below is valid then)
    int ct = 0;
    unsigned grid[3] = {1, 1, 1};        // (groups of ct column quads, bands, 1)
    bool full = false;                   // no ragged tiles: M % MXF_MF_RB == 0 and SB % 64 == 0
    // One scratch buffer, byte offsets.  [0, zero_bytes) is cleared on every call: zacc, double [M][16] (0..7 B_mq, 8 S_m, 9 R_m); dls3, double [8]
    // (sum_n x_nq^2 C_n); mx, unsigned [2] (bit patterns of max |w_m|, max |y_n - U_n|); and centre, float [8] (of the inducing inputs; written
    // after the clear).  Then the scaled, centred coordinates Zs, float [M][8], Xs, float [SB][8], and their squared norms Xn, float [SB].
    size_t zacc = 0, dls3 = 0, mx = 0, centre = 0, zero_bytes = 0, Zs = 0, Xs = 0, Xn = 0, total_bytes = 0;
};
// grid_target: work items, ~1024 (r03; was 8192).  Every workgroup ends with a flush of its row-side sums (LDS, then float64 atomics), a fixed cost
// per workgroup: with 8192 of them the pass took 0.82 ms at 4 samples where 3.0 / 8 = 0.38 was its share (per-rank step 5.02 -> 4.63 ms
// with 1024; 32 samples: 25.18 -> 24.79 ms; 512 measures the same, tests/probes/bwd_grid.sh)
inline SvgpBwdMfmaPlan svgp_bwd_mfma_plan(int64_t M, int64_t SB, int64_t B, int64_t grid_target) {
    SvgpBwdMfmaPlan p;
    p.dls3 = (size_t)M * 16 * sizeof(double);
    p.mx = p.dls3 + 8 * sizeof(double);
    p.centre = p.mx + sizeof(double);
    p.zero_bytes = p.Zs = ((size_t)M * 16 + 16) * sizeof(double);
    p.Xs = p.Zs + (size_t)M * 8 * sizeof(float);
    p.Xn = p.Xs + (size_t)SB * 8 * sizeof(float);
    p.total_bytes = p.Xn + (size_t)SB * sizeof(float);
    const int64_t quads = (SB + 63) / 64, bands = (M + MXF_MF_RB - 1) / MXF_MF_RB, ct = (quads * bands + grid_target - 1) / grid_target;
    p.ct = (int)(ct < 1 ? 1 : (ct > 256 ? 256 : ct));
    p.grid[0] = (unsigned)((quads + p.ct - 1) / p.ct); p.grid[1] = (unsigned)bands;
    p.full = (M % MXF_MF_RB == 0) && (SB % 64 == 0);
    if (SB > 2147483647LL - 4096) p.refusal = "more than 2^31 columns";      // (32-bit column indices in the pass)
    else if (B <= 0 || SB / B > 65535 || SB % B != 0) p.refusal = "bad sample layout";      // (whole samples, SB = S B, one grid row each in the prescale)
    else if (bands > 65535) p.refusal = "too many row bands";
    return p;
}
