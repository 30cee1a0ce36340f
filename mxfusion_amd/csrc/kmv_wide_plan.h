// Argument check, launch shape, LDS layout and scratch layout of the matrix-free kernel product for wide inputs (kmv_wide.hip: mxf_kmv_wide,
// mxf_kmv_wide_bwd) as one pure function of the request: plain C++, no HIP.  The request is mxf_kmv's (fused_plan.h: KmvRequest) and so are
// the texts of the refusals.  A workgroup of KW_LANES lanes owns a band of KW_TILE rows and walks tiles of KW_TILE columns; a lane owns
// KW_MICRO x KW_MICRO pairs of a tile.  The kernels carve their LDS block by kw_lds(): what the plan reports is what they use.
#pragma once
#include "fused_plan.h"      // KmvRequest, FusedRefusal, reduce_split, Carver, stride_ok

constexpr int KW_TILE = 64;         // rows of a band, columns of a tile
constexpr int KW_MICRO = 4;         // rows and columns of a lane's micro-tile: 16 lanes across a tile's columns, 16 down its rows
constexpr int KW_LANES = 256;
constexpr int KW_JB_SMALL = 4;      // columns of V per pass for J <= KW_JB_SMALL
constexpr int KW_TARGET = 512;      // workgroups the split of n2 aims for (two per compute unit)
constexpr int KW_WG = 64;           // weights of the bilinear form per launch of the kernel that writes them (a kernel argument)

constexpr int kw_qc(size_t es) { return es == 4 ? 16 : 8; }                     // coordinates (or columns of A and V) per staged chunk
constexpr int kw_ld(size_t es) { return KW_TILE + (int)(16 / es); }             // row stride of a staged chunk [kw_qc][kw_ld]: 16-byte pieces stay aligned
constexpr int kw_jb(size_t es) { return es == 4 ? 16 : 8; }                     // columns of V per pass above KW_JB_SMALL (the register counts)
constexpr int kw_vld(size_t es, int jb) { return jb + (int)(16 / es); }         // row stride of the tile of V [KW_TILE][kw_vld]: the 16 rows a wave reads lie in 16 bank groups

constexpr int KW_BWD_WAVES = 2;     // waves per SIMD the reverse kernel is compiled for: a budget of 256 registers

// byte offsets into a workgroup's LDS block.  Both passes: two buffers each of the band's and the tile's chunk (ps, zs) and of the chunk's
// per-coordinate scalars (ss).  Forward: the tile of V (vt).  Reverse: two buffers of the chunk's length-scale sums in double (dls), 16
// doubles for block_sum (red).
struct KwLds { size_t ps, zs, ss, vt, dls, red, bytes; };
constexpr KwLds kw_lds(size_t es, int jb, bool bwd) {
    KwLds l{};
    const size_t chunk = (size_t)kw_qc(es) * kw_ld(es) * es;
    l.ps = 0;
    l.zs = l.ps + 2 * chunk;
    l.ss = l.zs + 2 * chunk;
    l.vt = l.ss + (2 * kw_qc(es) * es + 15) / 16 * 16;
    l.dls = l.vt + (bwd ? 0 : (size_t)KW_TILE * kw_vld(es, jb) * es);
    l.red = l.dls + (bwd ? 2 * kw_qc(es) * sizeof(double) : 0);
    l.bytes = l.red + (bwd ? 16 * sizeof(double) : 0);
    return l;
}

struct KmvWidePlan : FusedRefusal {
    int jb = 0, npass = 0;              // forward: the kernel's <JB>; passes over n2 of jb columns of V each
    bool square = false; int64_t N2 = 0, ss_Z = 0;      // the second operand: X2, or X itself
    int64_t S_l = 1;                    // samples of the prepared scales
    int64_t ch = 0; int rows = 0;       // values of n2 per workgroup row (a multiple of KW_TILE), and the rows (grid[1])
    unsigned grid[3] = {1, 1, 1};       // (row bands, workgroup rows over n2, samples)
    int64_t n_scale = 0, n_out = 0, n_close = 0;      // items of the scale kernel, elements of out, threads of the close kernel
    int64_t ss_m2 = 0;                  // sample stride of the prepared scales
    int nl = 1;                         // length-scales per sample
    // zeroed doubles: the forward results under a split of n2; the sums of the reverse mode, (S, nl) then (S) at at_dv
    size_t n_zero = 0;
    size_t at_m2 = 0, at_w = 0, at_zero = 0, at_dv = 0, bytes = 0;
    size_t lds_bytes = 0;
};

inline KmvWidePlan kmv_wide_plan(const KmvRequest& r) {
    KmvWidePlan p;
    p.square = !r.has_X2;
    const int64_t N2 = p.N2 = p.square ? r.N : r.N2;
    p.ss_Z = p.square ? r.ss_X : r.ss_X2;
    if (r.S < 1 || r.S > 65535 || r.N < 1 || N2 < 1 || r.Q < 1 || r.J < 1) { p.refuse(-2, "1 <= S <= 65535 samples, N, N2, Q, J >= 1"); return p; }
    if (r.Q < MXF_KMV_WIDE_MIN_Q) { p.refusef(-3, "Q = %d belongs to mxf_kmv (Q <= %d)", r.Q, MXF_KMV_MAX_Q); return p; }
    if (r.Q > MXF_KMV_WIDE_MAX_Q) { p.refuse_q(r.Q, MXF_KMV_WIDE_MAX_Q); return p; }
    if (r.N > ((int64_t)1 << 31) || N2 > ((int64_t)1 << 31) || r.J > (1 << 16)) { p.refuse(-2, "N, N2 <= 2^31, J <= 2^16"); return p; }
    if (!r.has_X || !r.has_ls || !r.has_var || !r.has_V) { p.refuse(-2, "null X, lengthscale, variance or V"); return p; }
    if (r.bwd) {
        if (!r.has_A || !r.has_w) { p.refuse(-2, "null A or w"); return p; }
        if (!r.has_dls && !r.has_dvar) { p.refuse(-2, "null dls_acc and dvar_acc"); return p; }
    } else if (!r.has_out) { p.refuse(-2, "null out"); return p; }
    if (!stride_ok(r.ss_X, r.N * r.Q) || (!p.square && !stride_ok(r.ss_X2, N2 * r.Q)) || !stride_ok(r.ss_ls, r.ard ? r.Q : 1) || !stride_ok(r.ss_var, 1) ||
        (r.has_da && !stride_ok(r.ss_da, 1)) || !stride_ok(r.ss_V, N2 * r.J) || (r.bwd && !stride_ok(r.ss_A, r.N * r.J))) {
        p.refuse(-2, "a sample stride must be 0 or the elements of one sample (X: N Q; X2: N2 Q; lengthscale: Q or 1; variance, diag_add: 1; "
                     "V: N2 J; A: N J)");
        return p;
    }
    p.jb = r.bwd ? 0 : (r.J <= KW_JB_SMALL ? KW_JB_SMALL : kw_jb(r.esize));
    p.npass = r.bwd ? 1 : (int)mxf_cdiv(r.J, p.jb);
    p.S_l = r.ss_ls ? r.S : 1;
    p.nl = r.ard ? r.Q : 1;
    const ReduceSplit sp = reduce_split(r.S, r.N, N2, KW_TILE, KW_TILE, KW_TARGET);
    p.ch = sp.ch; p.rows = sp.rows;
    p.grid[0] = (unsigned)mxf_cdiv(r.N, KW_TILE); p.grid[1] = (unsigned)p.rows; p.grid[2] = (unsigned)r.S;
    p.n_scale = p.S_l * r.Q; p.n_out = (int64_t)r.S * r.N * r.J; p.n_close = p.nl;
    p.ss_m2 = p.S_l > 1 ? r.Q : 0;
    p.n_zero = r.bwd ? (size_t)r.S * (p.nl + 1) : (p.rows > 1 ? (size_t)p.n_out : 0);
    Carver cv(nullptr);
    p.at_m2 = mxf_piece(cv, (size_t)p.n_scale * r.esize);
    p.at_w = mxf_piece(cv, r.bwd ? (size_t)r.J * r.esize : 0);
    p.at_zero = mxf_piece(cv, p.n_zero * sizeof(double));
    p.at_dv = p.at_zero + (size_t)r.S * p.nl * sizeof(double);
    p.bytes = cv.off;
    p.lds_bytes = kw_lds(r.esize, r.bwd ? 0 : p.jb, r.bwd).bytes;
    return p;
}
