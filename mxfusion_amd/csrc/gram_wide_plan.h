// Argument check, launch shape and LDS layout of the wide-input Gram passes (gram_wide.hip: mxf_gram_wide, mxf_gram_wide_bwd) as one pure
// function of the request: plain C++, no HIP, checked on the host by tests/host/gram_wide_plan_check.cpp.  Both kernels give a workgroup of
// 256 lanes a tile of MXF_GW_TILE x MXF_GW_TILE pairs and a lane a micro-tile of MXF_GW_MICRO x MXF_GW_MICRO of them, whose r^2 live in
// registers; the tile's raw coordinates pass through LDS one chunk of gw_qc() coordinates at a time, double-buffered, so Q is bounded by
// index width only.  The kernels carve their LDS block by gw_lds(): what the plan reports is what they use.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mxf_gp.h"      // MXF_K_*, MXF_GW_MIN_Q, MXF_GW_MAX_Q

constexpr int MXF_GW_TILE = 64;                     // rows and columns of a workgroup's tile
constexpr int MXF_GW_MICRO = 4;                     // rows and columns of a lane's micro-tile: 16 lanes across a tile's columns, 16 down its rows
constexpr int MXF_GW_LANES = 256;
constexpr int MXF_GW_RS = MXF_GW_TILE + 1;          // row stride of a chunk's gradient sums in LDS (odd: the flush reads down a column of it)
constexpr size_t MXF_GW_LDS_MAX = 64 * 1024;        // the static LDS of a kernel

constexpr int gw_qc(size_t es) { return es == 4 ? 16 : 8; }                  // coordinates per chunk
constexpr int gw_ld(size_t es) { return MXF_GW_TILE + (int)(16 / es); }      // row stride of a staged chunk [gw_qc][gw_ld]: 16-byte pieces stay aligned

// byte offsets into a workgroup's LDS block.  Both passes: two buffers each of the rows' and the columns' chunk (xs, zs) and of the chunk's
// squared scales m2 and inverse length-scales il.  Reverse pass: two buffers each of the chunk's row-side and column-side sums (racc, cacc:
// [gw_qc][MXF_GW_RS]) and of its length-scale sums in double (dls: [gw_qc]), one double for an isotropic length-scale, 16 for block_sum.
struct GwLds { size_t xs, zs, m2, il, racc, cacc, dls, iso, red, bytes; };
constexpr GwLds gw_lds(size_t es, bool bwd) {
    GwLds l{};
    const size_t chunk = (size_t)gw_qc(es) * gw_ld(es) * es, par = (size_t)gw_qc(es) * es, sums = (size_t)gw_qc(es) * MXF_GW_RS * es;
    l.xs = 0;
    l.zs = l.xs + 2 * chunk;
    l.m2 = l.zs + 2 * chunk;
    l.il = l.m2 + 2 * par;
    l.racc = l.il + 2 * par;
    l.cacc = l.racc + (bwd ? (2 * sums + 15) / 16 * 16 : 0);
    l.dls = l.cacc + (bwd ? (2 * sums + 15) / 16 * 16 : 0);
    l.iso = l.dls + (bwd ? 2 * gw_qc(es) * sizeof(double) : 0);
    l.red = l.iso + (bwd ? 2 * sizeof(double) : 0);
    l.bytes = l.red + (bwd ? 16 * sizeof(double) : 0);
    return l;
}

struct GramWideRequest {
    int kind = 0; size_t elem_size = 4; bool bwd = false;
    int S = 1; int64_t N = 0, N2 = 0; int Q = 0; bool square = false;      // N2 is ignored on a square Gram
    bool has_X = true, has_ls = true, has_var = true, has_K = true;        // K_out (forward) or dK (reverse)
    int64_t sX = 0, sX2 = 0, sls = 0, svar = 0, sdiag = 0, ldk = 0, sK = 0;
};
struct GramWidePlan {
    int rc = 0; const char* refusal = nullptr;   // nothing below is valid after a refusal
    int qc = 0, chunks = 0;                      // coordinates per chunk, chunks per sweep
    unsigned grid[3] = {1, 1, 1};                // (column tiles, row tiles, samples)
    size_t lds_bytes = 0;
};

// rows [r0, r1) of row tile by, columns [c0, c1) of column tile bx
inline void gram_wide_span(int64_t n, unsigned b, int64_t& lo, int64_t& hi) { lo = (int64_t)b * MXF_GW_TILE; hi = lo + MXF_GW_TILE < n ? lo + MXF_GW_TILE : n; }

inline GramWidePlan gram_wide_plan(const GramWideRequest& r) {
    GramWidePlan p;
    auto refuse = [&](int rc, const char* why) { p.rc = rc; p.refusal = why; return p; };
    const int64_t N2 = r.square ? r.N : r.N2;
    // the limits first: before any pointer is looked at
    if (r.kind != MXF_K_RBF && r.kind != MXF_K_MATERN12 && r.kind != MXF_K_MATERN32 && r.kind != MXF_K_MATERN52) return refuse(-3, "stationary kinds only (RBF, Matern12, Matern32, Matern52)");
    if (r.Q < MXF_GW_MIN_Q) return refuse(-3, "Q <= 16 belongs to the coordinate kernels (mxf_gram, mxf_gram_bwd)");
    if (r.Q > MXF_GW_MAX_Q) return refuse(-3, "Q above MXF_GW_MAX_Q input dimensions");
    if (r.elem_size != 4 && r.elem_size != 8) return refuse(-2, "float32 or float64");
    if (r.S < 1 || r.N < 1 || N2 < 1) return refuse(-2, "S, N, N2 >= 1");
    const int64_t ct = (N2 + MXF_GW_TILE - 1) / MXF_GW_TILE, rt = (r.N + MXF_GW_TILE - 1) / MXF_GW_TILE;
    if (ct > 2147483647LL || rt > 65535 || r.S > 65535) return refuse(-3, "grid too large");
    if (!r.has_X || !r.has_ls || !r.has_var || !r.has_K) return refuse(-2, "null X, lengthscale, variance or matrix");
    if (r.sX < 0 || r.sX2 < 0 || r.sls < 0 || r.svar < 0 || r.sdiag < 0 || r.sK < 0 || r.ldk < N2) return refuse(-2, "negative sample stride or row stride below N2");
    p.qc = gw_qc(r.elem_size);
    p.chunks = (r.Q + p.qc - 1) / p.qc;
    p.grid[0] = (unsigned)ct; p.grid[1] = (unsigned)rt; p.grid[2] = (unsigned)r.S;
    p.lds_bytes = gw_lds(r.elem_size, r.bwd).bytes;
    if (p.lds_bytes > MXF_GW_LDS_MAX) return refuse(-3, "LDS above the bound");      // (not reachable: 36.9 KB at most)
    return p;
}
