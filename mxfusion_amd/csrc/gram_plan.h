// Path, tile sizes, grids and scratch layout of the forward Gram launchers (gram.hip: mxf_gram_internal, mxf_gram_planes_internal) as pure
// functions of the problem: plain C++, no HIP, checked on the host by tests/host/gram_plan_check.cpp.  The tile sizes are the kernels' own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mxf_gp.h"      // MXF_K_*, MXF_WRITE

namespace mxf_gram_tiles {
constexpr int TR = 64;                 // the pre-scaled x copy is padded to whole blocks of TR rows; the most rows a workgroup walks
// rows per workgroup, measured on MI355X at N=65536, Q=8 (tests/probes/gram_variants.hip, tests/probes/gram_time.py): single-wave workgroups;
// float32 RBF 12 rows as a compile-time constant with the diagonal term hoisted (gram_lean_kernel TRC); float64 RBF in the expansion form
// (gram_lean_kernel XF) 16 rows (5.71 ms = 6.02 TB/s, 32: 5.95, 64: 6.36 ms); the VALU-heavier epilogues (Matern, ...) 64
constexpr int TR_RBF_F32 = 12, TR_RBF_F64 = 16;
constexpr int GENERIC_COLS = 256;      // gram_generic_kernel: one column per thread
constexpr int PL_ROWS = 64, PL_KB = 16;   // gram_planes_lean_kernel: minor rows per workgroup, major points per k block
}  // namespace mxf_gram_tiles

enum { MXF_GRAM_GENERIC = 0, MXF_GRAM_COORD_FAST = 1, MXF_GRAM_COORD_SLOW = 2, MXF_GRAM_LEAN = 3, MXF_GRAM_LEAN_XF = 4 };
enum { MXF_GRAM_CENTRE_NONE = 0, MXF_GRAM_CENTRE_X = 1, MXF_GRAM_CENTRE_X2 = 2 };
struct GramPlan {
    const char* refusal = nullptr; int rc = 0;     // why the launcher cannot take this shape, and its error code (nothing below is valid then)
    int path = MXF_GRAM_GENERIC;
    int QT = 0;                                    // coordinate tile of the kernels (2, 4, 8, 16); 0 on the generic path
    int tr = 0; unsigned ncb = 0;                  // rows per workgroup; column blocks of 64 * VEC columns
    unsigned grid[3] = {1, 1, 1};                  // of the chosen path's Gram kernel
    int64_t padr = 0, padc = 0, padx = 0;          // padded rows of N, of N2, and of the x copy (a square Gram reads it in both roles)
    int Sx = 0, Sz = 0;                            // pre-scaled copies of X / X2: one shared by the samples, or one per sample
    int centre = MXF_GRAM_CENTRE_NONE; int64_t scen = 0;     // whose first row both operands are centred on, and its sample stride
    // One scratch buffer, offsets and sample strides in elements (a stride is 0 where the samples share the copy): the pre-scaled coordinates
    // xs [Sx][padx][QT] and zs [Sz][padc][QT], then (LEAN_XF only) their squared norms xn [Sx][padx] and zn [Sz][padc].  A square Gram has no z
    // regions: zs / zn are xs / xn.  BIAS and WHITE take no scratch.
    int64_t xs = 0, zs = 0, xn = 0, zn = 0, sxs = 0, szs = 0, sxn = 0, szn = 0;
    size_t bytes = 0;
    int has_diag = 0;                              // GramLean::has_diag: bit 0 a diagonal term exists, bit 1 the diagonal is set to the variance first
};

// vec_ok: the output takes 16-byte stores (ldk and the sample stride multiples of VEC, the base 16-byte aligned); has_diag: a square Gram with a
// diag_add array or a non-zero jitter.  N2, sX2 are ignored on a square Gram.
static inline GramPlan gram_plan(int kind, size_t elem_size, int S, int64_t N, int64_t N2, int Q, bool square, int64_t sX, int64_t sX2, int64_t sls,
                                 bool vec_ok, int mode, bool has_diag) {
    using namespace mxf_gram_tiles;
    GramPlan p;
    if (square) { N2 = N; sX2 = sX; }
    if (Q > 16) {      // one output per thread, coordinates from global memory; grid.y is capped at 65535 row slots
        p.grid[0] = (unsigned)((N2 + GENERIC_COLS - 1) / GENERIC_COLS); p.grid[1] = (unsigned)(N < 65535 ? N : 65535); p.grid[2] = (unsigned)S;
        return p;
    }
    const bool flat = kind == MXF_K_BIAS || kind == MXF_K_WHITE;      // no coordinates enter the covariance
    const bool rbf = kind == MXF_K_RBF;
    const int VEC = (int)(16 / elem_size);
    p.QT = (flat || Q <= 2) ? 2 : (Q <= 4 ? 4 : (Q <= 8 ? 8 : 16));
    p.tr = rbf ? (elem_size == 4 ? TR_RBF_F32 : TR_RBF_F64) : TR;
    const int64_t cw = 64 * VEC, rblocks = (N + p.tr - 1) / p.tr;      // columns per workgroup; row blocks
    p.ncb = (unsigned)((N2 + cw - 1) / cw);
    const int64_t nblk = (int64_t)p.ncb * rblocks;
    if (nblk > 2147483647LL) { p.refusal = "problem too large for one launch"; p.rc = -3; return p; }
    // fast: plain overwrite with whole 16-byte stores; lean: ... and coordinates, and the row blocks fit grid.y
    const bool fast = vec_ok && mode == MXF_WRITE && N2 % VEC == 0;
    const bool lean = fast && !flat && rblocks <= 65535;
    const bool xf = lean && elem_size == 8 && rbf;
    p.path = xf ? MXF_GRAM_LEAN_XF : (lean ? MXF_GRAM_LEAN : (fast ? MXF_GRAM_COORD_FAST : MXF_GRAM_COORD_SLOW));
    if (lean) { p.grid[0] = p.ncb; p.grid[1] = (unsigned)rblocks; }      // x = column block (fastest), y = row block
    else p.grid[0] = (unsigned)nblk;                                     // column block fastest within x
    p.grid[2] = (unsigned)S;
    p.has_diag = (has_diag ? 1 : 0) | ((xf && square) ? 2 : 0);
    if (flat) return p;
    p.padr = (N + TR - 1) / TR * TR;
    p.padc = (N2 + 4 * cw - 1) / (4 * cw) * (4 * cw);
    p.padx = square ? (p.padr > p.padc ? p.padr : p.padc) : p.padr;
    p.Sx = (sX == 0 && sls == 0) ? 1 : S;
    p.Sz = (sX2 == 0 && sls == 0) ? 1 : S;
    // the common centre of both operands: the first row of X, or of X2 when X is sampled and X2 shared (its pre-scaled copy is then shared by
    // the samples and must not depend on one of them)
    const bool cen_x2 = !square && sX != 0 && sX2 == 0;
    p.centre = kind == MXF_K_LINEAR ? MXF_GRAM_CENTRE_NONE : (cen_x2 ? MXF_GRAM_CENTRE_X2 : MXF_GRAM_CENTRE_X);
    p.scen = p.centre == MXF_GRAM_CENTRE_X ? sX : 0;
    const int64_t xrows = (int64_t)p.Sx * p.padx, zrows = square ? 0 : (int64_t)p.Sz * p.padc;
    p.sxs = p.Sx == 1 ? 0 : p.padx * p.QT; p.sxn = p.Sx == 1 ? 0 : p.padx;
    p.zs = square ? p.xs : xrows * p.QT;
    p.szs = square ? p.sxs : (p.Sz == 1 ? 0 : p.padc * p.QT);
    p.xn = (xrows + zrows) * p.QT;
    p.zn = square ? p.xn : p.xn + (xf ? xrows : 0);
    p.szn = square ? p.sxn : (p.Sz == 1 ? 0 : p.padc);
    p.bytes = (size_t)((xrows + zrows) * (p.QT + (xf ? 1 : 0))) * elem_size;
    return p;
}

// ---- the Gram as split planes (gram_planes_lean_kernel): a workgroup owns PL_ROWS minor rows and kbpb k blocks of PL_KB major points ----------
struct GramPlanesPlan {
    const char* refusal = nullptr; int rc = 0;
    int QT = 0;                         // 8 or 16
    int64_t padr = 0, padk = 0;         // padded minor rows / major points of the raw coordinate copies
    int kbpb = 0;                       // k blocks per workgroup
    unsigned grid[2] = {1, 1};          // (blocks of PL_ROWS rows, groups of kbpb k blocks)
    int PT = 0;                         // fused-row variant: 0 none, 1 one weight column, 8 up to eight
    size_t bytes = 0;                   // caller-owned scratch: (padr + padk) * QT floats
};
// fused: the pass also forms the row U = w^T K (grid.y == 1 then: every workgroup walks all k blocks of its rows); kb: the k blocks per
// workgroup otherwise (MXF_PLANES_KB), doubled until grid.y fits
static inline GramPlanesPlan gram_planes_plan(int64_t R, int64_t Kn, int Q, bool fused, bool has_w, int Pw, int64_t kb) {
    using namespace mxf_gram_tiles;
    GramPlanesPlan p;
    p.QT = Q <= 8 ? 8 : 16;
    const int64_t K16 = (Kn + PL_KB - 1) / PL_KB;
    p.padr = (R + 2 * PL_ROWS - 1) / (2 * PL_ROWS) * (2 * PL_ROWS);
    p.padk = (K16 + 15) / 16 * (16 * PL_KB);
    p.bytes = (size_t)(p.padr + p.padk) * p.QT * sizeof(float);
    if (Q > 16) { p.refusal = "Q > 16 not supported"; p.rc = -3; return p; }
    if (fused && (Pw > 8 || !has_w)) { p.refusal = "fused w^T K needs w and P <= 8"; p.rc = -3; return p; }
    p.kbpb = fused ? (int)K16 : (int)kb;
    while (!fused && (K16 + p.kbpb - 1) / p.kbpb > 65535) p.kbpb *= 2;
    p.grid[0] = (unsigned)((R + PL_ROWS - 1) / PL_ROWS); p.grid[1] = (unsigned)((K16 + p.kbpb - 1) / p.kbpb);
    p.PT = fused ? (Pw == 1 ? 1 : 8) : 0;
    return p;
}
// the caller-owned scratch of one planes pass: the same function of (R, Kn, Q) whatever else is asked
static inline size_t gram_planes_scratch_bytes(int64_t R, int64_t Kn, int Q) { return gram_planes_plan(R, Kn, Q, false, false, 0, 1).bytes; }
