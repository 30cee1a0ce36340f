// Argument check and launch shapes of the difference-form Gram pass and its reverse mode (gram_diff.hip) as one pure function of the request:
// plain C++, no HIP, checked on the host by tests/host/gram_diff_plan_check.cpp.  Both kernels give a lane a column and a workgroup of 256
// lanes a tile of MXF_GD_COLS columns and a band of rows: MXF_GD_TR rows in the forward pass; in the reverse pass rb rows, whose row-side sums
// (rb x QT values) wait in LDS for one flush per workgroup.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mxf_gp.h"      // MXF_KD_*, MXF_GD_*

constexpr int MXF_GD_COLS = 256;                 // columns per workgroup: one per lane
constexpr int MXF_GD_TR = 64;                    // rows per forward workgroup, and rows staged in LDS at a time in the reverse pass
constexpr size_t MXF_GD_BWD_LDS_MAX = 16 * 1024; // bound of the reverse pass's row-side sums in LDS (dynamic): three to four workgroups per CU
constexpr int64_t MXF_GD_BWD_BLOCKS = 1024;      // the bands are halved until the grid has this many workgroups (four per CU)

struct GramDiffRequest {
    int kind = 0; size_t elem_size = 4; bool bwd = false;
    int S = 1; int64_t N = 0, N2 = 0; int Q = 0, A = 1; bool square = false;      // N2 is ignored on a square Gram
    bool has_X = true, has_p = true, has_K = true;                              // X; all three parameter operands; K_out (forward) or dK (reverse)
    int64_t sX = 0, sX2 = 0, sp0 = 0, sp1 = 0, sp2 = 0, sdiag = 0, ldk = 0, sK = 0;
};
struct GramDiffPlan {
    int rc = 0; const char* refusal = nullptr;   // nothing below is valid after a refusal
    int QT = 0;                                  // coordinate tile of the kernel: 1, 2, 4, 8, 16
    int64_t rb = 0;                              // rows per band
    unsigned grid[3] = {1, 1, 1};                // (column tiles, bands, samples)
    size_t lds_bytes = 0;                        // dynamic LDS (reverse pass)
};

// rows [r0, r1) of band by, columns [c0, c1) of tile bx
inline void gram_diff_rows(const GramDiffPlan& p, int64_t N, unsigned by, int64_t& r0, int64_t& r1) { r0 = (int64_t)by * p.rb; r1 = r0 + p.rb < N ? r0 + p.rb : N; }
inline void gram_diff_cols(int64_t N2, unsigned bx, int64_t& c0, int64_t& c1) { c0 = (int64_t)bx * MXF_GD_COLS; c1 = c0 + MXF_GD_COLS < N2 ? c0 + MXF_GD_COLS : N2; }

inline GramDiffPlan gram_diff_plan(const GramDiffRequest& r) {
    GramDiffPlan p;
    auto refuse = [&](int rc, const char* why) { p.rc = rc; p.refusal = why; return p; };
    const bool sm = r.kind == MXF_KD_SM;
    const int64_t N2 = r.square ? r.N : r.N2;
    if (r.kind != MXF_KD_PERIODIC && r.kind != MXF_KD_RQ && !sm) return refuse(-2, "unknown kind");
    if (r.S < 1 || r.N < 1 || N2 < 1 || r.Q < 1 || (sm && r.A < 1)) return refuse(-2, "S, N, N2, Q, A >= 1");
    if (sm ? r.Q > MXF_GD_SM_MAX_Q : r.Q > MXF_GD_MAX_Q) return refuse(-3, sm ? "Q above the limit of 8 input dimensions (SpectralMixture)" : "Q above the limit of 16 input dimensions");
    if (sm && r.A > MXF_GD_SM_MAX_A) return refuse(-3, "A above the limit of 8 components");
    if (!r.has_X || !r.has_p || !r.has_K) return refuse(-2, "null X, parameter operand or matrix");
    if (r.sX < 0 || r.sX2 < 0 || r.sp0 < 0 || r.sp1 < 0 || r.sp2 < 0 || r.sdiag < 0 || r.sK < 0 || r.ldk < N2) return refuse(-2, "negative sample stride or row stride below N2");
    p.QT = r.Q <= 1 ? 1 : (r.Q <= 2 ? 2 : (r.Q <= 4 ? 4 : (r.Q <= 8 ? 8 : 16)));
    const int64_t tiles = (N2 + MXF_GD_COLS - 1) / MXF_GD_COLS;
    p.rb = MXF_GD_TR;
    if (r.bwd) {
        const int64_t npad = (r.N + MXF_GD_TR - 1) / MXF_GD_TR * MXF_GD_TR;
        int64_t rb = (int64_t)(MXF_GD_BWD_LDS_MAX / ((size_t)p.QT * r.elem_size)) / MXF_GD_TR * MXF_GD_TR;
        if (rb > npad) rb = npad;
        while (rb > MXF_GD_TR && tiles * ((r.N + rb - 1) / rb) * r.S < MXF_GD_BWD_BLOCKS) rb = (rb / 2 + MXF_GD_TR - 1) / MXF_GD_TR * MXF_GD_TR;
        p.rb = rb;
        p.lds_bytes = (size_t)rb * p.QT * r.elem_size;
    }
    const int64_t bands = (r.N + p.rb - 1) / p.rb;
    if (tiles > 2147483647LL || bands > 65535 || r.S > 65535) return refuse(-3, "grid too large");
    p.grid[0] = (unsigned)tiles; p.grid[1] = (unsigned)bands; p.grid[2] = (unsigned)r.S;
    return p;
}
