// Argument check and launch shapes of the fused ICM Gram pass and its reverse mode (gram_icm.hip) as one pure function of the request:
// plain C++, no HIP, checked on the host by tests/host/gram_icm_plan_check.cpp.  Both kernels give a lane a column and a workgroup of 256
// lanes a tile of MXF_ICM_COLS columns and a band of rows, staged MXF_ICM_TR rows at a time (coordinates and output indices) in LDS next to
// the sample's T x T coregionalisation matrix.  Forward: the band is MXF_ICM_TR rows.  Reverse: the band is rb rows, whose row-side sums
// (rb x QT values) wait in LDS for one flush per workgroup; with dB asked for, every lane owns one LDS word per output (T x 256 values: a
// lane's column has ONE output index, a row's is wave-uniform, so the pair's term goes to word [idx[row]][lane] with a plain read and
// write -- no atomic, no bank conflict) and the workgroup folds them into a T x T double partial in LDS before T x T global atomics.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mxf_gp.h"      // MXF_K_*, MXF_ICM_MAX_T

constexpr int MXF_ICM_COLS = 256;                   // columns per workgroup: one per lane
constexpr int MXF_ICM_TR = 64;                      // rows per forward workgroup, and rows staged in LDS at a time in the reverse pass
constexpr int MXF_ICM_MAX_Q = 16;                   // input dimensions (as mxf_gram2)
constexpr size_t MXF_ICM_BWD_ROWS_LDS_MAX = 16 * 1024; // bound of the reverse pass's row-side sums in LDS
constexpr size_t MXF_ICM_LDS_MAX = 112 * 1024;      // bound of a workgroup's LDS, both passes (the CU has 160 KB)
constexpr int64_t MXF_ICM_BWD_BLOCKS = 1024;        // the bands are halved until the grid has this many workgroups (four per CU)

struct GramIcmRequest {
    int kind = 0; size_t elem_size = 4; bool bwd = false;
    int S = 1; int64_t N = 0, N2 = 0; int Q = 0, T = 0; bool ard = false, square = false;      // N2 is ignored on a square Gram
    bool has_X = true, has_idx = true, has_idx2 = true, has_ls = true, has_var = true, has_B = true, has_K = true;      // K_out (forward) or dK (reverse)
    bool want_dB = false;                                                                      // reverse: dB is asked for
    int64_t sX = 0, sX2 = 0, sls = 0, svar = 0, sB = 0, sdiag = 0, ldk = 0, sK = 0;
};
struct GramIcmPlan {
    int rc = 0; const char* refusal = nullptr;   // nothing below is valid after a refusal
    int QT = 0;                                  // coordinate tile of the kernel: 1, 2, 4, 8, 16
    int64_t rb = 0;                              // rows per band
    unsigned grid[3] = {1, 1, 1};                // (column tiles, bands, samples)
    // LDS of a workgroup, byte offsets into one dynamic block: the staged coordinates xs [TR][QT], the staged output indices ridx [TR] and
    // B [T][T] (both passes); reverse pass only: the row-side sums racc [rb][QT], the per-lane dB words dBp [T][256] and their double fold
    // dBs [T][T] (these two only with want_dB), and 16 doubles for the block reductions
    size_t xs = 0, ridx = 0, Bs = 0, racc = 0, dBp = 0, dBs = 0, red = 0, lds_bytes = 0;
};

// rows [r0, r1) of band by, columns [c0, c1) of tile bx
inline void gram_icm_rows(const GramIcmPlan& p, int64_t N, unsigned by, int64_t& r0, int64_t& r1) { r0 = (int64_t)by * p.rb; r1 = r0 + p.rb < N ? r0 + p.rb : N; }
inline void gram_icm_cols(int64_t N2, unsigned bx, int64_t& c0, int64_t& c1) { c0 = (int64_t)bx * MXF_ICM_COLS; c1 = c0 + MXF_ICM_COLS < N2 ? c0 + MXF_ICM_COLS : N2; }

inline GramIcmPlan gram_icm_plan(const GramIcmRequest& r) {
    GramIcmPlan p;
    auto refuse = [&](int rc, const char* why) { p.rc = rc; p.refusal = why; return p; };
    auto up = [](size_t x) { return (x + 15) / 16 * 16; };
    const int64_t N2 = r.square ? r.N : r.N2;
    if (r.kind != MXF_K_RBF && r.kind != MXF_K_MATERN12 && r.kind != MXF_K_MATERN32 && r.kind != MXF_K_MATERN52) return refuse(-2, "stationary kinds only (RBF, Matern12, Matern32, Matern52)");
    if (r.S < 1 || r.N < 1 || N2 < 1 || r.Q < 1 || r.T < 1) return refuse(-2, "S, N, N2, Q, T >= 1");
    if (r.Q > MXF_ICM_MAX_Q) return refuse(-3, "Q above the limit of 16 input dimensions");
    if (r.T > MXF_ICM_MAX_T) return refuse(-3, "T above the limit of 32 outputs");
    if (!r.has_X || !r.has_idx || (!r.square && !r.has_idx2) || !r.has_ls || !r.has_var || !r.has_B || !r.has_K) return refuse(-2, "null X, index, parameter operand, B or matrix");
    if (r.sX < 0 || r.sX2 < 0 || r.sdiag < 0 || r.sK < 0 || r.ldk < N2) return refuse(-2, "negative sample stride or row stride below N2");
    // a parameter operand is shared by the samples (stride 0) or has one packed row per sample: its gradient is laid out the same way
    if ((r.sls != 0 && r.sls != (r.ard ? r.Q : 1)) || (r.svar != 0 && r.svar != 1) || (r.sB != 0 && r.sB != (int64_t)r.T * r.T))
        return refuse(-2, "a sample stride of lengthscale, variance or B that is neither 0 nor the operand's row");
    p.QT = r.Q <= 1 ? 1 : (r.Q <= 2 ? 2 : (r.Q <= 4 ? 4 : (r.Q <= 8 ? 8 : 16)));
    const int64_t tiles = (N2 + MXF_ICM_COLS - 1) / MXF_ICM_COLS;
    const size_t es = r.elem_size;
    p.rb = MXF_ICM_TR;
    if (r.bwd) {
        const int64_t npad = (r.N + MXF_ICM_TR - 1) / MXF_ICM_TR * MXF_ICM_TR;
        int64_t rb = (int64_t)(MXF_ICM_BWD_ROWS_LDS_MAX / ((size_t)p.QT * es)) / MXF_ICM_TR * MXF_ICM_TR;
        if (rb > npad) rb = npad;
        while (rb > MXF_ICM_TR && tiles * ((r.N + rb - 1) / rb) * r.S < MXF_ICM_BWD_BLOCKS) rb = (rb / 2 + MXF_ICM_TR - 1) / MXF_ICM_TR * MXF_ICM_TR;
        p.rb = rb;
    }
    p.xs = 0;
    p.ridx = p.xs + up((size_t)MXF_ICM_TR * p.QT * es);
    p.Bs = p.ridx + up((size_t)MXF_ICM_TR * sizeof(int));
    p.racc = p.Bs + up((size_t)r.T * r.T * es);
    p.dBp = p.racc + (r.bwd ? up((size_t)p.rb * p.QT * es) : 0);
    p.dBs = p.dBp + (r.bwd && r.want_dB ? up((size_t)r.T * MXF_ICM_COLS * es) : 0);
    p.red = p.dBs + (r.bwd && r.want_dB ? up((size_t)r.T * r.T * sizeof(double)) : 0);
    p.lds_bytes = p.red + (r.bwd ? 16 * sizeof(double) : 0);
    if (p.lds_bytes > MXF_ICM_LDS_MAX) return refuse(-3, "LDS above the bound");      // (not reachable within the limits above: 104.5 KB at most)
    const int64_t bands = (r.N + p.rb - 1) / p.rb;
    if (tiles > 2147483647LL || bands > 65535 || r.S > 65535) return refuse(-3, "grid too large");
    p.grid[0] = (unsigned)tiles; p.grid[1] = (unsigned)bands; p.grid[2] = (unsigned)r.S;
    return p;
}
