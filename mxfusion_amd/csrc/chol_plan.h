// The form a blocked Cholesky factorisation takes and the merge levels of the triangular inverse (chol.hip: mxf_potrf_internal,
// mxf_trtri_internal) as pure functions of the problem: plain C++, no HIP, checked on the host by tests/host/chol_plan_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mxf_chol_tiles {
constexpr int NB = 64;          // inner block
constexpr int NBO = 512;        // outer panel
constexpr int TRI_MIN = 1024;   // trtri merge levels from this block size on use the triangular-aware GEMM k ranges
}  // namespace mxf_chol_tiles

// zero_upper_kernel takes one matrix row per grid.y slot: nullptr, or why a launcher that runs it refuses n (error code -3, before anything is queued)
static inline const char* chol_rows_refusal(int64_t n) { return n > 65535 ? "n too large" : nullptr; }

// ---- potrf ----------------------------------------------------------------------------------------------------------------------------------
// What the launcher gathers.  capturing / aux_streams are only asked for (and the streams only created) when potrf_may_look says so.
struct PotrfRequest {
    size_t esize = 8; int S = 1; int64_t n = 0;
    int ncu = 64;                   // compute units of the device
    bool capturing = false;         // the caller's stream is being captured (the auxiliary streams are not part of the capture)
    bool aux_streams = false;       // the handle's auxiliary streams and events exist (mxf_potrf_aux_init)
    bool want_inverse = false;      // the caller passed a buffer for L^-1
    bool zero_upper = true;         // the strict upper triangle is zeroed afterwards
    // knobs: MXF_POTRF_ONE_MAX (n = 2048 as ONE left-looking launch: 2.6 ms vs 1.9 -- the last block rows carry 32 i^2 columns of products
    // each), MXF_POTRF_SPLIT_ROWS, MXF_POTRF_EAGER_INV (row blocks of the eager inverse in outer panels; 0: no eager inverse)
    int64_t one_max = 512, split_rows = 64, eager_panels = 2;
};

// float64 with n a multiple of 64: the tile kernel, one launch up to one_max, one per outer panel of NBO columns beyond; float32 and ragged n:
// one panel-kernel launch per 64 columns.  The stages of PotrfCall rely on:
//   one_launch => panel_tiles;   panel_tiles => 8-byte elements, n % NB == 0 and a workgroup per block row fits the device;
//   eager => look => the auxiliary streams exist and the stream is not being captured;   eager => panel_tiles and S == 1;   split(c0) => panel_tiles.
struct PotrfPlan {
    const char* refusal = nullptr;      // why the launcher cannot take this shape (error code -3; nothing below is valid then)
    int64_t n = 0; int S = 1;
    bool panel_tiles = false;  // the tile kernel factors a whole outer panel in one launch
    bool one_launch = false;   // ... and the whole matrix is one such panel, whatever its width
    bool look = false;         // look-ahead: the trailing update is split between the caller's stream and potrf_aux (PotrfCall::trailing_update)
    bool eager = false;        // L^-1 is formed next to the factorisation (PotrfCall::eager_row_block)
    int64_t split_rows = 0;    // an outer panel with at least this many block rows below it takes the split form (0: never)
    int64_t rbw = 0;           // eager: rows of a row block of the inverse

    int64_t panel_end(int64_t c0) const { return !one_launch && c0 + mxf_chol_tiles::NBO < n ? c0 + mxf_chol_tiles::NBO : n; }
    // does the outer panel at c0 take the split form (chain launch + rows-below launch)?
    bool split(int64_t c0) const { return panel_tiles && split_rows > 0 && (n - panel_end(c0)) / mxf_chol_tiles::NB >= split_rows; }
    // eager: row block [row_block_start(pe), pe) of L is final once the panel ending at pe has been factored (the rows above it in these columns are zero)
    bool fires_at(int64_t pe) const { return pe % rbw == 0 || pe == n; }
    int64_t row_block_start(int64_t pe) const { return (pe - 1) / rbw * rbw; }
    int64_t next_fire(int64_t pe) const {
        do pe = panel_end(pe); while (!fires_at(pe));
        return pe;
    }
};

// The tile kernel's workgroups hand tiles to each other through progress counters: every workgroup of a launch must be RESIDENT at once (one per
// CU: 256 threads at one wave per SIMD, ~76 KB of LDS), or a waiting workgroup could hold the CU its producer needs.  The grid (block rows x
// batch) is therefore bounded by the CU count of the device; larger problems take the launch-per-panel form.
static inline bool potrf_panel_tiles(const PotrfRequest& r) {
    using namespace mxf_chol_tiles;
    return r.esize == 8 && r.n % NB == 0 && r.n >= 2 * NB && r.S <= 64 && (int64_t)(r.n / NB) * r.S <= r.ncu;
}
static inline bool potrf_one_launch(const PotrfRequest& r) { return potrf_panel_tiles(r) && r.n <= r.one_max; }
// Look-ahead is possible at all (n >= 2048: at n = 8192 the 128 panel steps of 85 us each otherwise serialise with 3.7 ms of trailing GEMMs):
// only then does the launcher ask about the capture and, outside one, create the auxiliary streams.
static inline bool potrf_may_look(const PotrfRequest& r) { return r.n >= 2048 && !potrf_one_launch(r); }

// Eager inverse (a buffer for it, one matrix, whole outer panels, at least 16 of them and 4 row blocks): potrf(8192) is bound by its serial path
// (16 x (head update + chain + rows below)), the chip is ~40 % idle under it, and trtri(8192) afterwards took 3.9 ms of a 15 ms MAP step.
// DESIGN_HISTORY.md, "Variants measured and removed", has the other row-block widths.
static inline PotrfPlan potrf_plan(const PotrfRequest& r) {
    using namespace mxf_chol_tiles;
    PotrfPlan p;
    if (r.zero_upper && (p.refusal = chol_rows_refusal(r.n))) return p;
    p.n = r.n; p.S = r.S; p.split_rows = r.split_rows; p.rbw = r.eager_panels * NBO;
    p.panel_tiles = potrf_panel_tiles(r);
    p.one_launch = potrf_one_launch(r);
    p.look = potrf_may_look(r) && !r.capturing && r.aux_streams;
    p.eager = r.want_inverse && r.eager_panels && r.S == 1 && p.panel_tiles && p.look && r.n % NBO == 0 && r.n >= 16 * NBO && r.n >= 4 * p.rbw;
    return p;
}

// ---- trtri ----------------------------------------------------------------------------------------------------------------------------------
// Level 0 inverts all 64 x 64 diagonal blocks.  Merge level l = 0 .. trtri_levels(n) - 1 joins pairs of bs-row blocks (bs = NB << l) into their
// 2 bs-row inverse: `pairs` complete pairs from row 0 on, one batch; then, if the rows left over reach past one block, a ragged pair at
// ragged_at whose second block has ragged_b2 < bs rows (0: none; a single left-over block of <= bs rows waits for a later level).
struct TrtriLevel { int64_t bs = 0, pairs = 0, ragged_at = 0, ragged_b2 = 0; bool tri = false; };
static inline int trtri_levels(int64_t n) { int l = 0; while (((int64_t)mxf_chol_tiles::NB << l) < n) ++l; return l; }
static inline TrtriLevel trtri_level(int64_t n, int l) {
    const int64_t bs = (int64_t)mxf_chol_tiles::NB << l, pairs = n / (2 * bs), at = pairs * 2 * bs;
    return {bs, pairs, at, n - at > bs ? n - at - bs : 0, bs >= mxf_chol_tiles::TRI_MIN};
}
