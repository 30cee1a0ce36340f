// Grids, regimes, class buckets, index widths, scratch counts and refusals of the pointwise and per-row launchers that decide something
// (mxf_coldot of elementwise.hip, ewise.hip, simplex.hip, dense.hip) and the two grids every flat kernel is launched on, as pure functions of
// the request: plain C++, no HIP, checked on the host by tests/host/pointwise_plan_check.cpp.
// The flat entries of elementwise.hip, univariate.hip with unidist.h, mvn.hip, wishart.hip and transform.hip decide nothing beyond
// grid_for(n) and have no plan.
#pragma once
#include "fused_plan.h"      // FusedRefusal, mxf_cdiv, stride_ok

// kernels that end in ONE same-address atomic per workgroup (the scalar sums of normal_logpdf_kernel and univariate_logpdf_kernel): 2048 of them serialise at the L2
// (~15 ns apiece: 33 us for the 2 M-element log-pdf of a 4-sample step, of which the data take 6) -- two workgroups per CU
static inline unsigned grid_for_reduce(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > 512) b = 512;
    return (unsigned)b;
}

// grid-stride elementwise kernels without such an atomic
static inline unsigned grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (unsigned)b;
}

// What every plan below starts with: rc != 0, refused with that code and text; empty, nothing to do (the call returns 0); else launch.
struct PointwisePlan : FusedRefusal { bool empty = false; };
static inline bool bad_dtype(FusedRefusal& p, int dtype) {
    if (dtype != MXF_F32 && dtype != MXF_F64) p.refusef(-2, "bad dtype %d", dtype);
    return p.rc != 0;
}

// ---- elementwise.hip: mxf_coldot ---------------------------------------------------------------------------------------------------------
// small: coldot_small_kernel, a workgroup per 16 columns (few columns under many rows); else coldot_kernel, a thread per column
struct ColdotPlan { bool small; unsigned grid[2]; };
static inline ColdotPlan coldot_plan(int S, int64_t M, int64_t N) {
    const bool small = (int64_t)S * N < 16384 && M >= 64;
    return {small, {(unsigned)mxf_cdiv(N, small ? 16 : 256), (unsigned)S}};
}

// ---- ewise.hip: the broadcast map ------------------------------------------------------------------------------------------------------------
constexpr int EW_RANK = MXF_EW_MAX_RANK;
constexpr int64_t EW_LIMIT = (int64_t)1 << 35;        // elements of the output, and the span of an operand

struct EwAxes {
    int rank, op;
    int64_t extent[EW_RANK];
    int64_t sx[EW_RANK], sy[EW_RANK];      // operand strides in elements, 0: shared
    int64_t gx[EW_RANK], gy[EW_RANK];      // strides of the dense gradients (shared axes at extent 1), 0: shared
};
struct EwiseRequest {
    int dtype = MXF_F64, op = 0, rank = 0; bool bwd = false;
    const int64_t *extent = nullptr, *stride_x = nullptr, *stride_y = nullptr;      // host arrays of `rank` entries
    bool has_x = false, has_y = false, has_z = false, has_dx = false, has_dy = false;      // has_z: z, or dz of the reverse pass
};
struct EwisePlan : PointwisePlan {
    EwAxes a = {};
    bool binary = false, shared_x = false, shared_y = false;      // shared: over some axis of extent above 1
    int64_t total = 0, chunks = 0, items = 0;      // output elements; 16-byte chunks per innermost row; work items = total / inner * chunks
    int64_t numel_gx = 0, numel_gy = 0;            // elements of the dense gradients
    bool wide_index = false;                       // the kernels count items in 64 bits
    // reverse: the wanted gradient of a shared operand is summed in double (shared_grad.h), all terms of a chunk into one element
    bool sum_x = false, sum_y = false, inner_shared_x = false, inner_shared_y = false;
    unsigned grid = 1;
};

static inline EwisePlan ewise_plan(const EwiseRequest& r) {
    EwisePlan p;
    if (bad_dtype(p, r.dtype)) return p;
    if (r.op < 0 || r.op > 7) { p.refusef(-2, "op %d (0 add .. 7 log)", r.op); return p; }
    if (r.rank < 1) { p.refusef(-2, "rank %d", r.rank); return p; }
    if (r.rank > EW_RANK) { p.refusef(-3, "rank %d after merging; up to %d axes are supported", r.rank, EW_RANK); return p; }
    p.binary = r.op <= 4;
    if (!r.extent || !r.stride_x || !r.has_x || (p.binary && (!r.has_y || !r.stride_y))) { p.refuse(-2, "null operand, extent or stride array"); return p; }
    p.a.rank = r.rank; p.a.op = r.op;
    int64_t total = 1, span_x = 0, span_y = 0;
    for (int d = 0; d < r.rank; ++d) {
        const int64_t e = r.extent[d], sx = e > 1 ? r.stride_x[d] : 0, sy = p.binary && e > 1 ? r.stride_y[d] : 0;
        if (e < 0 || sx < 0 || sy < 0) { p.refusef(-2, "axis %d has extent %lld, strides %lld, %lld", d, (long long)e, (long long)sx, (long long)sy); return p; }
        if (e > EW_LIMIT || sx > EW_LIMIT || sy > EW_LIMIT) { p.refusef(-3, "axis %d is beyond 2^35 elements", d); return p; }
        p.a.extent[d] = e; p.a.sx[d] = sx; p.a.sy[d] = sy;
        if (e > 1 && sx == 0) p.shared_x = true;
        if (e > 1 && sy == 0 && p.binary) p.shared_y = true;
        if (e == 0) total = 0;
        else if (total > EW_LIMIT / e) { p.refuse(-3, "more than 2^35 elements"); return p; }
        else total *= e;
        span_x += e ? (e - 1) * sx : 0; span_y += e ? (e - 1) * sy : 0;
        if (span_x > EW_LIMIT || span_y > EW_LIMIT) { p.refuse(-3, "an operand spans more than 2^35 elements"); return p; }
    }
    p.total = total;
    if (total == 0) { p.empty = true; return p; }
    if (!r.has_z) { p.refuse(-2, r.bwd ? "null dz" : "null z"); return p; }
    const bool want_dx = r.bwd && r.has_dx, want_dy = r.bwd && r.has_dy && p.binary;      // (dy never under a unary op)
    if (r.bwd && !want_dx && !want_dy) { p.empty = true; return p; }
    // the dense gradients: row-major over the extents with the operand's shared axes at 1
    p.numel_gx = p.numel_gy = 1;
    for (int d = r.rank - 1; d >= 0; --d) {
        const bool own_x = p.a.extent[d] > 1 && p.a.sx[d] != 0, own_y = p.binary && p.a.extent[d] > 1 && p.a.sy[d] != 0;
        p.a.gx[d] = own_x ? p.numel_gx : 0;
        p.a.gy[d] = own_y ? p.numel_gy : 0;
        if (own_x) p.numel_gx *= p.a.extent[d];
        if (own_y) p.numel_gy *= p.a.extent[d];
    }
    const int last = r.rank - 1, V = r.dtype == MXF_F64 ? 2 : 4;
    const int64_t inner = p.a.extent[last];
    p.chunks = mxf_cdiv(inner, V);
    p.items = total / inner * p.chunks;
    p.wide_index = p.items >= ((int64_t)1 << 31);
    p.sum_x = want_dx && p.shared_x; p.sum_y = want_dy && p.shared_y;
    p.inner_shared_x = inner > 1 && p.a.sx[last] == 0; p.inner_shared_y = inner > 1 && p.a.sy[last] == 0;
    p.grid = p.sum_x || p.sum_y ? grid_for_reduce(p.items) : grid_for(p.items);      // (the sums end in atomics)
    return p;
}

// ---- ewise.hip: reductions behind the sample axis, x dense (outer, R, inner) -> y dense (outer, inner) ----------------------------------------
constexpr int64_t RED_WAVE_MAX = 512;      // inner == 1: a wave per row up to this R, a workgroup per row beyond

struct ReduceRequest {
    int dtype = MXF_F64, kind = 0; bool bwd = false;
    int64_t outer = 0, R = 0, inner = 0;
    bool has_x = false, has_y = false, has_dx = false;      // has_y: y, or dy of the reverse pass
};
// spread: reduce_spread_kernel (sum and mean, reverse); rows: the kernels of inner == 1, four rows per workgroup by_wave or one; else the
// column kernels.  items: what grid_for is handed (0 for rows); scratch: the doubles of the product's reverse pass
struct ReducePlan : PointwisePlan {
    bool spread = false, rows = false, by_wave = false;
    int64_t items = 0, scratch = 0;
    unsigned grid = 1;
};

static inline ReducePlan reduce_plan(const ReduceRequest& r) {
    ReducePlan p;
    if (bad_dtype(p, r.dtype)) return p;
    if (r.kind < 0 || r.kind > 2) { p.refusef(-2, "kind %d (0 sum, 1 mean, 2 prod)", r.kind); return p; }
    if (r.outer < 0 || r.R < 1 || r.inner < 0) { p.refusef(-2, "extents (%lld, %lld, %lld)", (long long)r.outer, (long long)r.R, (long long)r.inner); return p; }
    if (r.outer && r.inner && (r.outer > EW_LIMIT / r.inner || r.outer * r.inner > EW_LIMIT / r.R)) { p.refuse(-3, "more than 2^35 elements"); return p; }
    if (r.outer == 0 || r.inner == 0 || (r.bwd && !r.has_dx)) { p.empty = true; return p; }
    if (r.bwd ? !r.has_y || (r.kind == 2 && !r.has_x) : !r.has_x || !r.has_y) { p.refuse(-2, r.bwd ? "null x or dy" : "null x or y"); return p; }
    p.spread = r.bwd && r.kind != 2;
    p.rows = !p.spread && r.inner == 1;
    p.scratch = r.bwd && r.kind == 2 ? r.outer * r.R * r.inner : 0;
    if (p.rows) {
        p.by_wave = r.R <= RED_WAVE_MAX;
        const int64_t blocks = p.by_wave ? (r.outer + 3) / 4 : r.outer;
        p.grid = (unsigned)(blocks < 65536 ? blocks : 65536);
    } else {
        p.items = r.outer * r.inner * (p.spread ? r.R : 1);
        p.grid = grid_for(p.items);
    }
    return p;
}

// ---- simplex.hip -------------------------------------------------------------------------------------------------------------------------
struct SimplexRequest {
    int dtype = MXF_F64; bool bwd = false, dirichlet = false;
    int S = 0; int64_t B = 0; int K = 0;
    int64_t ss_x = 0, ss_p = 0, sb_p = 0;      // strides in elements, 0 = shared
    bool one_hot = false, labels = false;      // labels: x holds one element per row (the Categorical without one-hot encoding)
    bool has_x = false, has_p = false, has_out = false, has_cot = false, has_dp = false, has_dx = false;
};
// bucket: the lanes W that own a row.  Reverse: p_atomic, the parameter's gradient is summed over b in n_sum doubles (shared_grad.h);
// by_batch, a group owns b and loops over s; items: the groups' rows
struct SimplexPlan : PointwisePlan {
    int bucket = 0;
    bool p_atomic = false, by_batch = false;
    int64_t items = 0, n_sum = 0;
    unsigned grid = 1;
};

static inline SimplexPlan simplex_plan(const SimplexRequest& r) {
    SimplexPlan p;
    if (bad_dtype(p, r.dtype)) return p;
    if (r.K < 1) { p.refusef(-2, "K = %d classes, at least 1 is needed", r.K); return p; }
    if (r.bwd && !r.dirichlet && !r.one_hot && r.has_dx) { p.refuse(-2, "dx_acc must be null without one-hot encoding (a label has no gradient)"); return p; }
    if (r.S <= 0 || r.B <= 0) { p.empty = true; return p; }
    if (!r.has_x || !r.has_p) { p.refuse(-2, "null operand"); return p; }
    const int64_t dense_x = r.B * (r.labels ? 1 : r.K);
    if (!stride_ok(r.ss_x, dense_x)) { p.refusef(-2, "the sample stride of x is 0 or %lld (dense), got %lld", (long long)dense_x, (long long)r.ss_x); return p; }
    if (!stride_ok(r.sb_p, r.K)) { p.refusef(-2, "the batch stride of the parameter is 0 or K = %d, got %lld", r.K, (long long)r.sb_p); return p; }
    const int64_t dense_p = (r.sb_p ? r.B : 1) * r.K;
    if (!stride_ok(r.ss_p, dense_p)) { p.refusef(-2, "the sample stride of the parameter is 0 or %lld (dense), got %lld", (long long)dense_p, (long long)r.ss_p); return p; }
    if (r.bwd ? !r.has_cot : !r.has_out) { p.refuse(-2, r.bwd ? "null cotangent" : "null out"); return p; }
    if (r.bwd && !r.has_dp && !r.has_dx) { p.empty = true; return p; }
    p.bucket = r.K <= 4 ? 4 : (r.K <= 16 ? 16 : 64);
    p.p_atomic = r.bwd && r.has_dp && r.sb_p == 0 && r.B > 1;          // shared over b (the sum over s alone is by_batch's loop)
    p.by_batch = r.bwd && ((r.has_dp && !p.p_atomic && r.ss_p == 0 && r.S > 1) || (r.has_dx && r.ss_x == 0 && r.S > 1));
    p.items = p.by_batch ? r.B : (int64_t)r.S * r.B;
    p.n_sum = p.p_atomic ? (r.ss_p ? r.S : 1) * (int64_t)r.K : 0;
    p.grid = grid_for(p.items * p.bucket);
    return p;
}

// ---- dense.hip ---------------------------------------------------------------------------------------------------------------------------
constexpr int DENSE_MAX = 128;      // widths
static inline int dense_tile_rows(size_t esize) { return esize == 8 ? 16 : 32; }      // rows of a workgroup's tile (DenseTile of dense.hip)

struct DenseRequest {
    int dtype = MXF_F64; bool bwd = false;
    int S = 0; int64_t N = 0; int I = 0, O = 0, act = 0;
    int64_t ldx = 0, ss_x = 0, ss_w = 0, ss_b = 0;
    bool has_X = false, has_W = false, has_Y = false, has_dY = false, has_dX = false, has_dW = false, has_db = false;
};
// tiles: row tiles of one sample.  Reverse: by_rows, X is shared over the samples and dX is wanted, the workgroup owns a row tile and
// loops over s; n_dw, n_db: elements of dW (S|1, O, I) and db (S|1, O), summed in double whenever they are wanted
struct DensePlan : PointwisePlan {
    int64_t tiles = 0, n_dw = 0, n_db = 0;
    bool by_rows = false;
    unsigned grid = 1;
};

static inline DensePlan dense_plan(const DenseRequest& r) {
    DensePlan p;
    if (bad_dtype(p, r.dtype)) return p;
    if (r.I < 1 || r.O < 1 || r.I > DENSE_MAX || r.O > DENSE_MAX) { p.refusef(-3, "widths I = %d, O = %d; 1 .. %d are supported", r.I, r.O, DENSE_MAX); return p; }
    if (r.act < 0 || r.act > 3) { p.refusef(-2, "activation %d (0 identity, 1 tanh, 2 relu, 3 sigmoid)", r.act); return p; }
    if (r.S <= 0 || r.N <= 0) { p.empty = true; return p; }
    if (!r.has_Y || (r.bwd && !r.has_dY)) { p.refuse(-2, r.bwd ? "null Y or dY" : "null Y"); return p; }
    if (r.bwd && !r.has_dX && !r.has_dW && !r.has_db) { p.empty = true; return p; }
    if (!r.has_X || !r.has_W) { p.refuse(-2, "null operand"); return p; }
    if (r.ldx < r.I) { p.refusef(-2, "ldx = %lld < I = %d", (long long)r.ldx, r.I); return p; }
    if (r.ss_x != 0 && r.ss_x < (r.N - 1) * r.ldx + r.I) {
        p.refusef(-2, "the sample stride of X is 0 or at least (N - 1) ldx + I = %lld, got %lld", (long long)((r.N - 1) * r.ldx + r.I), (long long)r.ss_x);
        return p;
    }
    if (!stride_ok(r.ss_w, (int64_t)r.O * r.I)) { p.refusef(-2, "the sample stride of W is 0 or O I = %d (dense), got %lld", r.O * r.I, (long long)r.ss_w); return p; }
    if (!stride_ok(r.ss_b, r.O)) { p.refusef(-2, "the sample stride of b is 0 or O = %d, got %lld", r.O, (long long)r.ss_b); return p; }
    p.tiles = mxf_cdiv(r.N, dense_tile_rows(r.dtype == MXF_F64 ? 8 : 4));
    if (p.tiles * r.S > 0x7fffffffLL) { p.refusef(-2, "%lld row tiles x %d samples exceed the grid", (long long)p.tiles, r.S); return p; }
    p.by_rows = r.bwd && r.has_dX && r.ss_x == 0 && r.S > 1;
    p.n_dw = (r.ss_w ? r.S : 1) * (int64_t)r.O * r.I; p.n_db = (r.ss_b ? r.S : 1) * (int64_t)r.O;
    p.grid = (unsigned)(p.by_rows ? p.tiles : p.tiles * r.S);
    return p;
}
