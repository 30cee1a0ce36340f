// Prints the plans of mxfusion_amd/csrc/pointwise_plan.h for every request read from standard input, one line each:
//   grid n      ->  grid_for grid_for_reduce
//   coldot S M N      ->  small g0 g1
//   reduce dtype kind bwd outer R inner has_x has_y has_dx      ->  rc empty spread rows by_wave items scratch grid
//   simplex dtype bwd dirichlet S B K ss_x ss_p sb_p one_hot labels has_x has_p has_out has_cot has_dp has_dx
//       ->  rc empty bucket p_atomic by_batch items n_sum grid
//   dense dtype bwd S N I O act ldx ss_x ss_w ss_b has_X has_W has_Y has_dY has_dX has_dW has_db      ->  rc empty tiles n_dw n_db by_rows grid
//   ewise dtype op rank bwd has_extent has_stride_x has_stride_y has_x has_y has_z has_dx has_dy e0..e4 sx0..sx4 sy0..sy4
//       ->  rc empty binary shared_x shared_y total chunks items numel_gx numel_gy wide_index sum_x sum_y inner_shared_x inner_shared_y grid
//           extent0..4 sx0..4 sy0..4 gx0..4 gy0..4
//   text 0|1     ->  (nothing)  from here on a request prints "rc refusal" instead
// A refused or empty request prints rc, empty and zeros.  tests/test_pointwise_plan_host.py compiles this with the system C++ compiler.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pointwise_plan.h"

typedef long long ll;

static bool read(std::vector<ll>& v) {
    for (ll& x : v) if (scanf("%lld", &x) != 1) return false;
    return true;
}
static void print(const PointwisePlan& p, bool text, const std::vector<ll>& cols) {
    if (text) { printf("%d %s\n", p.rc, p.refusal); return; }
    printf("%d %d", p.rc, (int)p.empty);
    for (ll c : cols) printf(" %lld", p.rc || p.empty ? 0LL : c);
    printf("\n");
}

int main() {
    char what[16];
    bool text = false;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "text")) {
            std::vector<ll> v(1);
            if (!read(v)) return 1;
            text = v[0] != 0;
        } else if (!strcmp(what, "grid")) {
            std::vector<ll> v(1);
            if (!read(v)) return 1;
            printf("%u %u\n", grid_for(v[0]), grid_for_reduce(v[0]));
        } else if (!strcmp(what, "coldot")) {
            std::vector<ll> v(3);
            if (!read(v)) return 1;
            const ColdotPlan p = coldot_plan((int)v[0], v[1], v[2]);
            printf("%d %u %u\n", (int)p.small, p.grid[0], p.grid[1]);
        } else if (!strcmp(what, "reduce")) {
            std::vector<ll> v(9);
            if (!read(v)) return 1;
            ReduceRequest r;
            r.dtype = (int)v[0]; r.kind = (int)v[1]; r.bwd = v[2] != 0; r.outer = v[3]; r.R = v[4]; r.inner = v[5];
            r.has_x = v[6] != 0; r.has_y = v[7] != 0; r.has_dx = v[8] != 0;
            const ReducePlan p = reduce_plan(r);
            print(p, text, {p.spread, p.rows, p.by_wave, p.items, p.scratch, p.grid});
        } else if (!strcmp(what, "simplex")) {
            std::vector<ll> v(17);
            if (!read(v)) return 1;
            SimplexRequest r;
            r.dtype = (int)v[0]; r.bwd = v[1] != 0; r.dirichlet = v[2] != 0; r.S = (int)v[3]; r.B = v[4]; r.K = (int)v[5];
            r.ss_x = v[6]; r.ss_p = v[7]; r.sb_p = v[8]; r.one_hot = v[9] != 0; r.labels = v[10] != 0;
            r.has_x = v[11] != 0; r.has_p = v[12] != 0; r.has_out = v[13] != 0; r.has_cot = v[14] != 0; r.has_dp = v[15] != 0; r.has_dx = v[16] != 0;
            const SimplexPlan p = simplex_plan(r);
            print(p, text, {p.bucket, p.p_atomic, p.by_batch, p.items, p.n_sum, p.grid});
        } else if (!strcmp(what, "dense")) {
            std::vector<ll> v(18);
            if (!read(v)) return 1;
            DenseRequest r;
            r.dtype = (int)v[0]; r.bwd = v[1] != 0; r.S = (int)v[2]; r.N = v[3]; r.I = (int)v[4]; r.O = (int)v[5]; r.act = (int)v[6];
            r.ldx = v[7]; r.ss_x = v[8]; r.ss_w = v[9]; r.ss_b = v[10];
            r.has_X = v[11] != 0; r.has_W = v[12] != 0; r.has_Y = v[13] != 0; r.has_dY = v[14] != 0; r.has_dX = v[15] != 0; r.has_dW = v[16] != 0;
            r.has_db = v[17] != 0;
            const DensePlan p = dense_plan(r);
            print(p, text, {p.tiles, p.n_dw, p.n_db, p.by_rows, p.grid});
        } else if (!strcmp(what, "ewise")) {
            std::vector<ll> v(12 + 3 * EW_RANK);
            if (!read(v)) return 1;
            int64_t e[EW_RANK], sx[EW_RANK], sy[EW_RANK];
            for (int d = 0; d < EW_RANK; ++d) { e[d] = v[12 + d]; sx[d] = v[12 + EW_RANK + d]; sy[d] = v[12 + 2 * EW_RANK + d]; }
            EwiseRequest r;
            r.dtype = (int)v[0]; r.op = (int)v[1]; r.rank = (int)v[2]; r.bwd = v[3] != 0;
            r.extent = v[4] ? e : nullptr; r.stride_x = v[5] ? sx : nullptr; r.stride_y = v[6] ? sy : nullptr;
            r.has_x = v[7] != 0; r.has_y = v[8] != 0; r.has_z = v[9] != 0; r.has_dx = v[10] != 0; r.has_dy = v[11] != 0;
            const EwisePlan p = ewise_plan(r);
            std::vector<ll> cols = {p.binary, p.shared_x, p.shared_y, p.total, p.chunks, p.items, p.numel_gx, p.numel_gy, p.wide_index, p.sum_x, p.sum_y,
                                    p.inner_shared_x, p.inner_shared_y, p.grid};
            for (const int64_t* a : {p.a.extent, p.a.sx, p.a.sy, p.a.gx, p.a.gy}) cols.insert(cols.end(), a, a + EW_RANK);
            print(p, text, cols);
        } else {
            return 1;
        }
    }
    return 0;
}
