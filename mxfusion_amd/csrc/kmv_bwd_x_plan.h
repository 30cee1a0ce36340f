// The passes of the reverse mode of the matrix-free kernel product in its inputs (kmv_bwd_x.hip), as a pure function of the request: plain
// C++, no HIP.  A pass is one launch of kmv_bwd_x_kernel with its prep launches: its threads own the rows of one operand with one factor of
// the pair cotangent g = sum_j w_j A[n,j] V[m,j] and stream the other operand with the other, weighted factor.  Each pass is a kmv_plan of
// the reverse mode (fused_plan.h: <QP, JB>, the split of the streamed rows, the prepared operands) with the roles set as the pass needs.
//   rectangular   dX: rows of X with A, X2 and V streamed;  dX2: rows of X2 with V, X and A streamed
//   square        one fused pass, rows of X with A and V, X streamed with both weighted factors (g_nm + g_mn: a covariance per pair once);
//                 where that form would spill (kmv_bwd_x_fused) two passes into dX, rows of X with A, then rows of X with V
#pragma once
#include "fused_plan.h"

struct KmvBwdXRequest {
    size_t esize = 4;
    int S = 0; int64_t N = 0, N2 = 0; int Q = 0, J = 0, ard = 0;      // N2 is ignored on a square product (no X2)
    int64_t ss_X = 0, ss_X2 = 0, ss_ls = 0, ss_var = 0, ss_A = 0, ss_V = 0;
    bool has_X = false, has_X2 = false, has_ls = false, has_var = false, has_A = false, has_V = false, has_w = false, has_dX = false,
         has_dX2 = false;
};

struct KmvBwdXPass {
    KmvPlan k;                  // its N2: the streamed rows
    int64_t N = 0;              // the owned rows
    bool x2_side = false;       // the owned rows are X2's and the result is dX2's; otherwise X's and dX's
    bool own_V = false;         // the threads hold rows of V and stream the weighted A; otherwise rows of A and the weighted V
    bool fused = false;         // square: rows of A and of V, both weighted factors streamed
    int64_t S_U = 1, ss_ub = 0; // fused: samples and sample stride of the second prepared factor
    // the result (S_out, N, Q).  summed: through doubles acc (S, N, Q), zeroed where the streamed rows are split, which a closing launch adds
    // to the result, over S_sum samples in ascending order where the operand is shared
    int64_t S_out = 1, S_sum = 1, n_out = 0, n_acc = 0;
    bool summed = false, zeroed = false;
    size_t at_ub = 0, at_acc = 0, bytes = 0;
};

struct KmvBwdXPlan : FusedRefusal {
    int n = 0;
    KmvBwdXPass pass[2];
    size_t bytes = 0;           // the largest pass: the passes run one after the other in the same scratch
};

// whether the fused square kernel keeps its registers: all but float64 at JB = 16, whose two streamed blocks of factors alone are 64 of the
// 106 scalar registers (DESIGN.md 13 has the table)
constexpr bool kmv_bwd_x_fused(size_t esize, int qp, int jb) { return !(esize == 8 && jb == KMV_JB); }

static inline KmvBwdXPlan kmv_bwd_x_plan(const KmvBwdXRequest& r) {
    KmvBwdXPlan p;
    const bool square = !r.has_X2;
    // the pass whose threads own rows of X with A: it carries the checks of the shared operands
    KmvRequest q0 = {.esize = r.esize, .bwd = true, .S = r.S, .N = r.N, .N2 = r.N2, .Q = r.Q, .J = r.J, .ard = r.ard, .ss_X = r.ss_X,
                     .ss_X2 = r.ss_X2, .ss_ls = r.ss_ls, .ss_var = r.ss_var, .ss_V = r.ss_V, .ss_A = r.ss_A, .has_X = r.has_X, .has_X2 = r.has_X2,
                     .has_ls = r.has_ls, .has_var = r.has_var, .has_V = r.has_V, .has_A = r.has_A, .has_w = r.has_w, .has_dls = true};
    const KmvPlan k0 = kmv_plan(q0);
    if (k0.rc) { p.rc = k0.rc; snprintf(p.refusal, sizeof(p.refusal), "%s", k0.refusal); return p; }
    if (!r.has_dX && !r.has_dX2) { p.refuse(-2, "null dX_acc and dX2_acc"); return p; }
    if (square && r.has_dX2) { p.refuse(-2, "dX2_acc without an X2: the square product's gradient is dX_acc's"); return p; }
    const int64_t N2 = k0.N2;
    auto add = [&](const KmvPlan& k, int64_t N, int64_t ss_own, bool x2_side, bool own_V, bool fused) {
        KmvBwdXPass& a = p.pass[p.n++];
        a.k = k; a.N = N; a.x2_side = x2_side; a.own_V = own_V; a.fused = fused;
        a.S_out = ss_own ? r.S : 1; a.S_sum = ss_own ? 1 : r.S;
        a.n_out = a.S_out * N * r.Q;
        a.zeroed = k.rows > 1; a.summed = a.zeroed || a.S_sum > 1;
        a.n_acc = a.summed ? (int64_t)r.S * N * r.Q : 0;
        a.S_U = r.ss_A ? r.S : 1; a.ss_ub = a.S_U > 1 ? (int64_t)k.npass * k.N2 * k.jb : 0;
        Carver cv(nullptr);
        cv.off = k.bytes;
        a.at_ub = mxf_piece(cv, fused ? (size_t)(a.S_U * k.npass * k.N2) * k.jb * r.esize : 0);
        a.at_acc = mxf_piece(cv, (size_t)a.n_acc * sizeof(double));
        a.bytes = cv.off;
        if (a.bytes > p.bytes) p.bytes = a.bytes;
    };
    if (r.has_dX) {
        const bool fused = square && kmv_bwd_x_fused(r.esize, k0.qp, k0.jb);
        add(k0, r.N, r.ss_X, false, false, fused);
        if (square && !fused) {         // the same rows with V, the weighted A streamed
            KmvRequest q1 = q0;
            q1.ss_V = r.ss_A; q1.ss_A = r.ss_V;
            add(kmv_plan(q1), r.N, r.ss_X, false, true, false);
        }
    }
    if (r.has_dX2) {            // the roles exchanged, the centre still X2's first row
        KmvRequest q1 = q0;
        q1.N = N2; q1.N2 = r.N; q1.ss_X = r.ss_X2; q1.ss_X2 = r.ss_X; q1.ss_V = r.ss_A; q1.ss_A = r.ss_V; q1.ss_C = r.ss_X2;
        add(kmv_plan(q1), N2, r.ss_X2, true, true, false);
    }
    return p;
}
