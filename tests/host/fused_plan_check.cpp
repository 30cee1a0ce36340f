// Prints the plans of mxfusion_amd/csrc/fused_plan.h for every request read from standard input, one line each:
//   ps S n                                  ->  chunks grid
//   split S N R rb unit target              ->  ch rows
//   rff esize bwd S N D Q J ss_X ss_Om ss_ph ss_W has_X has_Om has_ph has_W has_out has_G has_dX
//       ->  rc qp jb npass ch rows grid[3] own_X summed scratch_sum n_prep n_out n_dx ss_om ss_ph ss_wb at_om at_ph at_wb at_acc zero_bytes bytes
//   kmv esize bwd S N N2 Q J ard ss_X ss_X2 ss_ls ss_var ss_da ss_V ss_A has_X has_X2 has_ls has_var has_da has_V has_out has_A has_w has_dls has_dvar
//       ->  rc qp jb npass square N2 ss_Z S_z S_V ch rows grid[3] gp n_prep_z n_out ss_zs ss_vb n_zero at_zs at_vb at_zero at_dv bytes
//           np0 items0 np_last items_last                  (kmv_prep_v of the first and of the last prep launch)
//   psi call esize S N M Q ard ss_mu ss_s ss_Z ss_ls ss_var has_mu has_s has_Z has_ls has_var has_Psi1 has_Psi2 has_G1 has_G2 has_dmu has_ds has_dZ
//       has_dls has_dvar J ss_A has_A has_R                                                          (call: 0 forward, 1 reverse, 2 contraction)
//       ->  rc qp n_prep n_mm grid1[3] rch grid_pairs[3] mch grid_rows[3] pairs_pass rows_pass wide fold close own_mu own_s own_Z own_l own_v
//           n_mu n_s n_Z npass n_out split at_z at_zh at_rows at_acc at_wt at_l2 at_dv at_big at_zero zero_bytes bytes
//   text 0|1                                ->  (nothing)  from here on rff / kmv / psi print "rc refusal" instead
// A refused request prints its rc and zeros.  tests/test_fused_plan_host.py compiles this with the system C++ compiler.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fused_plan.h"

typedef long long ll;
static bool text = false;

static bool read(std::vector<ll>& v, size_t n) {
    v.resize(n);
    for (ll& x : v) if (scanf("%lld", &x) != 1) return false;
    return true;
}
static void show(const FusedRefusal& p, std::vector<ll> cols) {
    if (text) { printf("%d %s\n", p.rc, p.refusal); return; }
    printf("%d", p.rc);
    for (ll c : cols) printf(" %lld", p.rc ? 0LL : c);
    printf("\n");
}

int main() {
    char what[16];
    std::vector<ll> v;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "text")) {
            if (!read(v, 1)) return 1;
            text = v[0] != 0;
        } else if (!strcmp(what, "ps")) {
            if (!read(v, 2)) return 1;
            const PerSamplePlan p = per_sample_plan((int)v[0], v[1]);
            printf("%d %u\n", p.chunks, p.grid);
        } else if (!strcmp(what, "split")) {
            if (!read(v, 6)) return 1;
            const ReduceSplit s = reduce_split((int)v[0], v[1], v[2], (int)v[3], (int)v[4], (int)v[5]);
            printf("%lld %d\n", (ll)s.ch, s.rows);
        } else if (!strcmp(what, "rff")) {
            if (!read(v, 18)) return 1;
            RffRequest r;
            r.esize = (size_t)v[0]; r.bwd = v[1] != 0; r.S = (int)v[2]; r.N = v[3]; r.D = v[4]; r.Q = (int)v[5]; r.J = (int)v[6];
            r.ss_X = v[7]; r.ss_Om = v[8]; r.ss_ph = v[9]; r.ss_W = v[10];
            r.has_X = v[11] != 0; r.has_Om = v[12] != 0; r.has_ph = v[13] != 0; r.has_W = v[14] != 0; r.has_out = v[15] != 0; r.has_G = v[16] != 0; r.has_dX = v[17] != 0;
            const RffPlan p = rff_plan(r);
            show(p, {p.qp, p.jb, p.npass, p.ch, p.rows, p.grid[0], p.grid[1], p.grid[2], p.own_X, p.summed, p.scratch_sum, p.n_prep, p.n_out, p.n_dx, p.ss_om,
                     p.ss_ph, p.ss_wb, (ll)p.at_om, (ll)p.at_ph, (ll)p.at_wb, (ll)p.at_acc, (ll)p.zero_bytes, (ll)p.bytes});
        } else if (!strcmp(what, "kmv")) {
            if (!read(v, 26)) return 1;
            KmvRequest r;
            r.esize = (size_t)v[0]; r.bwd = v[1] != 0; r.S = (int)v[2]; r.N = v[3]; r.N2 = v[4]; r.Q = (int)v[5]; r.J = (int)v[6]; r.ard = (int)v[7];
            r.ss_X = v[8]; r.ss_X2 = v[9]; r.ss_ls = v[10]; r.ss_var = v[11]; r.ss_da = v[12]; r.ss_V = v[13]; r.ss_A = v[14];
            r.has_X = v[15] != 0; r.has_X2 = v[16] != 0; r.has_ls = v[17] != 0; r.has_var = v[18] != 0; r.has_da = v[19] != 0; r.has_V = v[20] != 0;
            r.has_out = v[21] != 0; r.has_A = v[22] != 0; r.has_w = v[23] != 0; r.has_dls = v[24] != 0; r.has_dvar = v[25] != 0;
            const KmvPlan p = kmv_plan(r);
            KmvPrepV first = {0, 0}, last = {0, 0};
            if (!p.rc) {
                first = kmv_prep_v(p, 0);
                for (int pass0 = 0; pass0 < p.npass; pass0 += p.gp) last = kmv_prep_v(p, pass0);
            }
            show(p, {p.qp, p.jb, p.npass, p.square, p.N2, p.ss_Z, p.S_z, p.S_V, p.ch, p.rows, p.grid[0], p.grid[1], p.grid[2], p.gp, p.n_prep_z, p.n_out, p.ss_zs,
                     p.ss_vb, (ll)p.n_zero, (ll)p.at_zs, (ll)p.at_vb, (ll)p.at_zero, (ll)p.at_dv, (ll)p.bytes, first.np, first.items, last.np, last.items});
        } else if (!strcmp(what, "psi")) {
            if (!read(v, 30)) return 1;
            PsiRequest r;
            r.esize = (size_t)v[1]; r.S = (int)v[2]; r.N = v[3]; r.M = v[4]; r.Q = (int)v[5]; r.ard = (int)v[6];
            r.ss_mu = v[7]; r.ss_s = v[8]; r.ss_Z = v[9]; r.ss_ls = v[10]; r.ss_var = v[11];
            r.has_mu = v[12] != 0; r.has_s = v[13] != 0; r.has_Z = v[14] != 0; r.has_ls = v[15] != 0; r.has_var = v[16] != 0;
            r.has_Psi1 = v[17] != 0; r.has_Psi2 = v[18] != 0; r.has_G1 = v[19] != 0; r.has_G2 = v[20] != 0;
            r.has_dmu = v[21] != 0; r.has_ds = v[22] != 0; r.has_dZ = v[23] != 0; r.has_dls = v[24] != 0; r.has_dvar = v[25] != 0;
            r.J = (int)v[26]; r.ss_A = v[27]; r.has_A = v[28] != 0; r.has_R = v[29] != 0;
            const PsiPlan p = v[0] == 0 ? psi_fwd_plan(r) : (v[0] == 1 ? psi_bwd_plan(r) : psi_quad_plan(r));
            show(p, {p.qp, p.n_prep, p.n_mm, p.grid1[0], p.grid1[1], p.grid1[2], p.rch, p.grid_pairs[0], p.grid_pairs[1], p.grid_pairs[2], p.mch, p.grid_rows[0],
                     p.grid_rows[1], p.grid_rows[2], p.pairs_pass, p.rows_pass, p.wide, p.fold, p.close, p.own_mu, p.own_s, p.own_Z, p.own_l, p.own_v, p.n_mu,
                     p.n_s, p.n_Z, p.npass, p.n_out, p.split, (ll)p.at_z, (ll)p.at_zh, (ll)p.at_rows, (ll)p.at_acc, (ll)p.at_wt, (ll)p.at_l2, (ll)p.at_dv,
                     (ll)p.at_big, (ll)p.at_zero, (ll)p.zero_bytes, (ll)p.bytes});
        } else {
            return 1;
        }
    }
    return 0;
}
