// Prints the plan, the schedule and the scratch byte count of mxfusion_amd/csrc/svgp_plan.h for every request read from standard input:
//   plan esize kind S B M Q P sX sY nrows ncols ard want_grad use_mat form x_aligned16 psi2_ka psi2_ra ra_set psi2_rb rb_set
//     ->  rc use_mat ysamp het_stream het fused use_split whiten bt_path bt_wh het_split SS SYc lsn SB pl_big pl_h0 gp_scr t_blocked
//         KA reserve_a reserve_b few reserve_v reserve_phi scratch_bytes whitened_ok          (rc != 0: a refusal, the rest zero)
//   sweep, then fourteen lists "n v1 .. vn": esize kind S sX? sY? B M Q P noise want_grad form use_mat x_aligned16
//     ->  the same line for every element of the cross product, the last list fastest.  sX? / sY?: 0, or 1 for the contiguous stride;
//         noise: 0 (1,1), 1 (B,1), 2 (1,P), 3 (B,P), 4 a bad shape; ard = 1 and the default knobs
//   whitened_ok is svgp_whitened_ok(esize, S, B, M, Q, P, sX), the answer of mxf_svgp_whitened_ok.
// tests/test_svgp_plan_host.py compiles this with the system C++ compiler and checks the invariants of the plan.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "svgp_plan.h"

static void show(const SvgpRequest& r, const SvgpKnobs& k) {
    const SvgpPlan p = svgp_plan(r);
    const int wok = (int)svgp_whitened_ok(r.esize, r.S, r.B, r.M, r.Q, r.P, r.sX);
    if (p.refusal) { printf("%d 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 %d\n", p.rc, wok); return; }
    const SvgpSchedule s = svgp_psi2_schedule(p, k);
    Carver count(nullptr);      // the count pass of the launcher's carve_scratch
    if (r.esize == 4) { SvgpScratch<float> w = {}; w.carve(count, r, p); }
    else { SvgpScratch<double> w = {}; w.carve(count, r, p); }
    printf("0 %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %zu %zu %zu %d %lld %d %d %d %d %d %zu %d\n", (int)p.use_mat, (int)p.ysamp, (int)p.het_stream,
           (int)p.het, (int)p.fused, (int)p.use_split, (int)p.whiten, (int)p.bt_path, (int)p.bt_wh, (int)p.het_split, p.SS, p.SYc, p.lsn, (long long)p.SB,
           p.pl_big, p.pl_h0, p.gp_scr, p.t_blocked, (long long)s.KA, s.reserve_a, s.reserve_b, (int)s.few, s.reserve_v, s.reserve_phi, count.off, wok);
}

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "plan")) {
            long long v[21];
            for (long long& x : v) if (scanf("%lld", &x) != 1) return 1;
            SvgpRequest r;
            r.esize = (size_t)v[0]; r.kind = (int)v[1]; r.S = (int)v[2]; r.B = v[3]; r.M = v[4]; r.Q = (int)v[5]; r.P = (int)v[6]; r.sX = v[7]; r.sY = v[8];
            r.nrows = v[9]; r.ncols = (int)v[10]; r.ard = (int)v[11]; r.want_grad = (int)v[12]; r.use_mat = v[13] != 0; r.form = (int)v[14]; r.x_aligned16 = v[15] != 0;
            const SvgpKnobs k = {v[16], (int)v[17], v[18] != 0, (int)v[19], v[20] != 0};
            show(r, k);
        } else if (!strcmp(what, "sweep")) {
            std::vector<long long> ax[14];
            for (auto& a : ax) {
                int n;
                if (scanf("%d", &n) != 1) return 1;
                a.resize(n);
                for (long long& x : a) if (scanf("%lld", &x) != 1) return 1;
            }
            size_t i[14] = {};
            for (bool more = true; more;) {
                long long v[14];
                for (int a = 0; a < 14; ++a) v[a] = ax[a][i[a]];
                SvgpRequest r;
                r.esize = (size_t)v[0]; r.kind = (int)v[1]; r.S = (int)v[2]; r.B = v[5]; r.M = v[6]; r.Q = (int)v[7]; r.P = (int)v[8];
                r.sX = v[3] ? r.B * r.Q : 0; r.sY = v[4] ? r.B * r.P : 0;
                r.nrows = v[9] == 4 ? r.B + 1 : ((v[9] & 1) ? r.B : 1); r.ncols = (v[9] == 2 || v[9] == 3) ? r.P : 1;
                r.ard = 1; r.want_grad = (int)v[10]; r.form = (int)v[11]; r.use_mat = v[12] != 0; r.x_aligned16 = v[13] != 0;
                show(r, SvgpKnobs());
                more = false;
                for (int a = 13; a >= 0 && !more; --a) { if (++i[a] < ax[a].size()) more = true; else i[a] = 0; }
            }
        } else {
            return 1;
        }
    }
    return 0;
}
