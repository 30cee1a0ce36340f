// Prints the plans of mxfusion_amd/csrc/chol_plan.h for every request read from standard input, one per line:
//   potrf esize S n ncu capturing aux_streams want_inverse zero_upper one_max split_rows eager_panels
//     ->  "-" may_look panel_tiles one_launch look eager split_rows rbw npanels, then per outer panel (walking c0 = panel_end(c0)
//         from 0):  panel_end split,  and with eager, again per panel:  fires_at(pe) row_block_start(pe) next_fire(pe) (0 at pe == n)
//   trtri n
//     ->  "-" levels, then per merge level:  bs pairs ragged_at ragged_b2 tri
//   A refused request prints its refusal alone.
// tests/test_chol_plan_host.py compiles this with the system C++ compiler and checks the invariants of the plans.
#include <stdio.h>
#include <string.h>

#include "chol_plan.h"

int main() {
    char what[16];
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "potrf")) {
            int esize, S, ncu, cap, aux, inv, zu;
            long long n, one_max, split_rows, eager_panels;
            if (scanf("%d %d %lld %d %d %d %d %d %lld %lld %lld", &esize, &S, &n, &ncu, &cap, &aux, &inv, &zu, &one_max, &split_rows, &eager_panels) != 11) return 1;
            PotrfRequest r;
            r.esize = (size_t)esize; r.S = S; r.n = n; r.ncu = ncu; r.capturing = cap != 0; r.aux_streams = aux != 0; r.want_inverse = inv != 0;
            r.zero_upper = zu != 0; r.one_max = one_max; r.split_rows = split_rows; r.eager_panels = eager_panels;
            const PotrfPlan p = potrf_plan(r);
            if (p.refusal) { printf("%s\n", p.refusal); continue; }
            int np = 0;
            for (int64_t c0 = 0; c0 < n; c0 = p.panel_end(c0)) ++np;
            printf("- %d %d %d %d %d %lld %lld %d", (int)potrf_may_look(r), (int)p.panel_tiles, (int)p.one_launch, (int)p.look, (int)p.eager,
                   (long long)p.split_rows, (long long)p.rbw, np);
            for (int64_t c0 = 0; c0 < n; c0 = p.panel_end(c0)) printf(" %lld %d", (long long)p.panel_end(c0), (int)p.split(c0));
            if (p.eager)
                for (int64_t c0 = 0, pe; c0 < n; c0 = pe) {
                    pe = p.panel_end(c0);
                    printf(" %d %lld %lld", (int)p.fires_at(pe), (long long)p.row_block_start(pe), (long long)(pe < n ? p.next_fire(pe) : 0));
                }
            printf("\n");
        } else if (!strcmp(what, "trtri")) {
            long long n;
            if (scanf("%lld", &n) != 1) return 1;
            if (const char* why = chol_rows_refusal(n)) { printf("%s\n", why); continue; }
            printf("- %d", trtri_levels(n));
            for (int l = 0; l < trtri_levels(n); ++l) {
                const TrtriLevel v = trtri_level(n, l);
                printf(" %lld %lld %lld %lld %d", (long long)v.bs, (long long)v.pairs, (long long)v.ragged_at, (long long)v.ragged_b2, (int)v.tri);
            }
            printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
