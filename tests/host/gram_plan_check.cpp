// Prints the launch plans of mxfusion_amd/csrc/gram_plan.h for every request read from standard input, one per line:
//   G kind elem_size S N N2 Q square sX sX2 sls vec_ok mode has_diag
//     ->  path QT tr ncb grid.x grid.y grid.z padr padc padx Sx Sz centre scen xs zs xn zn sxs szs sxn szn bytes has_diag rc refusal ("-": none)
//   P R Kn Q fused has_w Pw kb
//     ->  QT padr padk kbpb grid.x grid.y PT bytes rc refusal
// tests/test_gram_plan_host.py compiles this with the system C++ compiler and checks the invariants of the plans.
#include <stdio.h>

#include "gram_plan.h"

int main() {
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag == 'G') {
            int kind, elem, S, Q, square, vec, mode, diag;
            long long N, N2, sX, sX2, sls;
            if (scanf("%d %d %d %lld %lld %d %d %lld %lld %lld %d %d %d", &kind, &elem, &S, &N, &N2, &Q, &square, &sX, &sX2, &sls, &vec, &mode, &diag) != 13) return 1;
            const GramPlan p = gram_plan(kind, (size_t)elem, S, N, N2, Q, square != 0, sX, sX2, sls, vec != 0, mode, diag != 0);
            printf("%d %d %d %u %u %u %u %lld %lld %lld %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %zu %d %d %s\n", p.path, p.QT, p.tr, p.ncb,
                   p.grid[0], p.grid[1], p.grid[2], (long long)p.padr, (long long)p.padc, (long long)p.padx, p.Sx, p.Sz, p.centre, (long long)p.scen,
                   (long long)p.xs, (long long)p.zs, (long long)p.xn, (long long)p.zn, (long long)p.sxs, (long long)p.szs, (long long)p.sxn,
                   (long long)p.szn, p.bytes, p.has_diag, p.rc, p.refusal ? p.refusal : "-");
        } else if (tag == 'P') {
            int Q, fused, has_w, Pw;
            long long R, Kn, kb;
            if (scanf("%lld %lld %d %d %d %d %lld", &R, &Kn, &Q, &fused, &has_w, &Pw, &kb) != 7) return 1;
            const GramPlanesPlan p = gram_planes_plan(R, Kn, Q, fused != 0, has_w != 0, Pw, kb);
            printf("%d %lld %lld %d %u %u %d %zu %d %s\n", p.QT, (long long)p.padr, (long long)p.padk, p.kbpb, p.grid[0], p.grid[1], p.PT, p.bytes, p.rc,
                   p.refusal ? p.refusal : "-");
        } else {
            return 1;
        }
    }
    return 0;
}
