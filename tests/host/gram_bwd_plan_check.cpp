// Prints the launch plans of mxfusion_amd/csrc/gram_bwd_plan.h for every request read from standard input, one per line:
//   g N N2 S QT PT elem_size lds_kb grid_target  ->  rb ct grid[0] grid[1] grid[2] lds_bytes grid_too_large
//   m M SB B grid_target                         ->  ct grid[0] grid[1] grid[2] full zacc dls3 mx centre Zs Xs Xn zero_bytes total_bytes refusal ("-": none)
// tests/test_gram_bwd_plan_host.py compiles this with the system C++ compiler and checks the invariants of the plans.
#include <stdio.h>

#include "gram_bwd_plan.h"

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'g') {
            long long N, N2, target;
            int S, QT, PT, elem, kb;
            if (scanf("%lld %lld %d %d %d %d %d %lld", &N, &N2, &S, &QT, &PT, &elem, &kb, &target) != 8) return 1;
            const GramBwdPlan p = gram_bwd_plan(N, N2, S, QT, PT, (size_t)elem, kb, target);
            printf("%lld %d %u %u %u %zu %d\n", (long long)p.rb, p.ct, p.grid[0], p.grid[1], p.grid[2], p.lds_bytes, (int)p.grid_too_large);
        } else if (what == 'm') {
            long long M, SB, B, target;
            if (scanf("%lld %lld %lld %lld", &M, &SB, &B, &target) != 4) return 1;
            const SvgpBwdMfmaPlan p = svgp_bwd_mfma_plan(M, SB, B, target);
            printf("%d %u %u %u %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %s\n", p.ct, p.grid[0], p.grid[1], p.grid[2], (int)p.full, p.zacc, p.dls3, p.mx,
                   p.centre, p.Zs, p.Xs, p.Xn, p.zero_bytes, p.total_bytes, p.refusal ? p.refusal : "-");
        } else {
            return 1;
        }
    }
    return 0;
}
