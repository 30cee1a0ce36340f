// Prints the plan of mxfusion_amd/csrc/fused_plan.h's nearest section for every request read from standard input, one line each:
//   nearest esize step N M Q has_X has_C has_idx has_Cnew has_counts has_inertia alias
//       ->  rc qp grid n_prep n_close at_cp at_zero at_sums at_counts at_inertia zero_bytes bytes
//   text 0|1     ->  (nothing)  from here on a request prints "rc refusal" instead
// A refused request prints its rc and zeros.  tests/test_kmeans_host.py compiles this with the system C++ compiler.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fused_plan.h"

typedef long long ll;

int main() {
    char what[16];
    bool text = false;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "text")) {
            ll t;
            if (scanf("%lld", &t) != 1) return 1;
            text = t != 0;
        } else if (!strcmp(what, "nearest")) {
            std::vector<ll> v(12);
            for (ll& x : v) if (scanf("%lld", &x) != 1) return 1;
            NearestRequest r;
            r.esize = (size_t)v[0]; r.step = v[1] != 0; r.N = v[2]; r.M = v[3]; r.Q = (int)v[4];
            r.has_X = v[5] != 0; r.has_C = v[6] != 0; r.has_idx = v[7] != 0; r.has_Cnew = v[8] != 0; r.has_counts = v[9] != 0;
            r.has_inertia = v[10] != 0; r.alias = v[11] != 0;
            const NearestPlan p = nearest_plan(r);
            if (text) { printf("%d %s\n", p.rc, p.refusal); continue; }
            printf("%d", p.rc);
            for (ll c : {(ll)p.qp, (ll)p.grid, (ll)p.n_prep, (ll)p.n_close, (ll)p.at_cp, (ll)p.at_zero, (ll)p.at_sums, (ll)p.at_counts, (ll)p.at_inertia,
                         (ll)p.zero_bytes, (ll)p.bytes})
                printf(" %lld", p.rc ? 0LL : c);
            printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
