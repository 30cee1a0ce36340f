// Prints the plans of mxfusion_amd/csrc/fused_plan.h's knn and vecchia sections for every request read from standard input, one line each:
//   knn esize N Nc Q k causal has_X has_C has_idx same
//       ->  rc qp kp grid n_prep at_cp bytes
//   vecchia esize call Nt N Q P k has_Xt has_X has_Y has_nbr has_ls has_var has_noise has_mean has_vout has_value has_g has_dY
//       ->  rc qp rows grid n_acc at_acc zero_bytes bytes dy_bytes
//   text 0|1     ->  (nothing)  from here on a request prints "rc refusal" instead
// A refused request prints its rc and zeros.  tests/test_vecchia_host.py compiles this with the system C++ compiler.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fused_plan.h"

typedef long long ll;

static bool read(std::vector<ll>& v) {
    for (ll& x : v) if (scanf("%lld", &x) != 1) return false;
    return true;
}

static void print(int rc, const char* refusal, bool text, std::initializer_list<ll> cols) {
    if (text) { printf("%d %s\n", rc, refusal); return; }
    printf("%d", rc);
    for (ll c : cols) printf(" %lld", rc ? 0LL : c);
    printf("\n");
}

int main() {
    char what[16];
    bool text = false;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "text")) {
            ll t;
            if (scanf("%lld", &t) != 1) return 1;
            text = t != 0;
        } else if (!strcmp(what, "knn")) {
            std::vector<ll> v(10);
            if (!read(v)) return 1;
            KnnRequest r;
            r.esize = (size_t)v[0]; r.N = v[1]; r.Nc = v[2]; r.Q = (int)v[3]; r.k = (int)v[4]; r.causal = v[5] != 0;
            r.has_X = v[6] != 0; r.has_C = v[7] != 0; r.has_idx = v[8] != 0; r.same = v[9] != 0;
            const KnnPlan p = knn_plan(r);
            print(p.rc, p.refusal, text, {(ll)p.qp, (ll)p.kp, (ll)p.grid, (ll)p.n_prep, (ll)p.at_cp, (ll)p.bytes});
        } else if (!strcmp(what, "vecchia")) {
            std::vector<ll> v(19);
            if (!read(v)) return 1;
            VecchiaRequest r;
            r.esize = (size_t)v[0]; r.call = (int)v[1]; r.Nt = v[2]; r.N = v[3]; r.Q = (int)v[4]; r.P = (int)v[5]; r.k = (int)v[6];
            r.has_Xt = v[7] != 0; r.has_X = v[8] != 0; r.has_Y = v[9] != 0; r.has_nbr = v[10] != 0; r.has_ls = v[11] != 0; r.has_var = v[12] != 0;
            r.has_noise = v[13] != 0; r.has_mean = v[14] != 0; r.has_vout = v[15] != 0; r.has_value = v[16] != 0; r.has_g = v[17] != 0;
            r.has_dY = v[18] != 0;
            const VecchiaPlan p = vecchia_plan(r);
            print(p.rc, p.refusal, text, {(ll)p.qp, (ll)p.rows, (ll)p.grid, (ll)p.n_acc, (ll)p.at_acc, (ll)p.zero_bytes, (ll)p.bytes, (ll)p.dy_bytes});
        } else {
            return 1;
        }
    }
    return 0;
}
