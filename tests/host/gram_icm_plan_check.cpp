// Prints the plan of mxfusion_amd/csrc/gram_icm_plan.h for every request read from standard input, one per line:
//   bwd elem_size kind S N N2 Q T ard square has_X has_idx has_idx2 has_ls has_var has_B has_K want_dB sls svar sB ldk
//     ->  rc QT rb grid[0] grid[1] grid[2] lds_bytes row_min row_max col_min col_max dBp_bytes      (zeros after the code of a refusal)
// row_min / row_max: the fewest and the most bands that own one row, over all rows (gram_icm_rows); col_min / col_max the same for the column
// tiles (gram_icm_cols); dBp_bytes: the size of the per-lane dB words in the LDS layout.  With "text 1" as the first line a refusal prints
// "rc reason" instead.  tests/test_gram_icm_host.py compiles this with the system C++ compiler.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gram_icm_plan.h"

int main() {
    int text = 0;
    char word[16];
    const int NV = 22;
    long long v[NV];
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "text")) { if (scanf("%d", &text) != 1) return 1; continue; }
        if (sscanf(word, "%lld", &v[0]) != 1) return 1;
        for (int i = 1; i < NV; ++i) if (scanf("%lld", &v[i]) != 1) return 1;
        GramIcmRequest r;
        r.bwd = v[0] != 0; r.elem_size = (size_t)v[1]; r.kind = (int)v[2]; r.S = (int)v[3]; r.N = v[4]; r.N2 = v[5]; r.Q = (int)v[6]; r.T = (int)v[7];
        r.ard = v[8] != 0; r.square = v[9] != 0; r.has_X = v[10] != 0; r.has_idx = v[11] != 0; r.has_idx2 = v[12] != 0; r.has_ls = v[13] != 0;
        r.has_var = v[14] != 0; r.has_B = v[15] != 0; r.has_K = v[16] != 0; r.want_dB = v[17] != 0; r.sls = v[18]; r.svar = v[19]; r.sB = v[20]; r.ldk = v[21];
        const GramIcmPlan p = gram_icm_plan(r);
        if (p.rc) {
            if (text) printf("%d %s\n", p.rc, p.refusal); else printf("%d 0 0 0 0 0 0 0 0 0 0 0\n", p.rc);
            continue;
        }
        const int64_t N2 = r.square ? r.N : r.N2;
        std::vector<int> rows((size_t)r.N, 0), cols((size_t)N2, 0);
        int64_t a, b;
        for (unsigned by = 0; by < p.grid[1]; ++by) { gram_icm_rows(p, r.N, by, a, b); for (int64_t i = a; i < b; ++i) ++rows[(size_t)i]; }
        for (unsigned bx = 0; bx < p.grid[0]; ++bx) { gram_icm_cols(N2, bx, a, b); for (int64_t i = a; i < b; ++i) ++cols[(size_t)i]; }
        int rmin = rows[0], rmax = rows[0], cmin = cols[0], cmax = cols[0];
        for (int x : rows) { rmin = x < rmin ? x : rmin; rmax = x > rmax ? x : rmax; }
        for (int x : cols) { cmin = x < cmin ? x : cmin; cmax = x > cmax ? x : cmax; }
        printf("%d %d %lld %u %u %u %zu %d %d %d %d %zu\n", p.rc, p.QT, (long long)p.rb, p.grid[0], p.grid[1], p.grid[2], p.lds_bytes, rmin, rmax, cmin, cmax,
               p.dBs - p.dBp);
    }
    return 0;
}
