// Prints the plan of mxfusion_amd/csrc/gram_wide_plan.h for every request read from standard input, one per line:
//   bwd elem_size kind S N N2 Q square has_X has_ls has_var has_K ldk
//     ->  rc qc chunks grid[0] grid[1] grid[2] lds_bytes row_min row_max col_min col_max      (zeros after the code of a refusal)
// row_min / row_max: the fewest and the most row tiles that own one row (gram_wide_span); col_min / col_max the same for the column tiles.
// With "text 1" as the first line a refusal prints "rc reason" instead.  Compiled by tests/test_gram_wide_host.py.
#include <stdio.h>
#include <string.h>
#include <vector>

#include "gram_wide_plan.h"

static void cover(int64_t n, unsigned tiles, int& lo, int& hi) {
    std::vector<int> c((size_t)n, 0);
    int64_t a, b;
    for (unsigned t = 0; t < tiles; ++t) { gram_wide_span(n, t, a, b); for (int64_t i = a; i < b; ++i) ++c[(size_t)i]; }
    lo = hi = c[0];
    for (int x : c) { lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
}

int main() {
    int text = 0;
    char word[16];
    const int NV = 13;
    long long v[NV];
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "text")) { if (scanf("%d", &text) != 1) return 1; continue; }
        if (sscanf(word, "%lld", &v[0]) != 1) return 1;
        for (int i = 1; i < NV; ++i) if (scanf("%lld", &v[i]) != 1) return 1;
        GramWideRequest r;
        r.bwd = v[0] != 0; r.elem_size = (size_t)v[1]; r.kind = (int)v[2]; r.S = (int)v[3]; r.N = v[4]; r.N2 = v[5]; r.Q = (int)v[6]; r.square = v[7] != 0;
        r.has_X = v[8] != 0; r.has_ls = v[9] != 0; r.has_var = v[10] != 0; r.has_K = v[11] != 0; r.ldk = v[12];
        const GramWidePlan p = gram_wide_plan(r);
        if (p.rc) {
            if (text) printf("%d %s\n", p.rc, p.refusal); else printf("%d 0 0 0 0 0 0 0 0 0 0\n", p.rc);
            continue;
        }
        int rmin, rmax, cmin, cmax;
        cover(r.N, p.grid[1], rmin, rmax);
        cover(r.square ? r.N : r.N2, p.grid[0], cmin, cmax);
        printf("%d %d %d %u %u %u %zu %d %d %d %d\n", p.rc, p.qc, p.chunks, p.grid[0], p.grid[1], p.grid[2], p.lds_bytes, rmin, rmax, cmin, cmax);
    }
    return 0;
}
