// Prints the launch plan of mxfusion_amd/csrc/gemm_plan.h for every request read from standard input, one per line:
//   elem_size ta M N K batch lower_only reserve_cus tri vecA vecB beta small_kmax
//     ->  kernel tm tn ntiles splitk kchunk atomic nwg xc_max rev_m prescale tri_normalised rc refusal ("-": none)
// tri is the caller's value: the launcher's normalisation (gemm_tri_normalise) is applied here as it is there.
// tests/test_gemm_plan_host.py compiles this with the system C++ compiler and checks the invariants of the plans.
#include <stdio.h>

#include "gemm_plan.h"

int main() {
    int elem, ta, batch, lower, reserve, tri, vecA, vecB;
    long long M, N, K, kmax;
    double beta;
    while (scanf("%d %d %lld %lld %lld %d %d %d %d %d %d %lf %lld", &elem, &ta, &M, &N, &K, &batch, &lower, &reserve, &tri, &vecA, &vecB, &beta, &kmax) == 13) {
        const int t = gemm_tri_normalise(tri, ta);
        const GemmPlan p = gemm_plan((size_t)elem, M, N, K, batch, lower, reserve, t, vecA != 0, vecB != 0, beta, kmax);
        printf("%d %lld %lld %lld %d %lld %d %lld %lld %d %d %d %d %s\n", p.kernel, (long long)p.tm, (long long)p.tn, (long long)p.ntiles, p.splitk,
               (long long)p.kchunk, p.atomic, (long long)p.nwg, (long long)p.xc_max, p.rev_m, (int)p.prescale, t, p.rc, p.refusal ? p.refusal : "-");
    }
    return 0;
}
