// Log-densities of the univariate family (gfx950): Gamma, Gamma by mean and variance, Beta, Laplace, Uniform, Bernoulli, Normal by mean
// and precision.  Built like
// normal_logpdf_kernel (elementwise.hip): thread i owns element i for all S samples, per-element parameter gradients need no atomics,
// single-element parameters are block-reduced, one atomic per workgroup per scalar.  Launch-bound at the sizes of a prior.
//
// Replaces: Gamma / GammaMeanVariance.log_pdf_impl (components/distributions/gamma.py:45-59, :127-159), Beta.log_pdf_impl
// (beta.py:46-68), Laplace.log_pdf_impl (laplace.py:37-55), Uniform.log_pdf_impl (uniform.py:38-62), Bernoulli.log_pdf_impl
// (bernoulli.py:62-78), NormalMeanPrecision.log_pdf_impl (normal.py:266-284) + the sum(mean_S(.)) of
// models/factor_graph.py:223, and MXNet autograd through them.  The evaluation struct and the kernels are in unidist.h, which the per-sample
// Normal of elementwise.hip shares; mxf_univariate_logpdf_ps* are the per-sample sums of the score-function estimators (no reference
// counterpart: inference/score_function.py:70-77 multiplies two scalars that are sample means already).
#include "unidist.h"

namespace {

// argument checks shared by the entry points, then the launch
int run(mxf_handle h, const char* name, int kind, int dtype, const UniArgs& u, int mode, void* stream) {
    if (!h) return -1;
    if (u.n <= 0 || u.S <= 0) return 0;
    if (kind < MXF_D_GAMMA || kind > MXF_D_NORMAL_PREC) MXF_FAIL(h, -2, "%s: unknown distribution kind %d", name, kind);
    if (const int rc = uni_check(h, name, dtype, u)) return rc < 0 ? rc : 0;
    return mxf_typed(h, name, dtype, [&](auto t) {
        return dispatch<MXF_D_GAMMA, MXF_D_GAMMA_MV, MXF_D_BETA, MXF_D_LAPLACE, MXF_D_UNIFORM, MXF_D_BERNOULLI, MXF_D_NORMAL_PREC>(kind, [&](auto k) {
            uni_launch_kind<decltype(t), decltype(k)::value>(u, mode, (hipStream_t)stream);
            return 0;
        });
    });
}

}  // namespace

extern "C" int mxf_univariate_logpdf(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                     const void* b, int64_t n_b, double scale, void* out_acc, void* dx_acc, void* da_acc, void* db_acc,
                                     void* stream) {
    const UniArgs u = {.S = S, .n = n, .x = x, .a = a, .n_a = n_a, .b = b, .n_b = n_b, .scale = scale, .out = out_acc, .dx = dx_acc, .da = da_acc, .db = db_acc};
    return run(h, "mxf_univariate_logpdf", kind, dtype, u, UNI_REDUCED, stream);
}

extern "C" int mxf_univariate_logpdf_elem(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                          int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b, double scale, void* out,
                                          void* stream) {
    if (h && n > 0 && S > 0 && !out) MXF_FAIL(h, -2, "mxf_univariate_logpdf_elem: null out");
    const UniArgs u = {.S = S, .n = n, .x = x, .a = a, .n_a = n_a, .ss_a = strideS_a, .b = b, .n_b = n_b, .ss_b = strideS_b, .scale = scale, .out = out};
    return run(h, "mxf_univariate_logpdf_elem", kind, dtype, u, UNI_ELEM, stream);
}

extern "C" int mxf_univariate_logpdf_bwd(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                         int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b, const void* cot, double scale,
                                         void* dx_acc, void* da_acc, void* db_acc, void* stream) {
    if (h && n > 0 && S > 0 && !cot) MXF_FAIL(h, -2, "mxf_univariate_logpdf_bwd: null cotangent");
    const UniArgs u = {.S = S, .n = n, .x = x, .a = a, .n_a = n_a, .ss_a = strideS_a, .b = b, .n_b = n_b, .ss_b = strideS_b, .scale = scale, .cot = cot, .cs_s = n,
                       .cs_i = 1, .dx = dx_acc, .da = da_acc, .db = db_acc};
    return run(h, "mxf_univariate_logpdf_bwd", kind, dtype, u, UNI_REDUCED, stream);
}

extern "C" int mxf_univariate_logpdf_ps(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                        int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b, double scale, void* out_acc,
                                        void* stream) {
    if (h && n > 0 && S > 0 && !out_acc) MXF_FAIL(h, -2, "mxf_univariate_logpdf_ps: null out");
    const UniArgs u = {.S = S, .n = n, .x = x, .a = a, .n_a = n_a, .ss_a = strideS_a, .b = b, .n_b = n_b, .ss_b = strideS_b, .scale = scale, .out = out_acc};
    return run(h, "mxf_univariate_logpdf_ps", kind, dtype, u, UNI_PER_SAMPLE, stream);
}

extern "C" int mxf_univariate_logpdf_ps_bwd(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x, const void* a, int64_t n_a,
                                            int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b, const void* w, double scale,
                                            void* dx_acc, void* da_acc, void* db_acc, void* stream) {
    if (h && n > 0 && S > 0 && !w) MXF_FAIL(h, -2, "mxf_univariate_logpdf_ps_bwd: null weights");
    const UniArgs u = {.S = S, .n = n, .x = x, .a = a, .n_a = n_a, .ss_a = strideS_a, .b = b, .n_b = n_b, .ss_b = strideS_b, .scale = scale, .cot = w, .cs_s = 1,
                       .cs_i = 0, .dx = dx_acc, .da = da_acc, .db = db_acc};
    return run(h, "mxf_univariate_logpdf_ps_bwd", kind, dtype, u, UNI_REDUCED, stream);
}
