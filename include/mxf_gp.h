/*
 * mxf_gp.h -- C ABI of libmxf_gp.so: the MI355X (gfx950) implementation of MXFusion's
 * Gaussian-process + SVI hot path.
 *
 * The reference (amzn/MXFusion v0.3.1) is pure Python on Apache MXNet; the arithmetic of this path
 * lives in MXNet operators called from four Python files.  Each entry point below names the
 * reference interface it replaces (file:line relative to the reference root).  The reference-side
 * binding a maintainer would add (a ctypes stub inside the reference's kernel / module classes) is
 * shown in INTEGRATION.md.
 *
 * Conventions (all entry points)
 *   - extern "C", plain pointers and sizes; no C++ / torch types.
 *   - return int status: 0 ok; <0 bad argument / runtime error (text via mxf_last_error);
 *     LAPACK-style "first non-PD leading minor" is reported asynchronously through a device-side
 *     int* info argument (never a host sync inside the library, like MXNet's lazy error).
 *   - the CALLER owns every data buffer (device pointers); the library owns only the opaque handle
 *     and its scratch workspace.  Row-major, leading sample axis S.  Strides are in ELEMENTS;
 *     a sample stride of 0 broadcasts that operand over S (the reference physically broadcasts,
 *     components/variables/runtime_variable.py:82-118).
 *   - dtype: MXF_F32 or MXF_F64 for every array of the call.
 *   - every call takes the hipStream_t (as void*) it is enqueued on and is asynchronous w.r.t. the host.
 *   - one handle per (thread, device); calls on one handle are not re-entrant.
 */
#ifndef MXF_GP_H
#define MXF_GP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mxf_ctx* mxf_handle;

enum { MXF_F32 = 0, MXF_F64 = 1 };

/* covariance-function kinds (components/distributions/gp/kernels/{rbf,matern,linear,static}.py) */
enum { MXF_K_RBF = 0, MXF_K_MATERN12 = 1, MXF_K_MATERN32 = 2, MXF_K_MATERN52 = 3,
       MXF_K_LINEAR = 4, MXF_K_BIAS = 5, MXF_K_WHITE = 6 };

/* how mxf_gram combines with the existing contents of K_out:
 * AddKernel / MultiplyKernel (kernels/add_kernel.py:44-68, multiply_kernel.py:44-67) */
enum { MXF_WRITE = 0, MXF_ACC_ADD = 1, MXF_ACC_MUL = 2 };

int mxf_version(void);
int mxf_create(int device, mxf_handle* out);
int mxf_destroy(mxf_handle h);
const char* mxf_last_error(mxf_handle h);
/* bytes of scratch currently held by the handle */
int64_t mxf_workspace_bytes(mxf_handle h);
/* Counts (re-)allocations of the handle's scratch.  The library owns its workspace and grows it on demand (hipFree + hipMalloc, never
 * inside a stream capture); a caller that captured launches into a hipGraph must re-capture when this number has changed, because the
 * captured kernels carry the old scratch addresses.  (The reference has no counterpart: MXNet owns its temporaries.) */
int64_t mxf_workspace_generation(mxf_handle h);
/* 1-norm condition number |Kuu + jitter I|_1 |(Kuu + jitter I)^-1|_1 of the last mxf_svgp_logpdf training call on this handle (both norms
 * are computed on the device next to the factorisation; this call copies them to the host, i.e. it synchronises).  The float32 streaming
 * form of the bound applies H0 = Kuu^-1 - Kuu^-1 Su Kuu^-1 explicitly, so its rounding error grows like cond * 2^-24: measured ELBO
 * agreement with float64 is 3e-6 at cond 1.4e3 and 2e-3 at 5e4 (tests/probes/f32_accuracy.py) -- above ~3e3 use float64.  0 if there was
 * no such call.  (No reference counterpart: svgp_regression.py:83-92 solves with the Cholesky factor, in whatever dtype the model has.) */
int mxf_svgp_last_cond(mxf_handle h, double* cond1_out);
/* The same quantity WITHOUT synchronising: the running maximum of the condition numbers that the training calls finished so far on this
 * handle have published (the last launch of every training call folds its cond_1 into one pinned, device-visible host word); reset != 0
 * clears it after the read.  A caller polls it every step for free and lags by at most the calls still in flight -- the float32 guard of
 * mxfusion_amd's SVGP module (automatic switch of the streaming stage to float64 above ~3e3) is built on it.  No reference counterpart. */
int mxf_svgp_cond_nowait(mxf_handle h, double* cond1_max_out, int reset);
/* Float32 streaming form of the NEXT mxf_svgp_logpdf / _sampled training calls on this handle, and the slot (0 <= cond_slot < 64) they
 * publish their condition number into.  MXF_SVGP_EXPLICIT (default): T = H0 Kuf with the explicit inverse H0 = Kuu^-1 - Kuu^-1 Su Kuu^-1
 * (two full-width split GEMMs; error ~ cond 2^-24).  MXF_SVGP_WHITENED: the factorised form the reference evaluates
 * (svgp_regression.py:83-92: trsm with the Cholesky factor) on the split GEMMs -- V = L^-1 Kuf (triangular product, written directly as
 * f16 planes), Phi = V V^T, T = L^-T (I - A_s A_s^T) V, U = (L^-1 mu)^T V -- three full-width products; every operand is bounded by
 * |L^-1| ~ sqrt(cond) and |v_n|^2 <= k_nn, so the float32 error grows like sqrt(cond) 2^-24 (ELBO 1e-7 at cond_2 1e5, 1e-6 at 4e6).
 * Applies to float32 training calls (want_grad) on shapes mxf_svgp_whitened_ok accepts; such a call on another shape fails with -3.
 * float64 calls ignore the form.  No reference counterpart (the reference has one dtype and one form).                                   */
enum { MXF_SVGP_EXPLICIT = 0, MXF_SVGP_WHITENED = 1 };
int mxf_svgp_configure(mxf_handle h, int form, int cond_slot);
/* 1 if the whitened float32 form covers this call shape (M % 128 == 0, S B % 256 == 0, Q <= 16, P <= 8, sampled X or S == 1), else 0 */
int mxf_svgp_whitened_ok(int dtype, int S, int64_t B, int64_t M, int Q, int P, int64_t strideS_X);
/* One slot's condition words without synchronising: the LAST value a finished call published into it and the running maximum (either
 * pointer may be NULL); reset != 0 clears both after the read.  A module instance that owns a slot sees its own Kuu only, whatever other
 * SVGP modules run on the same handle (mxf_svgp_cond_nowait = the maximum over all slots).                                               */
int mxf_svgp_cond_slot(mxf_handle h, int slot, double* last_out, double* max_out, int reset);
/* In-step durations of the bulk kernels of the LAST mxf_svgp_logpdf training call on this handle, measured with HIP events on the stream
 * each kernel runs on (enable with mxf_svgp_timing(h, 1); off by default).  mxf_svgp_timing_read synchronises the device and fills
 * ms_out[8] (-1 = not part of that call): [0] first Gram-planes pass (explicit form: Kuf planes; whitened: Kfu planes), [1] Psi2 / Phi
 * product, [2] second planes pass (explicit: Kfu planes + U; whitened: transposition of V + U), [3] T product, [4] fused reverse pass,
 * [5] the float64 core chain (Kuu ... H0 planes), [6] V = L^-1 Kuf (whitened), [7] the whole call on the caller's stream.
 * bench.py divides algorithmic bytes / flops by these (roofline_planes, step_breakdown_ms).  No reference counterpart.                  */
int mxf_svgp_timing(mxf_handle h, int enable);
int mxf_svgp_timing_read(mxf_handle h, double* ms_out);

/* out[0] = sum_i g[i] if the n values agree to 1e-6 relative, NaN otherwise.  The fused composites return the gradients of
 * gscale * sum_s logL[s] with ONE weight: the reverse-mode bridge uses this to scale them by the upstream gradient of mean_S(logL)
 * (factor_graph.py:233) and to poison the result -- on the device, no host sync -- if a caller weights the samples unequally.            */
int mxf_uniform_sum(mxf_handle h, int dtype, int64_t n, const void* g, void* out, void* stream);

/* MXNet SGD as driven by gluon.Trainer.step with optimizer='sgd' (the `optimizer` argument of batch_loop.py:29-44 is handed to the Trainer
 * by name): g = rescale_grad * grad + wd * w;  mom == NULL: w -= lr g;  else mom = momentum * mom - lr * g, w += mom.                     */
int mxf_sgd_step(mxf_handle h, int dtype, int64_t n, void* w, const void* g, void* mom, double lr, double momentum, double wd,
                 double rescale_grad, void* stream);

/* The other update rules gluon.Trainer is driven with by name through the same seam (batch_loop.py:46-49, minibatch_loop.py:71-74): MXNet 1.x
 * 'rmsprop' (non-centred), 'adagrad', 'adadelta', 'nag' on a flat buffer -- s1 / s2 are the optimiser's state buffers (n elements each,
 * zero-initialised by the caller; s2 only for adadelta), p1 = gamma1 / rho / momentum.  Rules in csrc/elementwise.hip (API knowledge of
 * MXNet; the reference holds no vector for them).                                                                                      */
#define MXF_OPT_RMSPROP 1
#define MXF_OPT_ADAGRAD 2
#define MXF_OPT_ADADELTA 3
#define MXF_OPT_NAG 4
int mxf_opt_step(mxf_handle h, int kind, int dtype, int64_t n, void* w, const void* g, void* s1, void* s2, double lr, double p1, double epsilon,
                 double wd, double rescale_grad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU gradient exchange (RCCL over xGMI), SURVEY.md section 8(b)/(e).  The reference has no multi-device path (one MXNet context
 * per Inference object); north_star shards the Monte-Carlo samples of StochasticVariationalInference.compute
 * (inference/variational.py:15-26) over the GPUs -- one process and one handle per GPU -- and sums the flat gradient ONCE per step
 * before the optimiser update (what Trainer.step of inference/batch_loop.py:46-60 would do with a kvstore).  librccl is opened on first
 * use; single-GPU callers never load it.
 *   mxf_comm_unique_id : rank 0 creates the 128-byte rendezvous id; the caller distributes it to the other ranks by its own means
 *                        (MPI, a file, the launcher's environment).
 *   mxf_comm_init      : collective over all ranks; binds a communicator of `nranks` ranks to this handle's device.
 *   mxf_allreduce_sum  : in-place sum over ranks of `count` elements (MXF_F32 / MXF_F64) at the device pointer `buf`, ordered on `stream`.
 *   mxf_bcast          : in-place broadcast from `root` (initial parameters; the minibatch permutation of config 4).
 *   mxf_comm_destroy   : releases the communicator (mxf_destroy does it too).
 * Returns 0, or < 0 with mxf_last_error (-6: librccl not loadable, -7: an RCCL call failed). */
#define MXF_COMM_ID_BYTES 128
int mxf_comm_unique_id(mxf_handle h, void* id_out /* MXF_COMM_ID_BYTES, host */);
int mxf_comm_init(mxf_handle h, int nranks, int rank, const void* id /* MXF_COMM_ID_BYTES, host */);
int mxf_allreduce_sum(mxf_handle h, int dtype, void* buf, int64_t count, void* stream);
int mxf_bcast(mxf_handle h, int dtype, void* buf, int64_t count, int root, void* stream);
int mxf_comm_destroy(mxf_handle h);

/* ---------------------------------------------------------------------------------------------
 * Gram build.  Replaces Kernel.K -> _compute_K (kernels/kernel.py:96-123), i.e.
 * StationaryKernel._compute_R2 (kernels/stationary.py:74-107) + RBF._compute_K (rbf.py:71-72) /
 * Matern{12,32,52}._compute_K (matern.py:84-88,116-120,148-151) / Linear (linear.py:59-89) /
 * Bias, White (static.py:56-74,125-150), fused into ONE pass that writes K once.
 *   X  : (S|1, N,  Q)   X2 : (S|1, N2, Q) or NULL (=> X2 = X, square Gram)
 *   lengthscale : (S|1, Q) if ard else (S|1, 1); for MXF_K_LINEAR it is `variances`; unused for BIAS/WHITE
 *   variance    : (S|1, 1)                       (unused for MXF_K_LINEAR)
 *   diag_add    : optional (S|1, 1) device scalar added to the diagonal (square Gram only):
 *                 the "+ eye*noise_var" of gp_regression.py:55-57;  jitter: host scalar, same place
 *                 (gp_regression.py:58-60, svgp_regression.py:70-72)
 *   K_out : (S, N, N2) with row stride ldk.
 * r^2 is evaluated as sum_q ((x_q - z_q)/l_q)^2 (difference form; the reference's expansion form
 * agrees to rounding in float64 and is less accurate in float32).                                  */
int mxf_gram(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q,
             const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
             const void* lengthscale, int ard, int64_t strideS_ls,
             const void* variance, int64_t strideS_var,
             const void* diag_add, int64_t strideS_diag, double jitter, int mode,
             void* K_out, int64_t ldk, int64_t strideS_K, void* stream);

/* K = k1(X, X2) + k2(X, X2) (op = MXF_ACC_ADD) or k1 * k2 (MXF_ACC_MUL) for TWO stationary kernels on the same inputs in ONE pass and ONE
 * write: AddKernel / MultiplyKernel._compute_K (kernels/add_kernel.py:44-68, multiply_kernel.py:44-67), which in the reference materialise
 * every sub-kernel's Gram and combine them (three N x N2 passes for two kernels).  Both covariances are formed from the same coordinate
 * differences (difference first, each kernel's length-scales after).  Arguments as mxf_gram, one (kind, lengthscale, ard, variance) set per
 * kernel; diag_add / jitter on the diagonal of a square Gram; Q <= 16.  Its reverse mode is mxf_gram_bwd per sub-kernel (ADD: with dK;
 * MUL: with dK * the other kernel's Gram).                                                                                              */
int mxf_gram2(mxf_handle h, int kind1, int kind2, int op, int dtype, int S, int64_t N, int64_t N2, int Q, const void* X, int64_t strideS_X,
              const void* X2, int64_t strideS_X2, const void* lengthscale1, int ard1, int64_t strideS_ls1, const void* variance1,
              int64_t strideS_var1, const void* lengthscale2, int ard2, int64_t strideS_ls2, const void* variance2, int64_t strideS_var2,
              const void* diag_add, int64_t strideS_diag, double jitter, void* K_out, int64_t ldk, int64_t strideS_K, void* stream);

/* Reverse mode of mxf_gram for the stationary kinds (what MXNet autograd does through
 * stationary.py:92-106 + rbf.py:71-72 / matern.py): given dK (S,N,N2) accumulates
 *   dX (S,N,Q), dX2 (S,N2,Q) [NULL when X2==NULL: both roles flow into dX], dls (S, Q|1), dvar (S,1).
 * Outputs are ACCUMULATED INTO (caller zeroes them); any output pointer may be NULL.               */
int mxf_gram_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q,
                 const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                 const void* lengthscale, int ard, int64_t strideS_ls,
                 const void* variance, int64_t strideS_var,
                 const void* dK, int64_t lddk, int64_t strideS_dK,
                 void* dX, void* dX2, void* dls, void* dvar, void* stream);

/* Gram build of the covariances that are NOT a function of one scaled distance: they work on the per-dimension differences
 * tau_d = x_d - x2_d, formed from the raw coordinates first (coincident rows give tau = 0 and an exact diagonal).  The reference has none
 * of them; the conventions are GPflow's / scikit-learn's (RQ) and Wilson & Adams 2013 (SpectralMixture).  Each kind takes three parameter
 * operands, each with its own sample stride (0: shared by the samples):
 *   kind             p0               p1                        p2                      K(tau)
 *   MXF_KD_PERIODIC  variance (S|1,1) lengthscale (S|1, Q|1)    period (S|1, Q|1)       p0 exp(-1/2 sum_d sin^2(pi tau_d / p2_d) / p1_d^2)
 *   MXF_KD_RQ        variance (S|1,1) lengthscale (S|1, Q|1)    alpha (S|1, 1)          p0 (1 + r2 / (2 p2))^-p2,  r2 = sum_d tau_d^2 / p1_d^2
 *   MXF_KD_SM        weights (S|1,A)  means (S|1, A, Q)         scales (S|1, A, Q)      sum_a p0_a exp(-2 pi^2 sum_d tau_d^2 p2_ad^2) prod_d cos(2 pi tau_d p1_ad)
 * (Q|1: Q values with ard, one without; ard and A are ignored where the table has no use for them.  Means are in cycles per unit of input.)
 * X, X2 (NULL: the square Gram), diag_add, jitter, K_out / ldk / strideS_K as mxf_gram; K_out is overwritten.  Limits: Q <= MXF_GD_MAX_Q for
 * PERIODIC and RQ, Q <= MXF_GD_SM_MAX_Q and A <= MXF_GD_SM_MAX_A for SM.  Status: -2 for an unknown kind or dtype, an extent < 1, a null
 * X / p0 / p1 / p2 / K_out, a negative stride or ldk < N2; -3 above a limit (checked before the pointers); no buffer is touched then.        */
enum { MXF_KD_PERIODIC = 0, MXF_KD_RQ = 1, MXF_KD_SM = 2 };
#define MXF_GD_MAX_Q 16
#define MXF_GD_SM_MAX_Q 8
#define MXF_GD_SM_MAX_A 8
int mxf_gram_diff(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int A,
                  const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                  const void* p0, int64_t strideS_p0, const void* p1, int64_t strideS_p1, const void* p2, int64_t strideS_p2, int ard,
                  const void* diag_add, int64_t strideS_diag, double jitter,
                  void* K_out, int64_t ldk, int64_t strideS_K, void* stream);

/* Its reverse mode: given dK (S, N, N2; row stride lddk) it recomputes K pair by pair and ACCUMULATES INTO dX (S|1, N, Q), dX2 (S|1, N2, Q)
 * [ignored when X2 == NULL: both roles flow into dX] and dp0, dp1, dp2, each laid out as its operand with its operand's sample stride -- a
 * shared operand's gradient is summed over the samples, a non-ard operand's over the dimensions (as mxf_gram_bwd).  The caller zeroes the
 * outputs; any of them may be NULL and its work is skipped.  dK need not be symmetric.  Status codes as mxf_gram_diff.                      */
int mxf_gram_diff_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int A,
                      const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                      const void* p0, int64_t strideS_p0, const void* p1, int64_t strideS_p1, const void* p2, int64_t strideS_p2, int ard,
                      const void* dK, int64_t lddk, int64_t strideS_dK,
                      void* dX, void* dX2, void* dp0, void* dp1, void* dp2, void* stream);

/* Gram build of the intrinsic coregionalisation model (multi-output GPs) in ONE pass and ONE write:
 *   K[s, i, j] = k_kind(x_i, x2_j) * B[s|0, idx[i], idx2[j]]
 * kind is MXF_K_RBF or MXF_K_MATERN12 / 32 / 52 with X, X2 (NULL: the square Gram), lengthscale, ard, variance, diag_add, jitter, K_out / ldk
 * / strideS_K as mxf_gram (K_out is overwritten; the distance is formed from the coordinate differences first, scaled after, as mxf_gram2).
 *   idx (N), idx2 (N2) : int32 output index of each row of X / X2, shared by the samples; idx2 is ignored on the square Gram (idx serves both
 *                        sides).  An index outside [0, T) is clamped into the range before it addresses B: a wrong value, never a read
 *                        outside B.  Validating the indices is the caller's business.
 *   B : (S|1, T, T) in the call's dtype, packed rows; strideS_B is 0 (shared) or T * T.  B need not be symmetric.
 * A sample stride of lengthscale is 0 or its row (Q with ard, else 1), of variance 0 or 1.  Limits: Q <= 16, T <= MXF_ICM_MAX_T.  Status: -2
 * for a non-stationary kind, a bad dtype, an extent < 1, a null operand, a negative stride, ldk < N2 or a parameter stride that is neither;
 * -3 above a limit (checked before the pointers); no buffer is touched then.                                                               */
#define MXF_ICM_MAX_T 32
int mxf_gram_icm(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int T,
                 const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2, const int32_t* idx, const int32_t* idx2,
                 const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                 const void* B, int64_t strideS_B, const void* diag_add, int64_t strideS_diag, double jitter,
                 void* K_out, int64_t ldk, int64_t strideS_K, void* stream);

/* Its reverse mode: given dK (S, N, N2; row stride lddk; not necessarily symmetric) it recomputes k pair by pair and ACCUMULATES INTO
 *   dX, dX2, dls, dvar : what mxf_gram_bwd gives for the cotangent dK[i, j] * B[idx[i], idx2[j]] (dX2 is ignored when X2 == NULL: both roles
 *                        flow into dX);
 *   dB[s|0, a, b] += sum over the pairs with idx[i] = a and idx2[j] = b of dK[s, i, j] * k(x_i, x2_j)   (laid out as B; on the square Gram
 *                        (a, b) and (b, a) receive their own pairs: nothing is symmetrised).
 * A gradient whose operand is shared by the samples is the sum over them.  dB, dls and dvar are summed in double for either dtype and
 * rounded once (float32: through scratch of the handle).  The caller zeroes the outputs; any of them may be NULL and its work is skipped.
 * Status codes as mxf_gram_icm; -4 when the scratch cannot be had.                                                                        */
int mxf_gram_icm_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int T,
                     const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2, const int32_t* idx, const int32_t* idx2,
                     const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                     const void* B, int64_t strideS_B, const void* dK, int64_t lddk, int64_t strideS_dK,
                     void* dX, void* dX2, void* dls, void* dvar, void* dB, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense building blocks (MXNet linalg.* call sites).  All batched over S with strides.  */

/* C = alpha*op(A)*op(B) + beta*C  -- linalg.gemm2 / linalg.syrk (svgp_regression.py:76,82,89,90 ...) */
int mxf_gemm(mxf_handle h, int dtype, int transA, int transB, int64_t M, int64_t N, int64_t K,
             double alpha, const void* A, int64_t lda, int64_t strideA,
             const void* B, int64_t ldb, int64_t strideB,
             double beta, void* C, int64_t ldc, int64_t strideC, int batch, void* stream);

/* The same product, C = alpha A B^T + beta C for k-contiguous float32 operands A (M x K), B (N x K), on the bf16 matrix pipe:
 * every f32 operand is split exactly into three bf16 terms and the six leading bf16 products accumulate in f32 (f32-equivalent
 * accuracy, 6/16 of the f32-MFMA cost; gemm_split.hip).  Replaces linalg.gemm2(A, B, False, True) / linalg.syrk call sites whose
 * operands are float32 (svgp_regression.py:88-107).  lower_only: only blocks / entries on or below the diagonal are written.     */
int mxf_gemm_f32x3(mxf_handle h, int64_t M, int64_t N, int64_t K, double alpha, const void* A, int64_t lda, const void* B, int64_t ldb,
                   double beta, void* C, int64_t ldc, int lower_only, void* stream);

/* The same product from TWO scaled f16 terms per operand and THREE matrix-pipe products (hi hi' + hi lo' + lo hi'; each operand is
 * scaled by the power of two that puts its largest magnitude at [2^13, 2^14), so the low term keeps its 11 bits over 2^18 of dynamic
 * range): the f32 MFMA's product accuracy at 3/16 of its cost.  This is the form the SVGP training step uses for Psi2 = Kuf Kuf^T and
 * T = H0 Kuf (MXF_SPLIT_MODE=bf16x3 selects the three-term form there).  Normwise f32 accuracy.
 * Supported range: the exponent of the scale is clamped to +-100, so the stated accuracy holds for an operand whose largest magnitude
 * lies in [2^-87, 2^114); a smaller maximum is scaled by 2^100 only and keeps fewer bits (its planes sit below 2^13), a larger one
 * overflows f16 from about 2^116.  A zero, denormal or non-finite maximum leaves the operand unscaled (scale 1).                       */
int mxf_gemm_f16x2(mxf_handle h, int64_t M, int64_t N, int64_t K, double alpha, const void* A, int64_t lda, const void* B, int64_t ldb,
                   double beta, void* C, int64_t ldc, int lower_only, void* stream);
/* Its two halves: mxf_f16x2_split writes the two planes of an (R x K) operand (2 * mxf_f32x3_plane_elems(R, K) 16-bit elements) and
 * the 32-bit word holding the bit pattern of max |X| (the operand's scale); mxf_gemm_f16x2_planes multiplies two split operands.
 * mxf_gemm_f16x2_planes only: lower_only = 2 writes the FULL product with C in 16-column blocks -- element (m, n) at
 * ((n / 16) * M + m) * 16 + n % 16, ldc ignored, N % 16 == 0, beta == 0 -- the layout the SVGP training step keeps T = H0 Kuf in.         */
int mxf_f16x2_split(mxf_handle h, int64_t R, int64_t K, const void* X, int64_t ld, void* planes, void* maxword, void* stream);
int mxf_gemm_f16x2_planes(mxf_handle h, int64_t M, int64_t N, int64_t K, double alpha, const void* A_planes, const void* A_maxword,
                          const void* B_planes, const void* B_maxword, double beta, void* C, int64_t ldc, int lower_only, void* stream);
/* The same product with the second operand stored the OTHER way round (r06): C (M x N) = alpha * A (M x K) * Bt (K x N), Bt_planes =
 * mxf_f16x2_split of the (K x N) matrix Bt itself (rows = contraction index).  The SVGP training step uses it for T = H0 Kuf on the SAME
 * planes of Kuf that Psi2 = Kuf Kuf^T reads (svgp_regression.py:85-90 needs Kuf in both roles; until r05 it was written twice).
 * M % 256 == 0, N % 256 == 0, K % 16 == 0, K >= 48.  blocked != 0: C in 16-column blocks (layout of lower_only = 2 above), else row-major
 * with ldc == N.  w (K floats) and U (N floats), both or neither: the same launch forms U[n] = sum_k w[k] Bt[k][n] (K <= 2048).          */
int mxf_gemm_f16x2_planes_kmajor(mxf_handle h, int64_t M, int64_t N, int64_t K, double alpha, const void* A_planes, const void* A_maxword,
                                 const void* Bt_planes, const void* Bt_maxword, void* C, int blocked, const void* w, void* U, void* stream);
/* Chained split products (the whitened SVGP tier, svgp_regression.py:83-92 in factorised float32 form):
 * mxf_gemm_f16x2_planes_out writes alpha * A B^T DIRECTLY as the two f16 planes (hi + lo, UNSCALED: the caller picks alpha so that the
 * largest magnitude sits near 2^13..2^14; as an operand of the next product its maxword is a word holding 8192.0f = scale 1) of the (M x N) operand whose contraction
 * index is its column -- element (m, n) at ((n / 16) * M + m) * 16 + n % 16 -- ready to be the operand of the next product; M % 128 == 0,
 * N % 256 == 0.  a_lower != 0: A is lower triangular (A[m][k] = 0 for k > m), the k loop of a row tile stops at its last row.
 * Ct_planes != NULL: the same launch ALSO writes the planes of the transposed (N x M) operand -- element (n, m) at
 * ((m / 16) * N + n) * 16 + m % 16 -- and, with a (M floats) and U (N floats) given, U[n] = sum_m a[m] (hi + lo)(m, n) in the planes' units
 * (what the whitened tier needs of V = L^-1 Kuf: V for Phi = V V^T, V^T for T = Hh V, a^T V for the mean term -- one pass).
 * mxf_f16x2_planes_transpose turns the planes of an (R x K) operand into those of its transpose (K x R) (R, K multiples of 64; 4 bytes
 * read + 4 written per element, HBM bound); U != NULL: the same pass forms U[k] = scale[0] * sum_r a[r] x(r, k) (a: R floats, scale: one
 * float, both on the device).                                                                                                            */
int mxf_gemm_f16x2_planes_out(mxf_handle h, int64_t M, int64_t N, int64_t K, double alpha, const void* A_planes, const void* A_maxword,
                              const void* B_planes, const void* B_maxword, void* C_planes, void* Ct_planes, const void* a, void* U,
                              int a_lower, void* stream);
int mxf_f16x2_planes_transpose(mxf_handle h, int64_t R, int64_t K, const void* planes_in, void* planes_out, const void* a, const void* scale,
                               void* U, void* stream);

/* The first stage of every float32 SVGP training step on its own: the Gram matrix cov(xmin[r], xmaj[k]) (r < R, k < Kn) of float32 inputs
 * under a stationary kind (RBF, Matern12/32/52), written DIRECTLY as the two f16 planes of the (R x Kn) operand (planes: 2 *
 * mxf_f32x3_plane_elems(R, Kn) 16-bit elements, 16-byte aligned; element (r, k) of a plane at ((k / 16) * R + r) * 16 + k % 16, the
 * columns Kn .. of the last 16-block zero).  The planes hold cov / variance * 2^14 as hi + lo (unit-variance covariances are <= 1, so the
 * format's power-of-two scale needs no reduction): dense = (hi + lo) * variance[0] * 2^-14, lo the exact f32 residual of hi rounded to f16.
 * Squared distances are formed difference first, scale after (sum_q (x_q - z_q)^2 (c / l_q)^2), so they do not depend on where the inputs
 * sit.  Xmin (R x Q), Xmaj (Kn x Q), lengthscale (Q if ard else 1), variance (1): device float32, contiguous; Q <= 16.
 *   w (Kn x Pw, 1 <= Pw <= 8) and U (Pw rows of ldU >= R floats), both or neither: the same pass forms U[p][r] = sum_k w[k][p] cov(r, k)
 *     (variance included) from the f32 covariances in registers, k in index order.
 *   majs / mins (each `period` device floats, or NULL): every covariance is multiplied by majs[k % period] and / or mins[r % period]
 *     before it is split and before it enters U -- the planes of K diag(s) / diag(s) K for the streaming heteroscedastic bound.
 * The padded copies of the coordinates live in the handle's Gram scratch (where mxf_gram keeps its pre-scaled ones): no caller buffer,
 * and like every handle call not re-entrant.  -2: bad shape, a null pointer, a non-stationary kind, period < 1, w without U; -3: Q > 16
 * or Pw > 8.  No reference counterpart (the reference materialises Kuf in float32, svgp_regression.py:73-75).                          */
int mxf_gram_planes(mxf_handle h, int kind, int64_t R, int64_t Kn, int Q, const void* Xmin, const void* Xmaj, const void* lengthscale,
                    int ard, const void* variance, void* planes, const void* w, int Pw, void* U, int64_t ldU, const void* majs,
                    const void* mins, int64_t period, void* stream);

/* The two halves of mxf_gemm_f32x3 for callers that reuse split operands (the SVGP step splits Kuf once for two products):
 * mxf_f32x3_split writes the three bf16 planes of an (R x K) float32 matrix (k16-blocked, see gemm_split.hip) into `planes`
 * (3 * mxf_f32x3_plane_elems(R, K) 16-bit elements); mxf_gemm_f32x3_planes multiplies two split operands.                         */
int64_t mxf_f32x3_plane_elems(int64_t R, int64_t K);
int mxf_f32x3_split(mxf_handle h, int64_t R, int64_t K, const void* X, int64_t ld, void* planes, void* stream);
int mxf_gemm_f32x3_planes(mxf_handle h, int64_t M, int64_t N, int64_t K, double alpha, const void* A_planes, const void* B_planes,
                          double beta, void* C, int64_t ldc, int lower_only, void* stream);

/* in-place lower Cholesky, strictly-upper part zeroed -- linalg.potrf (gp_regression.py:61,
 * svgp_regression.py:83-84).  info: device int[S], 0 or (1-based) index of the first bad pivot.   */
int mxf_potrf(mxf_handle h, int dtype, int S, int64_t n, void* A, int64_t lda, int64_t strideS_A,
              int* info, void* stream);

/* B <- op(L)^-1 B, L lower (n x n), B (n x nrhs) -- linalg.trsm(L,B,transpose)
 * (gp_regression.py:66,172; svgp_regression.py:85-87,153-156,164)                                   */
int mxf_trsm(mxf_handle h, int dtype, int transpose, int S, int64_t n, int64_t nrhs,
             const void* L, int64_t ldl, int64_t strideS_L, void* B, int64_t ldb, int64_t strideS_B,
             void* stream);

/* Linv <- L^-1 (lower) ; used for K^-1 = L^-T L^-1 in the closed-form gradients                    */
int mxf_trtri(mxf_handle h, int dtype, int S, int64_t n, const void* L, int64_t ldl, int64_t strideS_L,
              void* Linv, int64_t ldi, int64_t strideS_I, void* stream);

/* make_diagonal custom operator (mxfusion/util/customop.py:22-81): out (batch, n, n) = diag-embed of a (batch, n); mxf_diag_of is its
 * reverse mode, out (batch, n) = diagonal of g (batch, n, n) (customop.py:49-61).  Used for S = W W^T + make_diagonal(s)
 * (svgp_regression.py:76, :145).                                                                                                    */
int mxf_make_diagonal(mxf_handle h, int dtype, int64_t batch, int64_t n, const void* a, void* out, void* stream);
int mxf_diag_of(mxf_handle h, int dtype, int64_t batch, int64_t n, const void* g, void* out, void* stream);

/* out[s] = sum_i log|L_ii| -- linalg.sumlogdiag(abs(L)) (gp_regression.py:67)                       */
int mxf_sumlogdiag(mxf_handle h, int dtype, int S, int64_t n, const void* L, int64_t ldl, int64_t strideS_L,
                   void* out, void* stream);

/* out[s][n] = sum_m A[s][m][n]*B[s][m][n] -- F.sum(A*B, axis=-2) of the predictive variances
 * (gp_regression.py:181, svgp_regression.py:166-169, sparsegp_regression.py:153-155)                */
int mxf_coldot(mxf_handle h, int dtype, int S, int64_t M, int64_t N, const void* A, int64_t lda, int64_t strideS_A,
               const void* B, int64_t ldb, int64_t strideS_B, void* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Prediction composites (for a binder with no module code of its own; the Python mirror composes the same kernels).           */

/* Kernel.Kdiag: out (S, N) = diagonal of K(X[s], X[s]).  Stationary kinds, Bias, White: the variance (stationary.py:123-124,
 * static.py:76-86,152-162); Linear: sum_q variances_q x_q^2 with `lengthscale` carrying the variances (linear.py:91-104).           */
int mxf_kdiag(mxf_handle h, int kind, int dtype, int S, int64_t N, int Q, const void* X, int64_t strideS_X,
              const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
              void* out, void* stream);

/* GPRegressionMeanVariancePrediction.compute (gp_regression.py:146-196) for ONE posterior (L (N,N) lower, LinvY (N,P) as the inference
 * stored them, :203-234) and S samples of the test inputs X_test (S, Nt, Q): mean_out (S, Nt, P); var_out (S, Nt) -- the reference
 * broadcasts it over P -- or, full_cov, (S, Nt, Nt).  noise_free = 0 adds noise_var (1,).  Stationary kinds.                          */
int mxf_gp_predict(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t Nt, int Q, int P,
                   const void* X_cond, const void* X_test, const void* lengthscale, int ard, const void* variance,
                   const void* L, int64_t ldl, const void* LinvY, const void* noise_var, int noise_free, int full_cov,
                   void* mean_out, void* var_out, void* stream);

/* SVGPRegressionMeanVariancePrediction.compute (svgp_regression.py:121-189) from the variational parameters themselves: Z (M,Q),
 * qU_mean (M,P), qU_cov_W (M,M), qU_cov_diag (M,) (constrained values), S samples of X_test (S, Nt, Q).  Outputs as mxf_gp_predict;
 * info (2 ints, may be null): potrf status of Kuu + jitter I and of S = W W^T + diag.                                                */
int mxf_svgp_predict(mxf_handle h, int kind, int dtype, int S, int64_t M, int64_t Nt, int Q, int P,
                     const void* Z, const void* X_test, const void* lengthscale, int ard, const void* variance,
                     const void* qU_mean, const void* qU_cov_W, const void* qU_cov_diag, const void* noise_var,
                     double jitter, int noise_free, int full_cov, void* mean_out, void* var_out, void* info, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Elementwise / reduction pieces of the MC-ELBO loop.                                             */

/* y = log(1+exp(x)) and its reverse mode -- PositiveTransformation (var_trans.py:63-91)             */
int mxf_softplus_fwd(mxf_handle h, int dtype, int64_t n, const void* x, void* y, void* stream);
int mxf_softplus_bwd(mxf_handle h, int dtype, int64_t n, const void* x, const void* dy, void* dx_acc, void* stream);

/* x[s,i] = mean[i] + eps[s,i]*sqrt(var[i]) -- Normal.draw_samples_impl (normal.py:72-92); eps is the
 * caller-injected noise buffer (random_gen.py:26-28 seam).  n = elements per sample.               */
int mxf_normal_reparam(mxf_handle h, int dtype, int S, int64_t n, const void* mean, const void* var,
                       const void* eps, void* x, void* stream);

/* out += scale * sum_{s,i} logN(x[s,i] | mean[i], var[i])  (normal.py:52-70 then
 * factor_graph.py:223: sum(mean_S(.)) => scale = +-log_pdf_scaling/S), with wave-shuffle reductions;
 * optional reverse mode accumulated into dx (S,n), dmean (n), dvar (n) (all scaled by `scale`).
 * mean/var may be single-element broadcasts (n_mean, n_var in {1, n}).                            */
int mxf_normal_logpdf(mxf_handle h, int dtype, int S, int64_t n, const void* x,
                      const void* mean, int64_t n_mean, const void* var, int64_t n_var, double scale,
                      void* out_acc, void* dx_acc, void* dmean_acc, void* dvar_acc, void* stream);

/* reverse mode of mxf_normal_reparam: dmean += sum_s dx ; dvar += sum_s dx*eps/(2 sqrt(var))        */
int mxf_normal_reparam_bwd(mxf_handle h, int dtype, int S, int64_t n, const void* var, const void* eps,
                           const void* dx, void* dmean_acc, void* dvar_acc, void* stream);

/* x[s,i] = mean[i] + eps[s,i] / sqrt(precision[i]) -- NormalMeanPrecision.draw_samples_impl (normal.py:286-306); the operand layout of
 * mxf_normal_reparam: mean and precision flat with n elements, eps and x (S, n).  mxf_normal_reparam_prec_bwd is its reverse mode into
 * caller-zeroed buffers: dmean += sum_s dx ; dprecision += -1/2 sum_s dx * eps * precision^(-3/2); either may be null.                  */
int mxf_normal_reparam_prec(mxf_handle h, int dtype, int S, int64_t n, const void* mean, const void* precision,
                            const void* eps, void* x, void* stream);
int mxf_normal_reparam_prec_bwd(mxf_handle h, int dtype, int S, int64_t n, const void* precision, const void* eps,
                                const void* dx, void* dmean_acc, void* dprecision_acc, void* stream);

/* Variable transformations of several parameters in one launch (transform.hip): segment k of the flat buffers x, y holds sizes[k]
 * elements, one segment after the other, and is mapped by kinds[k] with the parameters p0[k], p1[k]:
 *   MXF_TR_SOFTPLUS  (p0 = offset)                  y = log(1 + exp(x)) + p0,  dy/dx = sigmoid(x)          Softplus (var_trans.py:53-91)
 *   MXF_TR_LOGISTIC  (p0 = lower, p1 = upper-lower) y = p0 + p1 sigmoid(x),    dy/dx = p1 s (1 - s)        Logistic (var_trans.py:105-147)
 * kinds, sizes, p0, p1 are HOST arrays of nseg entries read at call time (like the extent arrays of mxf_ewise_fwd): the segment table
 * travels in the kernel arguments, MXF_TR_MAX_SEG segments per launch (a longer list takes further launches), so a call makes no copy and
 * captures into a hipGraph.  sigmoid(x) is e / (1 + e) or 1 / (1 + e) with e = exp(-|x|), its slope e / (1 + e)^2 (no s (1 - s)
 * cancellation); an e below the smallest normal number counts as 0.  A Logistic y is clamped to [lower, upper] rounded inwards to the
 * working dtype: for |x| large y is the bound and the slope 0.  y is WRITTEN; mxf_transform_bwd adds dy * dy/dx into dx_acc.             */
enum { MXF_TR_SOFTPLUS = 0, MXF_TR_LOGISTIC = 1 };
#define MXF_TR_MAX_SEG 32
int mxf_transform_fwd(mxf_handle h, int dtype, int nseg, const int* kinds, const int64_t* sizes, const double* p0, const double* p1,
                      const void* x, void* y, void* stream);
int mxf_transform_bwd(mxf_handle h, int dtype, int nseg, const int* kinds, const int64_t* sizes, const double* p0, const double* p1,
                      const void* x, const void* dy, void* dx_acc, void* stream);

/* Log-densities of the univariate family, x the random variable, (a, b) the two parameters in the reference's order:
 *   MXF_D_GAMMA     (alpha, beta)      (a-1) log x - b x - lgamma(a) + a log b                      Gamma.log_pdf_impl (gamma.py:45-59)
 *   MXF_D_GAMMA_MV  (mean, variance)   Gamma with b = mean/variance, a = mean b                     GammaMeanVariance (gamma.py:127-159)
 *   MXF_D_BETA      (alpha, beta)      (a-1) log x + (b-1) log(1-x) - lgamma(a) - lgamma(b) + lgamma(a+b)   Beta.log_pdf_impl (beta.py:46-68)
 *   MXF_D_LAPLACE   (location, scale)  -log(2b) - |x-a|/b                                           Laplace.log_pdf_impl (laplace.py:37-55)
 *   MXF_D_UNIFORM   (low, high)        -log(b-a) where a <= x < b, else -inf                        Uniform.log_pdf_impl (uniform.py:38-62)
 *   MXF_D_BERNOULLI (prob_true, -)     x log a + (1-x) log(1-a); b is unused, pass a again          Bernoulli.log_pdf_impl (bernoulli.py:62-78)
 *   MXF_D_NORMAL_PREC (mean, precision)  (log b - log 2 pi) / 2 - b (x-a)^2 / 2                       NormalMeanPrecision.log_pdf_impl (normal.py:266-284)
 * mxf_univariate_logpdf has the contract of mxf_normal_logpdf: out += scale * sum_{s,i} log p(x[s,i] | a[i], b[i]) (factor_graph.py:223),
 * optional reverse mode accumulated into dx (S,n), da (n_a), db (n_b), all scaled by `scale`; n_a, n_b in {1, n}; any output may be null.
 * Gradients are closed forms (digamma for the Gamma and Beta parameters; GAMMA_MV chained to mean and variance; Laplace d/dx =
 * -sign(x-a)/b with sign(0) = 0; Uniform dx = 0, da = 1/(b-a), db = -1/(b-a) inside the support; outside it nothing is added to any
 * gradient, whatever the weight; Bernoulli dx = log a - log(1-a), da = x/a - (1-x)/(1-a), db = 0; NORMAL_PREC dx = -b (x-a), da = b (x-a),
 * db = (1/b - (x-a)^2) / 2).  A sum that holds an element outside the Uniform's support is -inf for scale > 0, +inf for scale < 0
 * and NaN (0 * inf) for scale == 0.                                                                                                    */
enum { MXF_D_GAMMA = 0, MXF_D_GAMMA_MV = 1, MXF_D_BETA = 2, MXF_D_LAPLACE = 3, MXF_D_UNIFORM = 4, MXF_D_BERNOULLI = 5, MXF_D_NORMAL_PREC = 6 };
int mxf_univariate_logpdf(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x,
                          const void* a, int64_t n_a, const void* b, int64_t n_b, double scale,
                          void* out_acc, void* dx_acc, void* da_acc, void* db_acc, void* stream);

/* The un-reduced log-density that Distribution.log_pdf returns: out[s,i] = scale * log p(x[s,i] | a, b), WRITTEN.  A parameter has no
 * sample axis (strideS = 0, n_a in {1, n}) or a full one (strideS = n, n_a = n: a is (S,n)).  Forward only.                            */
int mxf_univariate_logpdf_elem(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x,
                               const void* a, int64_t n_a, int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b,
                               double scale, void* out, void* stream);

/* Reverse mode of mxf_univariate_logpdf_elem -- the reduced kernel's gradients with the cotangent cot (S,n) in the place of `scale`:
 * dx[s,i] += scale * cot[s,i] * dlogp/dx, and likewise da, db: summed over s for a parameter without sample axis ((n_a) elements, a
 * single-element one also over i), (S,n) for a parameter with one.  Any output may be null.                                            */
int mxf_univariate_logpdf_bwd(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x,
                              const void* a, int64_t n_a, int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b,
                              const void* cot, double scale, void* dx_acc, void* da_acc, void* db_acc, void* stream);

/* Per-sample sums for the score-function estimators (Ranganath et al. 2014, Algorithm 1): out[s] += scale * sum_i log p(x[s,i] | a, b) for
 * s < S, out (S) ACCUMULATED INTO (caller zeroes it, like the reduced kernels).  x is (S, n); a parameter is a single element
 * (n_a = 1, strideS = 0), per element (n_a = n, strideS = 0) or per sample and element (n_a = n, strideS = n) -- the layouts of
 * mxf_univariate_logpdf_elem.  The reduced entry points bake the 1/S mean of factor_graph.py:223 into ONE scalar (factor_graph.py:192-238);
 * an estimator that weights each sample by f_s = log p - log q needs the S values apart.  The reference's own ScoreFunctionInference
 * (inference/score_function.py:70-77) multiplies two values that are sample means already and has no per-sample quantity to replace;
 * mxfusion_amd/inference/score_function.py implements the paper's estimator on these.  A sample with an element outside the Uniform's
 * support gets -inf (scale > 0); the other samples are not touched by it.
 * mxf_univariate_logpdf_ps_bwd is the reverse mode with the per-sample weights w (S elements, device, dtype of the call):
 * dx[s,i] += scale * w[s] * dlogp/dx, and likewise da, db -- summed over s for a parameter without sample axis ((n_a) elements, a
 * single-element one also over i), (S,n) for a parameter with one.  Any output may be null.  The support rules of mxf_univariate_logpdf
 * hold unchanged (outside the Uniform's support nothing is added; Laplace sign(0) = 0; Bernoulli db = 0).                              */
int mxf_univariate_logpdf_ps(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x,
                             const void* a, int64_t n_a, int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b,
                             double scale, void* out_acc, void* stream);
int mxf_univariate_logpdf_ps_bwd(mxf_handle h, int kind, int dtype, int S, int64_t n, const void* x,
                                 const void* a, int64_t n_a, int64_t strideS_a, const void* b, int64_t n_b, int64_t strideS_b,
                                 const void* w, double scale, void* dx_acc, void* da_acc, void* db_acc, void* stream);

/* The same pair for the Normal by mean and variance (Normal.log_pdf_impl, normal.py:52-70): out[s] += scale * sum_i logN(x[s,i] | mean,
 * var), and dx, dmean, dvar += scale * w[s] * dlogN/d(.).  Unlike mxf_normal_logpdf, mean and var may carry a sample axis (strideS = n):
 * the likelihood whose mean is a function of sampled latent variables, r = f(x; w_s) of shape (S, N, 1), is the large operand of this
 * path.                                                                                                                                 */
int mxf_normal_logpdf_ps(mxf_handle h, int dtype, int S, int64_t n, const void* x,
                         const void* mean, int64_t n_mean, int64_t strideS_mean, const void* var, int64_t n_var, int64_t strideS_var,
                         double scale, void* out_acc, void* stream);
int mxf_normal_logpdf_ps_bwd(mxf_handle h, int dtype, int S, int64_t n, const void* x,
                             const void* mean, int64_t n_mean, int64_t strideS_mean, const void* var, int64_t n_var, int64_t strideS_var,
                             const void* w, double scale, void* dx_acc, void* dmean_acc, void* dvar_acc, void* stream);

/* Expected log-likelihood of a non-Gaussian observation model under Gaussian marginals, the data term of the sparse variational GP bound
 *   ELBO = c sum_{n,p} E_{N(f; m[n,p], v[n])}[log p(y[n,p] | f)] - KL(q(u) || p(u))
 * (Hensman, Matthews, Ghahramani 2015, "Scalable Variational Gaussian Process Classification").  No reference counterpart: the reference's
 * SVGP is regression with Gaussian noise only (svgp_regression.py:43-109).  With g(f) = log p(y | f) and mu(f) = E[y | f]:
 *   MXF_LIK_BERNOULLI_LOGIT   y in {0, 1}      g = log sigmoid((2y - 1) f)           mu = sigmoid(f)
 *   MXF_LIK_BERNOULLI_PROBIT  y in {0, 1}      g = log Phi((2y - 1) f)               mu = Phi(f)
 *   MXF_LIK_POISSON_EXP       y = 0, 1, 2, ... g = y f - exp(f) - lgamma(y + 1)      mu = exp(f)
 * all finite and accurate over |f| <= 40 in both precisions (mxfusion_amd/csrc/likelihood.h has the tail forms).
 * The expectation is Gauss-Hermite quadrature: nodes and weights are HOST arrays of nq <= MXF_LIK_MAX_NODES doubles, the rule of
 * numpy.polynomial.hermite.hermgauss as it comes (weight function exp(-x^2)); E[g] ~ sum_k w_k / sqrt(pi) g(m + sqrt(2 max(v, 0)) x_k).
 * They travel in the kernel arguments: a call allocates nothing, copies nothing and captures into a hipGraph.  A negative v counts as 0.
 * y (S|1, n, P), m (S|1, n, P) and v (S|1, n), the variance of a row shared by its P columns, are dense; strideS_* is the sample stride in
 * elements (n P, n P, n), or 0 for an operand shared by the S samples -- shared labels under sampled m, v is the common case.
 *
 * mxf_lik_expect: out[s] += scale * sum_{i,p} E[g], out (S) ACCUMULATED INTO, and in the same pass the reverse mode, also accumulated, with
 * w = scale, or scale * cot[s] given the per-sample weights cot (S, device, dtype of the call):
 *   dm[s,i,p] += w sum_k w_k g'(f_k)            the exact derivative of the quadrature sum
 *   dv[s,i]   += w / 2 sum_p sum_k w_k g''(f_k)  Price's theorem, d/dv E[g] = E[g''] / 2
 * The Price form is the derivative of the exact expectation, so it differs from the derivative of the quadrature sum by the quadrature
 * error (1e-6 of the value at nq = 20 for |m| <= 3, v <= 4; tests/test_likelihood_host.py has the figure); the chain rule through
 * sqrt(v) is 0 / 0 at v = 0 and loses four digits of a float32 at v = 1e-8.  dm (S, n, P) and dv (S, n) always carry the sample axis:
 * the caller of a shared m or v sums them over s.  out, dm, dv may each be null.
 * mxf_lik_expect_elem: out[s,i,p] = scale * E[g], (S, n, P), WRITTEN.  Forward only.
 * mxf_lik_moments: e1[s,i,p] = E[mu(f)], e2[s,i,p] = E[mu(f)^2], (S, n, P), WRITTEN: the predictive mean E[y] = e1 and variance
 * e1 - e1^2 (Bernoulli kinds) or e1 + e2 - e1^2 (Poisson).                                                                              */
enum { MXF_LIK_BERNOULLI_LOGIT = 0, MXF_LIK_BERNOULLI_PROBIT = 1, MXF_LIK_POISSON_EXP = 2 };
#define MXF_LIK_MAX_NODES 64
int mxf_lik_expect(mxf_handle h, int kind, int dtype, int S, int64_t n, int P, const void* y, int64_t strideS_y,
                   const void* m, int64_t strideS_m, const void* v, int64_t strideS_v, int nq, const double* nodes, const double* weights,
                   const void* cot, double scale, void* out_acc, void* dm_acc, void* dv_acc, void* stream);
int mxf_lik_expect_elem(mxf_handle h, int kind, int dtype, int S, int64_t n, int P, const void* y, int64_t strideS_y,
                        const void* m, int64_t strideS_m, const void* v, int64_t strideS_v, int nq, const double* nodes,
                        const double* weights, double scale, void* out, void* stream);
int mxf_lik_moments(mxf_handle h, int kind, int dtype, int S, int64_t n, int P, const void* m, int64_t strideS_m,
                    const void* v, int64_t strideS_v, int nq, const double* nodes, const double* weights, void* e1, void* e2, void* stream);

/* Robust-max, the multi-class likelihood of the sparse variational GP (Hernandez-Lobato et al. 2011): C latent functions per row, a label
 * y in {0 .. C-1}, p(y | f) = 1 - eps where f_y is the largest of the row and eps / (C - 1) otherwise.  No reference counterpart.  Under
 * independent marginals f_c ~ N(m[c], v), one v per row,
 *   p = P(f_y is the largest) ~ sum_k w_k / sqrt(pi) prod_{c != y} Phi((m[y] - m[c]) / sqrt(v_eff) + sqrt(2) x_k),   v_eff = max(v, 1e-12)
 *   E[log p(y | f)] = L0 + p (L1 - L0),   L1 = log(1 - eps),   L0 = log(eps / (C - 1))
 * with nodes and weights as in mxf_lik_expect (host arrays, nq <= MXF_LIK_MAX_NODES, carried in the kernel arguments: nothing is allocated
 * or copied and the calls capture into a hipGraph).  y (S|1, n, 1) of the call's dtype, m (S|1, n, C) and v (S|1, n) are dense; strideS_*
 * is the sample stride in elements (n, n C, n), or 0 for an operand shared by the S samples.  A v below the floor 1e-12, a negative one
 * included, counts as the floor.  The label is read as an integer -- truncated toward zero and clamped to [0, C - 1] -- so no label value
 * can index outside the row: -1 reads as 0, C as C - 1, 2.5 as 2.  2 <= C <= MXF_ROBUSTMAX_MAX_C: any other C is status -3 and no
 * buffer is touched.  Every intermediate is finite in float32 for |m[y] - m[c]| <= 1e3 (mxfusion_amd/csrc/likelihood.h has the argument).
 *
 * mxf_robustmax_expect: out[s] += scale * sum_i E[log p(y_i | f_i)], out (S) ACCUMULATED INTO and required; in the same pass the reverse
 * mode, accumulated with w = scale, or scale * cot[s] given the per-sample weights cot (S, device, dtype of the call): the exact derivatives
 * of the quadrature sum (not Price's theorem: the integrand couples the C values of a row).  With P_k the product at node k and
 * lambda = phi / Phi:
 *   dm[s,i,c] += -w (L1 - L0) / sqrt(v_eff) sum_k w_k P_k lambda(z_kc)   (c != y),      dm[s,i,y] += minus the sum of those over c != y
 *   dv[s,i]   += -w (L1 - L0) / (2 v_eff^(3/2)) sum_k w_k P_k sum_{c != y} lambda(z_kc) (m[y] - m[c])      (nothing where v < 1e-12)
 * A node whose P_k underflows to 0 contributes exactly 0.  dm (S, n, C) and dv (S, n) always carry the sample axis: the caller of a
 * shared m or v sums them over s.  dm and dv may each be null.  eps is in (0, 1): anything else is status -2.
 * mxf_robustmax_probs: probs[s,i,c] = P(f_c is the largest), (S, n, C), WRITTEN.  Forward only.  The values are NOT renormalised: their sum
 * over c differs from 1 by the error of the rule (at nq = 20 with v = 25 in the data 7e-5 for C = 10 and 1.6e-3 for C = 32; 2e-9 for
 * C = 2 and v <= 4).                                                                                                                    */
#define MXF_ROBUSTMAX_MAX_C 32
int mxf_robustmax_expect(mxf_handle h, int dtype, int S, int64_t n, int C, const void* y, int64_t strideS_y, const void* m,
                         int64_t strideS_m, const void* v, int64_t strideS_v, int nq, const double* nodes, const double* weights,
                         double eps, const void* cot, double scale, void* out_acc, void* dm_acc, void* dv_acc, void* stream);
int mxf_robustmax_probs(mxf_handle h, int dtype, int S, int64_t n, int C, const void* m, int64_t strideS_m, const void* v,
                        int64_t strideS_v, int nq, const double* nodes, const double* weights, void* probs, void* stream);

/* RBF psi statistics: the expected kernel under a Gaussian input x_n ~ N(mu_n, diag(s_n)), the closed form that replaces Kuf and
 * Kuf Kuf^T in the collapsed sparse-GP bound when the inputs are uncertain (Titsias & Lawrence 2010, "Bayesian Gaussian Process Latent
 * Variable Model").  No reference counterpart: the reference averages its bound over draws of x.  With l2_q = lengthscale_q^2:
 *   Psi1[m,n]  = var   prod_q (1 + s_nq / l2_q)^-1/2   exp(-1/2 sum_q (mu_nq - z_mq)^2 / (s_nq + l2_q))                           (M, N)
 *   Psi2[m,m'] = var^2 sum_n prod_q (1 + 2 s_nq / l2_q)^-1/2 exp(-sum_q (z_mq - z_m'q)^2 / (4 l2_q)
 *                                                                 - sum_q (mu_nq - (z_mq + z_m'q) / 2)^2 / (2 s_nq + l2_q))        (M, M)
 * (psi0 = N var needs no kernel).  At s = 0, Psi1 = K(Z, X) and Psi2 = K(Z, X) K(Z, X)^T; s = 0 is a valid input, and a row far from
 * every z gives zeros, in the values and in the gradients.  mu, s (S|1, N, Q), Z (S|1, M, Q), lengthscale (S|1, Q with ard, else 1) and
 * variance (S|1, 1) are dense; strideS_* is the sample stride in elements, or 0 for an operand shared by the S samples.
 * 1 <= Q <= MXF_PSI_MAX_Q: a larger Q is status -3, and no buffer is touched.  The N M^2 / 2 terms of Psi2 are never stored; the sum over n is
 * formed in double for either dtype (mxfusion_amd/csrc/psi.hip has the decomposition).  Scratch comes from the handle.
 *
 * mxf_psi_rbf_fwd: Psi1 (S, M, N) and Psi2 (S, M, M) are WRITTEN; either may be null.  Psi2 is formed on m' <= m and mirrored: bitwise
 * symmetric.
 * mxf_psi_rbf_bwd: the cotangents G1 (S, M, N) and G2 (S, M, M), either may be null; G2 need not be symmetric (G2 + G2^T is what counts).
 * The gradients are ACCUMULATED into dense buffers shaped like their operands with a shared sample axis at extent 1 (then summed over the
 * samples): dmu, ds (S|1, N, Q), dZ (S|1, M, Q), dls (S|1, Q or 1), dvar (S|1, 1); any may be null.
 * mxf_psi_rbf_quad: the per-row contraction R[s,n,j] = sum_{m,m'} A[s,j,m,m'] psi2n[s,n,m,m'] of the terms Psi2 sums over n, for J >= 1
 * weight matrices A (S|1, J, M, M) that need not be symmetric (A_j + A_j^T is what counts; strideS_A is 0 or J M M).  R (S, N, J) is
 * WRITTEN.  A thread owns a row; the sum over (m, m') is formed in double for either dtype.  J < 1 or a null A or R is status -2.  It is
 * the second moment of a sparse-GP prediction at a Gaussian test input (BayesianGPLVMUncertainInputPrediction).  No reverse mode.      */
#define MXF_PSI_MAX_Q 16
int mxf_psi_rbf_fwd(mxf_handle h, int dtype, int S, int64_t N, int64_t M, int Q, const void* mu, int64_t strideS_mu,
                    const void* s, int64_t strideS_s, const void* Z, int64_t strideS_Z, const void* lengthscale, int ard, int64_t strideS_ls,
                    const void* variance, int64_t strideS_var, void* Psi1, void* Psi2, void* stream);
int mxf_psi_rbf_bwd(mxf_handle h, int dtype, int S, int64_t N, int64_t M, int Q, const void* mu, int64_t strideS_mu,
                    const void* s, int64_t strideS_s, const void* Z, int64_t strideS_Z, const void* lengthscale, int ard, int64_t strideS_ls,
                    const void* variance, int64_t strideS_var, const void* G1, const void* G2, void* dmu_acc, void* ds_acc, void* dZ_acc,
                    void* dls_acc, void* dvar_acc, void* stream);
int mxf_psi_rbf_quad(mxf_handle h, int dtype, int S, int64_t N, int64_t M, int Q, const void* mu, int64_t strideS_mu,
                     const void* s, int64_t strideS_s, const void* Z, int64_t strideS_Z, const void* lengthscale, int ard, int64_t strideS_ls,
                     const void* variance, int64_t strideS_var, int J, const void* A, int64_t strideS_A, void* R, void* stream);

/* Random Fourier feature expansion of stationary GP prior draws, the prior part of a pathwise posterior sample (Wilson et al. 2020,
 * "Efficiently sampling functions from Gaussian process posteriors").  No reference counterpart.
 *   out[s,n,j] = sum_d cos(X[s,n,:] . Omega[s,d,:] + phase[s,d]) W[s,d,j]
 * X (S|1, N, Q), the frequencies Omega (S|1, D, Q) with the lengthscales already divided in, phase (S|1, D) and the weights W (S|1, D, J) with
 * the amplitude already multiplied in are dense; strideS_* is the sample stride in elements, or 0 for an operand shared by the S samples.
 * 1 <= Q <= MXF_RFF_MAX_Q: a larger Q is status -3, and no buffer is touched; a null pointer or a bad shape or stride is status -2.  The
 * N x D cosines are never stored: a thread owns a row and evaluates each cosine once for all J columns; the sum over d is formed in double
 * for either dtype (mxfusion_amd/csrc/rff.hip has the decomposition).  float32 uses the hardware cosine and sine on an argument reduced to
 * one revolution.  Scratch comes from the handle.
 *
 * mxf_rff_eval: out (S, N, J) is WRITTEN.
 * mxf_rff_eval_bwd: the cotangent G (S, N, J) of out; the gradient in the inputs,
 *   dX[s,n,q] += -sum_d sin(X[s,n,:] . Omega[s,d,:] + phase[s,d]) Omega[s,d,q] sum_j G[s,n,j] W[s,d,j],
 * is ACCUMULATED into dX_acc, dense and shaped like X, a shared sample axis at extent 1 and summed over.  There is no reverse mode for
 * Omega, phase or W.                                                                                                                    */
#define MXF_RFF_MAX_Q 16
int mxf_rff_eval(mxf_handle h, int dtype, int S, int64_t N, int64_t D, int Q, int J, const void* X, int64_t strideS_X,
                 const void* Omega, int64_t strideS_Om, const void* phase, int64_t strideS_ph, const void* W, int64_t strideS_W, void* out,
                 void* stream);
int mxf_rff_eval_bwd(mxf_handle h, int dtype, int S, int64_t N, int64_t D, int Q, int J, const void* X, int64_t strideS_X,
                     const void* Omega, int64_t strideS_Om, const void* phase, int64_t strideS_ph, const void* W, int64_t strideS_W,
                     const void* G, void* dX_acc, void* stream);

/* Matrix-free product of a stationary covariance matrix with a block of J vectors, the primitive of conjugate-gradient exact GP regression
 * (Wang et al. 2019, "Exact Gaussian processes on a million data points").  No reference counterpart.
 *   out[s,n,j] = sum_n2 k(X[s,n,:], X2[s,n2,:]) V[s,n2,j]   (+ diag_add[s] V[s,n,j] when X2 is NULL: the square product with X2 = X, N2 = N)
 * kind is MXF_K_RBF or MXF_K_MATERN12 / 32 / 52, and the covariance of a pair is the function of the operands that mxf_gram evaluates (the
 * difference form on operands centred on the first row of X2, the same clipping of r in the Matern kinds).  X (S|1, N, Q), X2 (S|1, N2, Q),
 * lengthscale (S|1, Q with ard else 1), variance and diag_add (S|1, 1; diag_add may be NULL, and is ignored with an X2) and V (S|1, N2, J) are
 * dense; strideS_* is the sample stride in elements, or 0 for an operand shared by the S samples.  1 <= Q <= MXF_KMV_MAX_Q: a larger Q is
 * status -3, and no buffer is touched; S <= 65535, N, N2 <= 2^31, J <= 2^16; a null pointer, a bad shape or a bad stride is status -2.
 * Nothing of size N x N2 is stored: a thread owns a row and evaluates each covariance once for J (up to 16 at a time) columns; the sum over
 * n2 is formed in double for either dtype (mxfusion_amd/csrc/kmv.hip has the decomposition).  Scratch, (N2 (Q + J) elements and, for few
 * rows and many columns, S N J doubles), comes from the handle.
 *
 * mxf_kmv: out (S, N, J) is WRITTEN.
 * mxf_kmv_bwd: the gradient of the weighted bilinear form  sum_s sum_j w[j] A[s,:,j]^T K(X[s], X2[s]) V[s,:,j]  in lengthscale and variance,
 *   ACCUMULATED into dls_acc and dvar_acc, shaped like lengthscale and variance, a shared sample axis at extent 1 and summed over; either may
 *   be NULL.  A (S|1, N, J); w: J doubles on the HOST, read before the call returns.  The cotangent of a pair, sum_j w[j] A[n,j] V[n2,j], is
 *   formed in registers.  There is no reverse mode in X or X2, and none is needed for V: the gradient of the product in V is mxf_kmv with X
 *   and X2 exchanged.                                                                                                                       */
#define MXF_KMV_MAX_Q 16
int mxf_kmv(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int J, const void* X, int64_t strideS_X, const void* X2,
            int64_t strideS_X2, const void* lengthscale, int64_t strideS_ls, int ard, const void* variance, int64_t strideS_var,
            const void* diag_add, int64_t strideS_da, const void* V, int64_t strideS_V, void* out, void* stream);
int mxf_kmv_bwd(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q, int J, const void* X, int64_t strideS_X, const void* X2,
                int64_t strideS_X2, const void* lengthscale, int64_t strideS_ls, int ard, const void* variance, int64_t strideS_var,
                const void* A, int64_t strideS_A, const void* V, int64_t strideS_V, const double* w, void* dls_acc, void* dvar_acc,
                void* stream);

/* Nearest-centre assignment and one Lloyd iteration of k-means, the primitive of initialising inducing inputs from data
 * (mxfusion_amd/util/inducing.py).  No reference counterpart: the reference draws its inducing inputs from a standard normal.
 *   idx[n] = argmin_m sum_q (X[n,q] - C[m,q])^2,   d2[n] = that minimum
 * There is no sample axis.  X (N, Q) and the centres C (M, Q) are dense row-major in dtype (float32 or float64).  The distance is the
 * difference form, summed in the working dtype -- not |x|^2 - 2 x.c + |c|^2, which cancels for nearby points.  m is scanned in ascending
 * order with a strict <: among exact ties the SMALLEST index wins (a contract).  Inputs are finite: the caller's precondition, not checked.
 * 1 <= Q <= MXF_NEAREST_MAX_Q: a larger Q is status -3, and no buffer is touched; a null required pointer, N, M or Q < 1, N > 2^31,
 * M > 2^31 - 1 or C_new == C is status -2.  Nothing of size N x M is stored: a thread owns a row and scans the centres, which arrive as
 * scalar loads (mxfusion_amd/csrc/nearest.hip has the decomposition).  Scratch, M Q elements and for a step M (Q + 1) doubles (Q padded to
 * 4, 8 or 16), comes from the handle.
 *
 * mxf_nearest: idx (N) int32 is WRITTEN, and d2 (N) in dtype where it is not NULL.
 * mxf_kmeans_step: one Lloyd iteration in one call.  C_new (M, Q) is WRITTEN: row m is the mean of the rows of X assigned to m (summed in
 *   double, rounded once), or C[m] bitwise where no row is, with counts[m] = 0.  counts (M) int64 and inertia[0] = sum_n d2[n] (a double
 *   on the device) are WRITTEN; idx (N) is written where it is not NULL.  C_new must not alias C.  The sums are atomic: C_new and inertia
 *   can differ in their last bits from call to call, idx and counts cannot.                                                                */
#define MXF_NEAREST_MAX_Q 16
int mxf_nearest(mxf_handle h, int dtype, int64_t N, int64_t M, int Q, const void* X, const void* C, int32_t* idx, void* d2, void* stream);
int mxf_kmeans_step(mxf_handle h, int dtype, int64_t N, int64_t M, int Q, const void* X, const void* C, void* C_new, int32_t* idx,
                    int64_t* counts, double* inertia, void* stream);

/* The k nearest rows of C (Nc, Q) for every row of X (N, Q), the neighbour search of nearest-neighbour (Vecchia) GP regression.  No reference
 * counterpart.  With causal != 0 the candidates of row n are the rows j < n of X itself: the caller passes C == X and Nc == N, anything else
 * is status -2.  Otherwise they are all rows j < Nc.  There is no sample axis; X and C are dense row-major in dtype.  The distance is
 * mxf_nearest's difference form, summed in the working dtype.  idx (N, k) int32 and, where it is not NULL, d2 (N, k) in dtype are WRITTEN:
 * a row's slots are sorted ascending by (d2, j), lexicographic and strict, so the result is deterministic and among exact ties the smaller
 * index comes first; slots beyond the number of candidates hold idx = -1 and d2 = +inf.  Inputs are finite: the caller's precondition.
 * 1 <= Q <= MXF_KNN_MAX_Q and 1 <= k <= MXF_KNN_MAX_K: above either is status -3, and no buffer is touched; a null required pointer, N, Nc, Q
 * or k < 1, N > 2^31 or Nc > 2^31 - 1 is status -2.  Nothing of size N x Nc is stored: a thread owns a row, keeps its running list in
 * registers and scans the candidates, which arrive as scalar loads (mxfusion_amd/csrc/knn.hip).  Scratch, Nc Q elements (Q padded to 4, 8
 * or 16), comes from the handle.  A lengthscale is the caller's job: pass X / lengthscale.                                                */
#define MXF_KNN_MAX_Q 16
#define MXF_KNN_MAX_K 32
int mxf_knn(mxf_handle h, int dtype, int64_t N, int64_t Nc, int Q, int k, int causal, const void* X, const void* C, int32_t* idx, void* d2,
            void* stream);

/* Nearest-neighbour (Vecchia) Gaussian process regression (Vecchia 1988; Datta et al. 2016): every row is conditioned on at most k <= 32
 * other rows, so the log-likelihood is a sum of N independent problems of order k.  No reference counterpart.  With c the neighbours of a
 * row (nbr (rows, k) int32: entries are -1, an empty slot anywhere in the row, or a row of X), A = K(X_c, X_c) + noise I,
 * kappa = K(X_c, x), a = k(x, x) + noise:
 *   b = A^-1 kappa,  alpha = A^-1 Y_c,  s = a - kappa^T b,  r = y - kappa^T alpha,  l = -P/2 log 2 pi - P/2 log s - |r|^2 / (2 s)
 * kind is MXF_K_RBF or MXF_K_MATERN12 / 32 / 52 and the covariance of a pair is the function of its scaled distance that mxf_gram evaluates,
 * the clip of r in the Matern kinds included (so k(x, x) of the log-pdf is the diagonal mxf_gram writes; the predictor's k(x*, x*) is the
 * variance, as mxf_kdiag).  X (N, Q), Y (N, P), lengthscale (Q with ard else 1), variance (1) and noise (1) are dense in dtype on the
 * device; there is no sample axis.  Q <= MXF_KNN_MAX_Q, k <= MXF_KNN_MAX_K, P <= MXF_VECCHIA_MAX_P: above is status -3, and no buffer is
 * touched; a null required pointer or an extent < 1 is status -2.  The caller's preconditions, not checked: the entries of nbr are -1 or in
 * [0, N) and, for the log-pdf of row i, < i (an entry outside [0, N) is read as -1).  The k x k matrices live in LDS in double for either
 * dtype; nothing of size N x k^2 is stored or saved between the passes.  A pivot that is not positive makes that row's term, and with it the
 * value and the gradients, NaN; nothing traps.  The value and the parameter gradients are summed per workgroup in double and meet in double
 * scratch with atomics, and dY is scattered with atomics: their last bits can differ from call to call.
 *
 * mxf_vecchia_cond: the predictor.  For every row of Xt (Nt, Q) with its neighbours nbr (Nt, k) among the rows of X, mean_out (Nt, P) =
 *   kappa^T alpha and var_out (Nt) = k(x*, x*) - kappa^T b, the latent values, are WRITTEN.
 * mxf_vecchia_logpdf: terms_out (N) in dtype, the l_i, where it is not NULL, and value_out[0], their sum (a double on the device), are WRITTEN.
 * mxf_vecchia_logpdf_bwd: the gradient of g[0] * sum_i l_i (g: one element of dtype on the device) in lengthscale (dls: Q with ard else
 *   1), variance (dvar), noise (dnoise) and Y (dY (N, P)), WRITTEN, not accumulated; each may be NULL.  The factor is recomputed.  There is no
 *   reverse mode in X.                                                                                                                    */
#define MXF_VECCHIA_MAX_P 32
int mxf_vecchia_cond(mxf_handle h, int kind, int dtype, int64_t Nt, int64_t N, int Q, int P, int k, int ard, const void* Xt, const void* X,
                     const void* Y, const int32_t* nbr, const void* lengthscale, const void* variance, const void* noise, void* mean_out,
                     void* var_out, void* stream);
int mxf_vecchia_logpdf(mxf_handle h, int kind, int dtype, int64_t N, int Q, int P, int k, int ard, const void* X, const void* Y,
                       const int32_t* nbr, const void* lengthscale, const void* variance, const void* noise, void* terms_out, double* value_out,
                       void* stream);
int mxf_vecchia_logpdf_bwd(mxf_handle h, int kind, int dtype, int64_t N, int Q, int P, int k, int ard, const void* X, const void* Y,
                           const int32_t* nbr, const void* lengthscale, const void* variance, const void* noise, const void* g, void* dls,
                           void* dvar, void* dnoise, void* dY, void* stream);

/* Multivariate normal of order n <= 32 over x (S, B, n), mean (S|1, B|1, n) and A (S|1, B|1, n, n): A is the covariance (form 0) or the
 * precision (form 1).  A larger n is status -3 from every entry point, and no buffer is touched (such matrices take mxf_potrf /
 * mxf_trsm).  Replaces MultivariateNormal.log_pdf_impl (components/distributions/normal.py:157-178: linalg.potrf, linalg.trsm,
 * linalg.sumlogdiag) and MultivariateNormalMeanPrecision.log_pdf_impl (normal.py:369-394: the per-row F.dot loop and log_determinant),
 * and MXNet autograd through them.  Launch-bound at the sizes of a prior: one launch each, two for the reverse mode with dA.
 *
 * mxf_mvn_factor: the S_A * B_A distinct matrices of A (row stride lda, sample and batch strides in elements; an axis that A is shared
 * over has extent 1) -> F (S_A, B_A, n, n) dense, lower with a zero upper triangle: L^-1 of A = L L^T (form 0) or L itself (form 1), and
 * logdet (S_A, B_A) = sum_i log L_ii.  info: device int[S_A * B_A], zeroed by the caller; a matrix whose j-th pivot is not positive gets
 * info = j (1-based, its first such pivot, as mxf_potrf), NaN in logdet and NaN from that column on in F.  The call still returns 0.
 * float32 forms the pivot sums and the log-determinant in double.                                                                      */
int mxf_mvn_factor(mxf_handle h, int dtype, int form, int S_A, int64_t B_A, int n, const void* A, int64_t lda, int64_t strideS_A,
                   int64_t strideB_A, void* F, void* logdet, int* info, void* stream);

/* out[s,b] = scale * log N(x[s,b] | mean, A), WRITTEN, from the factor stage's F and logdet; S_A in {1, S}, B_A in {1, B} say which axes
 * the matrices have.  x: rows of n contiguous elements, batch stride n, sample stride strideS_x (0: shared by the samples); mean: sample
 * and batch stride, either may be 0.  form 0: z = L^-1 (x - mean), -1/2 |z|^2 - logdet - n/2 log 2 pi (normal.py:173-178);
 * form 1: z = L^T (x - mean), + logdet (normal.py:384-394).                                                                            */
int mxf_mvn_logpdf(mxf_handle h, int dtype, int form, int S, int64_t B, int n, const void* x, int64_t strideS_x, const void* mean,
                   int64_t strideS_mean, int64_t strideB_mean, const void* F, const void* logdet, int S_A, int64_t B_A, double scale,
                   void* out, void* stream);

/* Reverse mode of mxf_mvn_logpdf with the cotangent cot (S, B): w = scale * cot[s,b], alpha = A^-1 (x - mean) (form 1: A (x - mean)),
 *   dx -= w alpha,  dmean += w alpha,  dA += 1/2 w (alpha alpha^T - A^-1)   (form 1: dA += 1/2 w (A^-1 - d d^T), d = x - mean)
 * ACCUMULATED into dense buffers shaped like their operands -- dx (S|1, B, n), dmean (S|1, B|1, n), dA (S_A, B_A, n, n), symmetric -- and
 * summed over the axes an operand is shared over.  The term in A^-1 is added once per distinct matrix with the summed weight.  Any
 * output may be null.                                                                                                                   */
int mxf_mvn_logpdf_bwd(mxf_handle h, int dtype, int form, int S, int64_t B, int n, const void* x, int64_t strideS_x, const void* mean,
                       int64_t strideS_mean, int64_t strideB_mean, const void* F, int S_A, int64_t B_A, const void* cot, double scale,
                       void* dx_acc, void* dmean_acc, void* dA_acc, void* stream);

/* Wishart density of order n <= 32 over X (S|1, B, n, n) with the scale matrices V (S|1, B|1, n, n) and the degrees of freedom
 * dof (S|1, B|1), all symmetric positive definite resp. > n - 1:
 *   out[s,b] = scale * (1/2 [(dof - n - 1) log|X| - tr(V^-1 X) - dof n log 2 - dof log|V|] - log Gamma_n(dof / 2)),  WRITTEN,
 *   log Gamma_n(a) = n (n - 1) / 4 log pi + sum_{k=1..n} lgamma(a + (1 - k) / 2).
 * Replaces Wishart.log_pdf_impl (components/distributions/wishart.py:62-96) and the per-element loops it calls (util/special.py:21-132:
 * log_determinant, solve, trace, log_multivariate_gamma), and MXNet autograd through them.  Launch-bound at the sizes of a prior: one
 * launch each (float32 reverse mode with shared operands: a fill and a fold more).  A larger n is status -3 and no buffer is touched.
 * Strides are in elements.  X: rows of n contiguous elements at row stride ldx, the B matrices of a sample n * ldx apart, sample stride
 * strideS_X (0: shared by the samples).  V: row stride ldv, sample and batch strides; S_V in {1, S} and B_V in {1, B} say which axes it
 * has.  dof: sample and batch stride, either may be 0.  Only the lower triangles of X and V are read.  float32 operands are factorised in
 * double.  info: device int[S * B], zeroed by the caller; a row gets j (1-based) when the j-th pivot of its V is not positive, else n + j
 * for the j-th pivot of its X, else 2 n + 1 when dof <= n - 1, and its value is NaN.  The call still returns 0.                         */
int mxf_wishart_logpdf(mxf_handle h, int dtype, int S, int64_t B, int n, const void* X, int64_t ldx, int64_t strideS_X, const void* dof,
                       int64_t strideS_dof, int64_t strideB_dof, const void* V, int64_t ldv, int64_t strideS_V, int64_t strideB_V, int S_V,
                       int64_t B_V, double scale, void* out, int* info, void* stream);

/* Reverse mode of mxf_wishart_logpdf with the cotangent cot (S, B), w = scale * cot[s,b] (wishart.py:62-96 under autograd):
 *   dX += w [1/2 (dof - n - 1) X^-1 - 1/2 V^-1],   dV += w [1/2 V^-1 X V^-1 - 1/2 dof V^-1],
 *   ddof += w [1/2 (log|X| - n log 2 - log|V|) - 1/2 sum_{k=1..n} psi((dof + 1 - k) / 2)]
 * ACCUMULATED into dense buffers shaped like their operands with the shared axes at extent 1 -- dX (S|1, B, n, n) and dV (S_V, B_V, n, n),
 * full symmetric matrices, ddof (S|1, B|1) -- and summed, in double for either dtype, over the axes an operand is shared over.  A row that
 * fails as above contributes NaN.  Any output may be null.                                                                             */
int mxf_wishart_logpdf_bwd(mxf_handle h, int dtype, int S, int64_t B, int n, const void* X, int64_t ldx, int64_t strideS_X, const void* dof,
                           int64_t strideS_dof, int64_t strideB_dof, const void* V, int64_t ldv, int64_t strideS_V, int64_t strideB_V, int S_V,
                           int64_t B_V, const void* cot, double scale, void* dX_acc, void* ddof_acc, void* dV_acc, void* stream);

/* Categorical and Dirichlet: log-densities that reduce along a class axis.  Rows are (s, b), s < S samples and b < B batch entries, of
 * K >= 1 contiguous elements; strides are in elements and dense where not 0: a sample or batch stride of 0 shares the operand over that
 * axis.  One group of 4 (K <= 4), 16 (K <= 16) or 64 lanes per row, reductions over K on wave shuffles.  Launch-bound at the size of a
 * prior, bandwidth-bound at the size of a classification likelihood: one launch each (float32 reverse mode with a parameter shared over
 * the batch axis: a fill and a fold more).
 *
 * mxf_categorical_logpdf: out[s,b] = scale * lp[x[s,b]] (one_hot = 0) or scale * sum_k x[s,b,k] lp_k (one_hot = 1), WRITTEN, with
 * lp = logp - logsumexp(logp) along K (normalize = 1; the row maximum is subtracted first, a row of all -inf is NaN) or lp = logp.
 * logp (S|1, B|1, K).  one_hot = 0: x (S|1, B), class indices held in the floating type, truncated toward zero and clipped to
 * [0, K - 1] (the default mode of MXNet's pick).  one_hot = 1: x (S|1, B, K).  Replaces Categorical.log_pdf_impl
 * (components/distributions/categorical.py:83-106: log_softmax, pick / broadcast_mul and sum).                                        */
int mxf_categorical_logpdf(mxf_handle h, int dtype, int S, int64_t B, int K, const void* logp, int64_t strideS_lp, int64_t strideB_lp,
                           const void* x, int64_t strideS_x, int one_hot, int normalize, double scale, void* out, void* stream);

/* Reverse mode of mxf_categorical_logpdf with the cotangent cot (S, B), w = scale * cot[s,b] (categorical.py:83-106 under autograd):
 *   dlogp_k += w (t_k - p_k sum_j t_j), p = exp(lp)  (normalize = 1)   or   w t_k  (normalize = 0),     dx_k += w lp_k  (one_hot = 1)
 * with t the one-hot row of the clipped index, or x itself when one_hot = 1.  ACCUMULATED into dense buffers shaped like their operands
 * with the shared axes at extent 1 -- dlogp (S|1, B|1, K), dx (S|1, B, K) -- and summed over the axes an operand is shared over (over
 * the batch axis in double for either dtype).  dx_acc must be null when one_hot = 0 (an index has no gradient): status -2.  Any output
 * may be null.                                                                                                                         */
int mxf_categorical_logpdf_bwd(mxf_handle h, int dtype, int S, int64_t B, int K, const void* logp, int64_t strideS_lp, int64_t strideB_lp,
                               const void* x, int64_t strideS_x, int one_hot, int normalize, const void* cot, double scale,
                               void* dlogp_acc, void* dx_acc, void* stream);

/* mxf_dirichlet_logpdf: x (S|1, B, K), alpha (S|1, B|1, K),
 *   out[s,b] = scale * (sum_k (alpha_k - 1) log xt_k + lgamma(sum_k alpha_k) - sum_k lgamma(alpha_k)),  WRITTEN,
 * xt = x / sum_k |x_k| (normalize = 1) or x.  The three lgamma sums are formed in double for either dtype.  A row with an x_k <= 0 or
 * an alpha_k <= 0 is NaN, the others are unaffected, and the call still returns 0.  Replaces Dirichlet.log_pdf_impl
 * (components/distributions/dirichlet.py:43-65: norm, broadcast_power, prod and the log of a quotient of gamma products, which
 * overflows from alpha ~ 170; the value is the same).                                                                                 */
int mxf_dirichlet_logpdf(mxf_handle h, int dtype, int S, int64_t B, int K, const void* x, int64_t strideS_x, const void* alpha,
                         int64_t strideS_a, int64_t strideB_a, int normalize, double scale, void* out, void* stream);

/* Reverse mode of mxf_dirichlet_logpdf with the cotangent cot (S, B), w = scale * cot[s,b] (dirichlet.py:43-65 under autograd):
 *   dalpha_k += w (log xt_k + psi(sum_j alpha_j) - psi(alpha_k)),
 *   dx_j += w ((alpha_j - 1) / x_j - [normalize] sum_k (alpha_k - 1) / sum_k |x_k|)
 * ACCUMULATED and summed over shared axes as in mxf_categorical_logpdf_bwd: dx (S|1, B, K), dalpha (S|1, B|1, K).  A row that fails as
 * above contributes NaN.  Any output may be null.                                                                                     */
int mxf_dirichlet_logpdf_bwd(mxf_handle h, int dtype, int S, int64_t B, int K, const void* x, int64_t strideS_x, const void* alpha,
                             int64_t strideS_a, int64_t strideB_a, int normalize, const void* cot, double scale, void* dx_acc,
                             void* dalpha_acc, void* stream);

/* A dense neural-network layer with the sample axis (dense.hip): X (S|1, N, I) with rows ldx >= I elements apart, W (S|1, O, I)
 * row-major and dense (the layout of torch.nn.Linear.weight), b (S|1, O) or null; a sample stride of 0 shares the operand over the
 * samples.  act: 0 identity, 1 tanh, 2 relu, 3 sigmoid.  Widths 1 <= I, O <= 128; anything else is status -3 (the caller's to route to
 * mxf_gemm).  One launch for all S samples; every element of W[s] and b[s] is fetched once per workgroup of 32 (float) or 16 (double)
 * rows.
 *
 * mxf_dense_fwd: Y[s,n,:] = act(X[s,n,:] W[s]^T + b[s]), WRITTEN to the dense Y (S, N, O).  Replaces the per-sample loop of
 * FunctionEvaluation.eval over a Gluon Dense block (components/functions/function_evaluation.py:77-96).                                */
int mxf_dense_fwd(mxf_handle h, int dtype, int S, int64_t N, int I, int O, int act, const void* X, int64_t ldx, int64_t strideS_x,
                  const void* W, int64_t strideS_w, const void* b, int64_t strideS_b, void* Y, void* stream);

/* Reverse mode of mxf_dense_fwd from its result Y (every supported act' is a function of Y) and the cotangent dY (S, N, O), both dense:
 *   G = dY act'(Y),   dX[s] += G W[s],   dW[s] += G^T X[s],   db[s] += sum_n G
 * ACCUMULATED into dense buffers shaped like their operands with a shared sample axis at extent 1 -- dX (S|1, N, I), dW (S|1, O, I),
 * db (S|1, O); strideS_b says whether db is shared (0) or own (O).  The sums over the rows, and over s where the operand is shared, are
 * formed in double for either dtype (float32: zeroed handle scratch and a fold more for dW and db).  Any output may be null.           */
int mxf_dense_bwd(mxf_handle h, int dtype, int S, int64_t N, int I, int O, int act, const void* X, int64_t ldx, int64_t strideS_x,
                  const void* W, int64_t strideS_w, int64_t strideS_b, const void* Y, const void* dY, void* dX_acc, void* dW_acc,
                  void* db_acc, void* stream);

/* The model operators' arithmetic (ewise.hip): one broadcast map over up to MXF_EW_MAX_RANK axes -- the sample axis included, counted
 * after the caller has merged what can be merged -- for all samples in one launch.
 *   op: 0 add, 1 subtract, 2 multiply, 3 divide, 4 power, 5 square, 6 exp, 7 log   (5..7: y and stride_y are ignored and may be null)
 * extent[0] is the sample axis S; stride_x / stride_y are in elements, and a stride of 0 (or an extent of 1) shares the operand over that
 * axis.  extent and the strides are HOST arrays of `rank` entries, read during the call and passed to the kernel by value.  Strides are
 * not negative; anything else goes (a transposed view, an odd start: the kernel uses 16-byte accesses where a chunk is aligned and
 * contiguous and scalar ones elsewhere).  exp, log and pow are the device library's accurate functions.
 * Status -2: bad arguments (dtype, op, rank < 1, a null operand or array, a negative extent or stride).  Status -3: rank above
 * MXF_EW_MAX_RANK, or more than 2^31 * 16 output elements, or an operand spanning more than that; no buffer is touched (the caller's to
 * route elsewhere).
 *
 * mxf_ewise_fwd: z = op(x, y), WRITTEN, z dense row-major over extent.  Replaces add .. log of
 * components/functions/operators/operator_impl.py:27-85 run once per sample by the loop of FunctionEvaluation.eval
 * (components/functions/function_evaluation.py:72-96).                                                                                 */
#define MXF_EW_MAX_RANK 5
int mxf_ewise_fwd(mxf_handle h, int op, int dtype, int rank, const int64_t* extent, const void* x, const int64_t* stride_x,
                  const void* y, const int64_t* stride_y, void* z, void* stream);

/* Reverse mode of mxf_ewise_fwd with the cotangent dz, dense over extent (operator_impl.py:27-85 under MXNet autograd, one sample at a
 * time: function_evaluation.py:72-96):
 *   add dz, dz | subtract dz, -dz | multiply dz y, dz x | divide dz / y, -dz x / y^2 | power dz y x^(y-1), dz x^y log x |
 *   square 2 x dz | exp dz exp x | log dz / x
 * ACCUMULATED into dx_acc and dy_acc: dense, shaped like their operand with every shared axis at extent 1.  An operand without a shared
 * axis gets plain stores; a shared operand's gradient is the sum over its shared axes, formed in double for either dtype (float32: zeroed
 * handle scratch and a fold more) after a workgroup has reduced what it holds for one element.  For power a wanted dy at x <= 0 is NaN or
 * infinite, as log x is.  Either output may be null.                                                                                   */
int mxf_ewise_bwd(mxf_handle h, int op, int dtype, int rank, const int64_t* extent, const void* x, const int64_t* stride_x,
                  const void* y, const int64_t* stride_y, const void* dz, void* dx_acc, void* dy_acc, void* stream);

/* The reductions behind the sample axis (ewise.hip).  kind: 0 sum, 1 mean, 2 prod.  x dense (outer, R, inner) -> y dense (outer, inner),
 * WRITTEN; R >= 1.  inner == 1: a wave per row up to R = 512, a workgroup per row beyond; inner > 1: lanes along inner, a loop over R.
 * Every kind accumulates in double for either dtype.  Status -3 beyond 2^31 * 16 elements.  Replaces sum, mean and prod of
 * operator_impl.py:27-85 under the per-sample loop of function_evaluation.py:72-96.                                                     */
int mxf_reduce_fwd(mxf_handle h, int kind, int dtype, int64_t outer, int64_t R, int64_t inner, const void* x, void* y, void* stream);

/* Reverse mode of mxf_reduce_fwd with the cotangent dy (outer, inner), ACCUMULATED into dx_acc (outer, R, inner) (operator_impl.py:27-85
 * under autograd, function_evaluation.py:72-96): sum dy; mean dy / R; prod dy times the product of the other entries, formed from
 * exclusive prefix and suffix products (double, handle scratch; the forward's regimes) and never by dividing -- a row with one zero or
 * several is right.
 * x is read by prod only.  A null dx_acc: nothing to do.                                                                               */
int mxf_reduce_bwd(mxf_handle h, int kind, int dtype, int64_t outer, int64_t R, int64_t inner, const void* x, const void* dy,
                   void* dx_acc, void* stream);

/* MXNet Adam as driven by gluon.Trainer.step (batch_loop.py:46-60, minibatch_loop.py:71-91):
 * g*=rescale; m=b1 m+(1-b1)g; v=b2 v+(1-b2)g^2; w -= lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps)      */
int mxf_adam_step(mxf_handle h, int dtype, int64_t n, void* w, const void* g, void* m, void* v,
                  double lr, double beta1, double beta2, double epsilon, double rescale_grad, int t,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused composites: one call = one reference `compute` body, value AND reverse mode.               */

/* GPRegressionLogPdf.compute (modules/gp_modules/gp_regression.py:42-76), stationary kernel.
 *   X (S|1,N,Q)  Y (S|1,N,P) [already minus mean]  noise_var (S|1,1)
 * outputs: logL (S);  L (S,N,N) and LinvY (S,N,P) (the posterior side effect of :72-75);
 * if want_grad: dX (S,N,Q), dY (S,N,P), dnoise (S), dls (S,Q|1), dvar (S) = d logL[s] / d(.) , WRITTEN.
 * info: device int[S].                                                                             */
int mxf_gp_logpdf(mxf_handle h, int kind, int dtype, int S, int64_t N, int Q, int P,
                  const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y,
                  const void* noise_var, int64_t strideS_noise,
                  const void* lengthscale, int ard, int64_t strideS_ls,
                  const void* variance, int64_t strideS_var, double jitter,
                  void* logL, void* L, void* LinvY, int* info, int want_grad,
                  void* dX, void* dY, void* dnoise, void* dls, void* dvar, void* stream);

/* SVGPRegressionLogPdf.compute (modules/gp_modules/svgp_regression.py:43-109), homoscedastic noise,
 * stationary kernel, streaming sufficient-statistics form: Kuf is never the operand of a
 * triangular solve; all (M x M) factorisation work is done once (not S times) in float64.
 *   X (S|1,B,Q)  Y (S|1,B,P) [minus mean]  Z (M,Q)  noise_var (1)  qU_mean (M,P)  qU_cov_W (M,M)
 *   qU_cov_diag (M) [positive]  lengthscale (Q|1)  variance (1); scaling = log_pdf_scaling (:108)
 * outputs: logL (S) per-sample bound.  If want_grad: gradients of  sum_s gw[s]*logL[s]  (gw: host
 * weights folded as a single scalar `gscale` applied to every sample, i.e. the mean_S of
 * factor_graph.py:233 => gscale = 1/S): dX (S,B,Q) dY (S,B,P) dZ (M,Q) dnoise (1) dmu (M,P) dW (M,M)
 * dSdiag (M) dls (Q|1) dvar (1), all WRITTEN.                                                      */
int mxf_svgp_logpdf(mxf_handle h, int kind, int dtype, int S, int64_t B, int64_t M, int Q, int P,
                    const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y,
                    const void* Z, const void* noise_var, const void* qU_mean, const void* qU_cov_W,
                    const void* qU_cov_diag, const void* lengthscale, int ard, const void* variance,
                    double jitter, double scaling, double gscale,
                    void* logL, int* info, int want_grad,
                    void* dX, void* dY, void* dZ, void* dnoise, void* dmu, void* dW, void* dSdiag,
                    void* dls, void* dvar, void* stream);

/* The same bound with SAMPLED parameters: every operand of svgp_regression.py:43-109 may carry the sample axis (the reference broadcasts
 * all of them to S, components/variables/runtime_variable.py:96-118, exercised by its tests with sampled variables): sample s uses slice
 * s of every operand with a non-zero sample stride (in elements; 0 = shared), incl. its own Kuu / q(u) core.
 *   X (S|1,B,Q)  Y (S|1,B,P)  Z (S|1,M,Q)  noise_var (S|1,1)  qU_mean (S|1,M,P)  qU_cov_W (S|1,M,M)  qU_cov_diag (S|1,M)
 *   lengthscale (S|1,Q|1)  variance (S|1,1)
 * outputs: logL (S), info (S ints).  If want_grad: dX (S,B,Q) dY (S,B,P) dZ (S,M,Q) dnoise (S) dmu (S,M,P) dW (S,M,M) dSdiag (S,M)
 * dls (S,Q|1) dvar (S), all WRITTEN: slice s = gradient of gscale * logL[s] w.r.t. the operands sample s used (a shared operand's
 * gradient is the sum of its slices).                                                                                            */
int mxf_svgp_logpdf_sampled(mxf_handle h, int kind, int dtype, int S, int64_t B, int64_t M, int Q, int P,
                            const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y, const void* Z, int64_t strideS_Z,
                            const void* noise_var, int64_t strideS_noise, const void* qU_mean, int64_t strideS_mu,
                            const void* qU_cov_W, int64_t strideS_W, const void* qU_cov_diag, int64_t strideS_sd,
                            const void* lengthscale, int ard, int64_t strideS_ls, const void* variance, int64_t strideS_var,
                            double jitter, double scaling, double gscale, void* logL, int* info, int want_grad,
                            void* dX, void* dY, void* dZ, void* dnoise, void* dmu, void* dW, void* dSdiag, void* dls, void* dvar,
                            void* stream);

/* The same bound with heteroscedastic and/or per-output noise (svgp_regression.py:61-67: noise_var of shape (N, D'), D' in {1, D};
 * testing/modules/svgpregression_test.py:142-167).  noise_var is (noise_rows, noise_cols) with noise_rows in {1, B} and noise_cols in {1, P},
 * shared by all samples; dnoise has the same shape.  Per-row noise (B, 1) with one output column in float32 (want_grad, Q <= 8, B % 16 == 0,
 * M % 16 == 0, M >= 128, explicit form) STREAMS (r04): with nmin = min noise and r_n = nmin / noise_n the Gram planes are written as
 * Kuf diag(sqrt r) and diag(r) Kfu, the homoscedastic split products and fused reverse pass run with noise := nmin, and one extra pass
 * over the Kfu planes and T forms sum_n e_n^2 / noise_n and the (B, 1) noise gradient (8.4 vs 26.2 ms at B = 65 536, M = 1 024, S = 8).
 * Every other shape: the generic (materialised dKuf) path, same results.                                                             */
int mxf_svgp_logpdf_het(mxf_handle h, int kind, int dtype, int S, int64_t B, int64_t M, int Q, int P,
                        const void* X, int64_t strideS_X, const void* Y, int64_t strideS_Y,
                        const void* Z, const void* noise_var, int64_t noise_rows, int noise_cols,
                        const void* qU_mean, const void* qU_cov_W, const void* qU_cov_diag, const void* lengthscale, int ard,
                        const void* variance, double jitter, double scaling, double gscale,
                        void* logL, int* info, int want_grad,
                        void* dX, void* dY, void* dZ, void* dnoise, void* dmu, void* dW, void* dSdiag,
                        void* dls, void* dvar, void* stream);

/* The same bound from MATERIALISED Gram matrices, ONE sample per call: for kernels whose K is composed on the host
 * (AddKernel / MultiplyKernel, add_kernel.py:44-68, multiply_kernel.py:44-67 -- the deep-GP configuration's Matern52+RBF).
 *   Kuu (M,M) WITHOUT jitter (added here, svgp_regression.py:70-72), Kuf (M,B), Kdiag (B), Y (S,B,P) [minus mean]: S samples of the
 *   outputs over the SAME inputs (a hidden layer of a deep GP); logL (S), dY (S,B,P); the other gradients are summed over the samples;
 *   noise_var (noise_rows, noise_cols) as above.
 * if want_grad: gscale * d logL / d(.) WRITTEN into dKuu (M,M) dKuf (M,B) dKdiag (B) dY dnoise dmu dW dSdiag; the caller chains
 * dKuu / dKuf / dKdiag into the kernels' own reverse mode (mxf_gram_bwd).                                                        */
int mxf_svgp_logpdf_mat(mxf_handle h, int dtype, int S, int64_t B, int64_t M, int P, const void* Kuu, const void* Kuf, const void* Kdiag,
                        const void* Y, int64_t strideS_Y, const void* noise_var, int64_t noise_rows, int noise_cols, const void* qU_mean,
                        const void* qU_cov_W, const void* qU_cov_diag, double jitter, double scaling, double gscale, void* logL,
                        int* info, int want_grad, void* dKuu, void* dKuf, void* dKdiag, void* dY, void* dnoise, void* dmu,
                        void* dW, void* dSdiag, void* stream);

/* SparseGPRegressionLogPdf.compute (modules/gp_modules/sparsegp_regression.py:42-108), Titsias bound, ONE sample
 * (callers loop over samples), stationary kernel, sufficient-statistics form with C = Kuu + Psi2/noise.
 *   X (B,Q)  Y (B,P) [minus mean]  Z (M,Q)  noise_var (1)  lengthscale (Q|1)  variance (1)
 * outputs: logL (1); the posterior side products of :99-106: wv (M,P), L (M,M), LA (M,M) (any may be NULL);
 * if want_grad: gscale * d logL / d(.) WRITTEN into dX (B,Q) dY (B,P) dZ (M,Q) dnoise (1) dls (Q|1) dvar (1).       */
int mxf_sgp_logpdf(mxf_handle h, int kind, int dtype, int64_t B, int64_t M, int Q, int P, const void* X, const void* Y,
                   const void* Z, const void* noise_var, const void* lengthscale, int ard, const void* variance,
                   double jitter, double gscale, void* logL, void* wv, void* L, void* LA, int* info, int want_grad,
                   void* dX, void* dY, void* dZ, void* dnoise, void* dls, void* dvar, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MXF_GP_H */
