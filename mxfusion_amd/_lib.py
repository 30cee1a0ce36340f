"""ctypes binding of libmxf_gp.so (include/mxf_gp.h).  There is NO CPU fallback: if the HIP library is
missing or no GPU is present the product path raises."""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MXF_GP_LIB', os.path.join(_HERE, 'libmxf_gp.so'))   # env override: A/B builds of the kernels

F32, F64 = 0, 1
K_RBF, K_MATERN12, K_MATERN32, K_MATERN52, K_LINEAR, K_BIAS, K_WHITE = range(7)
WRITE, ACC_ADD, ACC_MUL = 0, 1, 2
KD_PERIODIC, KD_RQ, KD_SM = range(3)      # MXF_KD_*: the difference-form covariances (mxf_gram_diff)
GD_MAX_Q, GD_SM_MAX_Q, GD_SM_MAX_A = 16, 8, 8   # MXF_GD_MAX_Q, MXF_GD_SM_MAX_Q, MXF_GD_SM_MAX_A
ICM_MAX_T = 32             # MXF_ICM_MAX_T: outputs of the fused coregionalisation Gram pass (mxf_gram_icm)
D_GAMMA, D_GAMMA_MV, D_BETA, D_LAPLACE, D_UNIFORM, D_BERNOULLI, D_NORMAL_PREC = range(7)
TR_SOFTPLUS, TR_LOGISTIC = range(2)
LIK_BERNOULLI_LOGIT, LIK_BERNOULLI_PROBIT, LIK_POISSON_EXP = range(3)
LIK_MAX_NODES = 64         # MXF_LIK_MAX_NODES: quadrature nodes per call
ROBUSTMAX_MAX_C = 32       # MXF_ROBUSTMAX_MAX_C: classes of a robust-max row
PSI_MAX_Q = 16             # MXF_PSI_MAX_Q: input dimensions of the psi statistics
RFF_MAX_Q = 16             # MXF_RFF_MAX_Q: input dimensions of the random Fourier features
KMV_MAX_Q = 16             # MXF_KMV_MAX_Q: input dimensions of the matrix-free kernel product
NEAREST_MAX_Q = 16         # MXF_NEAREST_MAX_Q: input dimensions of the nearest-centre assignment
KNN_MAX_Q = 16             # MXF_KNN_MAX_Q: input dimensions of the k-nearest-neighbour search and of the Vecchia kernels
KNN_MAX_K = 32             # MXF_KNN_MAX_K: neighbours per row
VECCHIA_MAX_P = 32         # MXF_VECCHIA_MAX_P: output columns of the Vecchia kernels
TR_MAX_SEG = 32           # MXF_TR_MAX_SEG: segments per launch; a longer list takes further launches inside the call
ACT_IDENTITY, ACT_TANH, ACT_RELU, ACT_SIGMOID = range(4)
DENSE_MAX_WIDTH = 128
EW_ADD, EW_SUBTRACT, EW_MULTIPLY, EW_DIVIDE, EW_POWER, EW_SQUARE, EW_EXP, EW_LOG = range(8)
EW_MAX_RANK = 5            # MXF_EW_MAX_RANK
EW_MAX_ELEMS = 1 << 35     # the output, and the span of an operand
RED_SUM, RED_MEAN, RED_PROD = range(3)

_c = ctypes
_vp, _i, _i64, _d = _c.c_void_p, _c.c_int, _c.c_int64, _c.c_double
_p64 = _c.POINTER(_c.c_int64)          # a host array of extents or strides
_pi, _pd = _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)       # host arrays of a segment table

# name -> argtypes (after the handle); every entry point include/mxf_gp.h declares is listed here
SIGNATURES = {
    'mxf_gram': [_i, _i, _i, _i64, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _vp, _i64, _d, _i,
                 _vp, _i64, _i64, _vp],
    'mxf_gram2': [_i, _i, _i, _i, _i, _i64, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _vp, _i64, _d,
                  _vp, _i64, _i64, _vp],
    'mxf_gram_bwd': [_i, _i, _i, _i64, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _vp, _i64, _i64,
                     _vp, _vp, _vp, _vp, _vp],
    'mxf_gram_diff': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _vp, _i64, _d,
                      _vp, _i64, _i64, _vp],
    'mxf_gram_diff_bwd': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _vp, _i64, _i64,
                          _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_gram_icm': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _d,
                     _vp, _i64, _i64, _vp],
    'mxf_gram_icm_bwd': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64,
                         _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_gemm': [_i, _i, _i, _i64, _i64, _i64, _d, _vp, _i64, _i64, _vp, _i64, _i64, _d, _vp, _i64, _i64, _i, _vp],
    'mxf_potrf': [_i, _i, _i64, _vp, _i64, _i64, _vp, _vp],
    'mxf_trsm': [_i, _i, _i, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp],
    'mxf_trtri': [_i, _i, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp],
    'mxf_sumlogdiag': [_i, _i, _i64, _vp, _i64, _i64, _vp, _vp],
    'mxf_coldot': [_i, _i, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp],
    'mxf_kdiag': [_i, _i, _i, _i64, _i, _vp, _i64, _vp, _i, _i64, _vp, _i64, _vp, _vp],
    'mxf_gp_predict': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _i64, _vp, _vp, _i, _i, _vp, _vp, _vp],
    'mxf_svgp_predict': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _d, _i, _i, _vp, _vp, _vp, _vp],
    'mxf_softplus_fwd': [_i, _i64, _vp, _vp, _vp],
    'mxf_softplus_bwd': [_i, _i64, _vp, _vp, _vp, _vp],
    'mxf_normal_reparam': [_i, _i, _i64, _vp, _vp, _vp, _vp, _vp],
    'mxf_normal_logpdf': [_i, _i, _i64, _vp, _vp, _i64, _vp, _i64, _d, _vp, _vp, _vp, _vp, _vp],
    'mxf_univariate_logpdf': [_i, _i, _i, _i64, _vp, _vp, _i64, _vp, _i64, _d, _vp, _vp, _vp, _vp, _vp],
    'mxf_univariate_logpdf_elem': [_i, _i, _i, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _d, _vp, _vp],
    'mxf_univariate_logpdf_bwd': [_i, _i, _i, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _d, _vp, _vp, _vp, _vp],
    'mxf_univariate_logpdf_ps': [_i, _i, _i, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _d, _vp, _vp],
    'mxf_univariate_logpdf_ps_bwd': [_i, _i, _i, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _d, _vp, _vp, _vp, _vp],
    'mxf_normal_logpdf_ps': [_i, _i, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _d, _vp, _vp],
    'mxf_normal_logpdf_ps_bwd': [_i, _i, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _d, _vp, _vp, _vp, _vp],
    'mxf_lik_expect': [_i, _i, _i, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _i, _pd, _pd, _vp, _d, _vp, _vp, _vp, _vp],
    'mxf_lik_expect_elem': [_i, _i, _i, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _i, _pd, _pd, _d, _vp, _vp],
    'mxf_lik_moments': [_i, _i, _i, _i64, _i, _vp, _i64, _vp, _i64, _i, _pd, _pd, _vp, _vp, _vp],
    'mxf_robustmax_expect': [_i, _i, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _i, _pd, _pd, _d, _vp, _d, _vp, _vp, _vp, _vp],
    'mxf_robustmax_probs': [_i, _i, _i64, _i, _vp, _i64, _vp, _i64, _i, _pd, _pd, _vp, _vp],
    'mxf_psi_rbf_fwd': [_i, _i, _i64, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _vp, _vp, _vp],
    'mxf_psi_rbf_bwd': [_i, _i, _i64, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_psi_rbf_quad': [_i, _i, _i64, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _i, _vp, _i64, _vp, _vp],
    'mxf_rff_eval': [_i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp],
    'mxf_rff_eval_bwd': [_i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    'mxf_kmv': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp],
    'mxf_kmv_bwd': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _pd, _vp, _vp, _vp],
    'mxf_nearest': [_i, _i64, _i64, _i, _vp, _vp, _vp, _vp, _vp],
    'mxf_kmeans_step': [_i, _i64, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_knn': [_i, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    'mxf_vecchia_cond': [_i, _i, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_vecchia_logpdf': [_i, _i, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_vecchia_logpdf_bwd': [_i, _i, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_mvn_factor': [_i, _i, _i, _i64, _i, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    'mxf_mvn_logpdf': [_i, _i, _i, _i64, _i, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _i, _i64, _d, _vp, _vp],
    'mxf_mvn_logpdf_bwd': [_i, _i, _i, _i64, _i, _vp, _i64, _vp, _i64, _i64, _vp, _i, _i64, _vp, _d, _vp, _vp, _vp, _vp],
    'mxf_wishart_logpdf': [_i, _i, _i64, _i, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i, _i64, _d, _vp, _vp, _vp],
    'mxf_wishart_logpdf_bwd': [_i, _i, _i64, _i, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i, _i64, _vp, _d, _vp, _vp, _vp, _vp],
    'mxf_categorical_logpdf': [_i, _i, _i64, _i, _vp, _i64, _i64, _vp, _i64, _i, _i, _d, _vp, _vp],
    'mxf_categorical_logpdf_bwd': [_i, _i, _i64, _i, _vp, _i64, _i64, _vp, _i64, _i, _i, _vp, _d, _vp, _vp, _vp],
    'mxf_dirichlet_logpdf': [_i, _i, _i64, _i, _vp, _i64, _vp, _i64, _i64, _i, _d, _vp, _vp],
    'mxf_dirichlet_logpdf_bwd': [_i, _i, _i64, _i, _vp, _i64, _vp, _i64, _i64, _i, _vp, _d, _vp, _vp, _vp],
    'mxf_dense_fwd': [_i, _i, _i64, _i, _i, _i, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp],
    'mxf_dense_bwd': [_i, _i, _i64, _i, _i, _i, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_ewise_fwd': [_i, _i, _i, _p64, _vp, _p64, _vp, _p64, _vp, _vp],
    'mxf_ewise_bwd': [_i, _i, _i, _p64, _vp, _p64, _vp, _p64, _vp, _vp, _vp, _vp],
    'mxf_reduce_fwd': [_i, _i, _i64, _i64, _i64, _vp, _vp, _vp],
    'mxf_reduce_bwd': [_i, _i, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    'mxf_normal_reparam_bwd': [_i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_normal_reparam_prec': [_i, _i, _i64, _vp, _vp, _vp, _vp, _vp],
    'mxf_normal_reparam_prec_bwd': [_i, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_transform_fwd': [_i, _i, _pi, _p64, _pd, _pd, _vp, _vp, _vp],
    'mxf_transform_bwd': [_i, _i, _pi, _p64, _pd, _pd, _vp, _vp, _vp, _vp],
    'mxf_adam_step': [_i, _i64, _vp, _vp, _vp, _vp, _d, _d, _d, _d, _d, _i, _vp],
    'mxf_sgd_step': [_i, _i64, _vp, _vp, _vp, _d, _d, _d, _d, _vp],
    'mxf_opt_step': [_i, _i, _i64, _vp, _vp, _vp, _vp, _d, _d, _d, _d, _d, _vp],
    'mxf_uniform_sum': [_i, _i64, _vp, _vp, _vp],
    'mxf_gp_logpdf': [_i, _i, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i, _i64, _vp, _i64, _d,
                      _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_svgp_logpdf': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp,
                        _d, _d, _d, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_svgp_logpdf_sampled': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i, _i64,
                                _vp, _i64, _d, _d, _d, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_gram_planes': [_i, _i64, _i64, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i64, _vp, _vp, _i64, _vp],
    'mxf_f32x3_split': [_i64, _i64, _vp, _i64, _vp, _vp],
    'mxf_gemm_f32x3_planes': [_i64, _i64, _i64, _d, _vp, _vp, _d, _vp, _i64, _i, _vp],
    'mxf_gemm_f32x3': [_i64, _i64, _i64, _d, _vp, _i64, _vp, _i64, _d, _vp, _i64, _i, _vp],
    'mxf_make_diagonal': [_i, _i64, _i64, _vp, _vp, _vp],
    'mxf_diag_of': [_i, _i64, _i64, _vp, _vp, _vp],
    'mxf_gemm_f16x2': [_i64, _i64, _i64, _d, _vp, _i64, _vp, _i64, _d, _vp, _i64, _i, _vp],
    'mxf_f16x2_split': [_i64, _i64, _vp, _i64, _vp, _vp, _vp],
    'mxf_gemm_f16x2_planes': [_i64, _i64, _i64, _d, _vp, _vp, _vp, _vp, _d, _vp, _i64, _i, _vp],
    'mxf_gemm_f16x2_planes_kmajor': [_i64, _i64, _i64, _d, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp],
    'mxf_svgp_logpdf_het': [_i, _i, _i, _i64, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i, _vp,
                            _d, _d, _d, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_svgp_logpdf_mat': [_i, _i, _i64, _i64, _i, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i, _vp, _vp, _vp, _d, _d, _d, _vp, _vp, _i,
                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_sgp_logpdf': [_i, _i, _i64, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _d, _d, _vp, _vp, _vp, _vp, _vp, _i,
                       _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_svgp_last_cond': [_c.POINTER(_d)],
    'mxf_svgp_cond_nowait': [_c.POINTER(_d), _i],
    'mxf_svgp_configure': [_i, _i],
    'mxf_svgp_timing': [_i],
    'mxf_svgp_timing_read': [_c.POINTER(_d)],
    'mxf_svgp_cond_slot': [_i, _c.POINTER(_d), _c.POINTER(_d), _i],
    'mxf_gemm_f16x2_planes_out': [_i64, _i64, _i64, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    'mxf_f16x2_planes_transpose': [_i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
    'mxf_comm_unique_id': [_vp],
    'mxf_comm_init': [_i, _i, _vp],
    'mxf_allreduce_sum': [_i, _vp, _i64, _vp],
    'mxf_bcast': [_i, _vp, _i64, _i, _vp],
    'mxf_comm_destroy': [],
}
PLAIN = {  # entry points without the (handle, ...) -> int shape
    'mxf_version': ([], _i),
    'mxf_create': ([_i, _c.POINTER(_vp)], _i),
    'mxf_destroy': ([_vp], _i),
    'mxf_last_error': ([_vp], _c.c_char_p),
    'mxf_workspace_bytes': ([_vp], _i64),
    'mxf_workspace_generation': ([_vp], _i64),
    'mxf_f32x3_plane_elems': ([_i64, _i64], _i64),
    'mxf_svgp_whitened_ok': ([_i, _i, _i64, _i64, _i, _i, _i64], _i),
}
ALL_SYMBOLS = sorted(list(SIGNATURES) + list(PLAIN))

_lib = None
_lock = threading.Lock()
_handles = {}


class MXFError(RuntimeError):
    pass


def load():
    """dlopen libmxf_gp.so and declare prototypes.  Raises (loudly) when the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise MXFError('libmxf_gp.so not found at %s -- build it with `python -c "import __graft_entry__ as g; '
                           'g.build()"` (or make -C mxfusion_amd/csrc). There is no CPU fallback.' % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (args, res) in PLAIN.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, res
        for name, args in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise MXFError('libmxf_gp.so does not export %s' % name)
            fn.argtypes, fn.restype = [_vp] + args, _i
        _lib = lib
    return _lib


def handle(device_index):
    """One library handle per (thread, device): handle calls are not re-entrant (include/mxf_gp.h)."""
    key = (threading.get_ident(), int(device_index))
    h = _handles.get(key)
    if h is None:
        lib = load()
        out = _vp()
        rc = lib.mxf_create(int(device_index), ctypes.byref(out))
        if rc != 0:
            raise MXFError('mxf_create(device=%d) failed with %d: no usable MI355X visible. There is no CPU '
                           'fallback.' % (device_index, rc))
        h = out
        _handles[key] = h
    return h


def workspace_generation(device_index):
    """Re-allocation count of the (thread, device) handle's scratch (mxf_workspace_generation): hipGraph holders compare it before a
    replay -- a captured launch carries the scratch addresses of capture time."""
    return int(load().mxf_workspace_generation(handle(device_index)))


def svgp_cond_nowait(device_index, reset=False):
    """Running maximum of cond_1(Kuu + jitter I) over the SVGP training calls finished so far on this (thread, device) handle
    (mxf_svgp_cond_nowait: a read of pinned host memory, no synchronisation)."""
    out = _d(0.0)
    call('mxf_svgp_cond_nowait', handle(device_index), ctypes.byref(out), int(bool(reset)))
    return float(out.value)


FORM_EXPLICIT, FORM_WHITENED = 0, 1
COND_SLOTS = 64


def svgp_configure(device_index, form, slot):
    """Float32 streaming form (FORM_EXPLICIT / FORM_WHITENED) and condition slot of the next SVGP training calls of this (thread, device)
    handle (mxf_svgp_configure)."""
    call('mxf_svgp_configure', handle(device_index), int(form), int(slot))


def svgp_cond_slot(device_index, slot, reset=False):
    """(last, running max) of the condition numbers the finished training calls published into `slot` -- no synchronisation
    (mxf_svgp_cond_slot)."""
    last, mx = _d(0.0), _d(0.0)
    call('mxf_svgp_cond_slot', handle(device_index), int(slot), ctypes.byref(last), ctypes.byref(mx), int(bool(reset)))
    return float(last.value), float(mx.value)


TIMING_KEYS = ('planes_a', 'psi2', 'planes_b', 't_gemm', 'reverse_pass', 'core_chain', 'v_gemm', 'call')


def svgp_timing(device_index, enable):
    call('mxf_svgp_timing', handle(device_index), int(bool(enable)))


def svgp_timing_read(device_index):
    """In-step durations (ms) of the last SVGP training call's bulk kernels (mxf_svgp_timing_read; synchronises); absent stages are dropped."""
    buf = (_d * 8)()
    call('mxf_svgp_timing_read', handle(device_index), buf)
    return {k: float(buf[i]) for i, k in enumerate(TIMING_KEYS) if buf[i] >= 0}


def svgp_whitened_ok(dtype, S, B, M, Q, P, stride_x):
    return bool(load().mxf_svgp_whitened_ok(int(dtype), int(S), int(B), int(M), int(Q), int(P), int(stride_x)))


def svgp_last_cond(device_index):
    """1-norm condition number of Kuu + jitter I of the last SVGP training call on this (thread, device) handle (mxf_svgp_last_cond;
    synchronises)."""
    out = _d(0.0)
    call('mxf_svgp_last_cond', handle(device_index), ctypes.byref(out))
    return float(out.value)


def call(name, h, *args):
    lib = load()
    rc = getattr(lib, name)(h, *args)
    if rc != 0:
        raise MXFError('%s failed (%d): %s' % (name, rc, lib.mxf_last_error(h).decode()))
