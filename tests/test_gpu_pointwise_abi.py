"""The C ABI of the pointwise and per-row entry points (elementwise.hip, ewise.hip, simplex.hip, univariate.hip, mvn.hip, wishart.hip,
dense.hip, transform.hip) on the MI355X, called through _lib.load(): the status and the mxf_last_error text of every refusal, which check wins
where two apply, the 0 of an empty call, and that the pre-filled output and accumulator buffers are untouched after all of them.  Every
call here is refused on the host before any launch or is a valid launch of a handful of elements (S = 2, n = 5, B = 3, K = 4); the
expectations were written against the launchers as they stood before their plans were split out, and hold for either library."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F64, BAD = 1, 7
S, N, B, K, FILL = 2, 5, 3, 4, 123.0
SRC, SINK, OUT, NULL = 'src', 'sink', 'out', None      # device buffers: operands (0.5 everywhere), guarded outputs, outputs of the valid launches


def i64s(*v):
    return (ctypes.c_int64 * len(v))(*v)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def dbls(*v):
    return (ctypes.c_double * len(v))(*v)


# name -> the arguments of a valid call after the handle, in order and by name (the stream is appended)
UNI = [('kind', 0), ('dtype', F64), ('S', S), ('n', N), ('x', SRC), ('a', SRC), ('n_a', N), ('ss_a', 0), ('b', SRC), ('n_b', 1), ('ss_b', 0)]
NORMAL_PS = [(k, v) for k, v in UNI if k != 'kind']
MVN = [('dtype', F64), ('form', 0), ('S', S), ('B', B), ('n', 4), ('x', SRC), ('ss_x', 12), ('mean', SRC), ('ss_m', 12), ('sb_m', 4), ('F', SRC)]
WISH = [('dtype', F64), ('S', S), ('B', B), ('n', 4), ('X', SRC), ('ldx', 4), ('ss_X', 48), ('dof', SRC), ('ss_d', 3), ('sb_d', 1), ('V', SRC), ('ldv', 4),
        ('ss_V', 48), ('sb_V', 16), ('S_V', S), ('B_V', B)]
CAT = [('dtype', F64), ('S', S), ('B', B), ('K', K), ('logp', SRC), ('ss_lp', 12), ('sb_lp', 4), ('x', SRC), ('ss_x', 12), ('one_hot', 1), ('normalize', 1)]
DIR = [('dtype', F64), ('S', S), ('B', B), ('K', K), ('x', SRC), ('ss_x', 12), ('alpha', SRC), ('ss_a', 12), ('sb_a', 4), ('normalize', 1)]
DENSE = [('dtype', F64), ('S', S), ('N', N), ('I', 3), ('O', 4), ('act', 1), ('X', SRC), ('ldx', 3), ('ss_x', 15), ('W', SRC), ('ss_w', 12)]
EW = [('op', 0), ('dtype', F64), ('rank', 2), ('extent', i64s(3, 5)), ('x', SRC), ('sx', i64s(5, 1)), ('y', SRC), ('sy', i64s(0, 1))]
RED = [('kind', 0), ('dtype', F64), ('outer', 2), ('R', 4), ('inner', 3), ('x', SRC)]
TR = [('dtype', F64), ('nseg', 2), ('kinds', ints(0, 1)), ('sizes', i64s(3, 2)), ('p0', dbls(0.0, -1.0)), ('p1', dbls(0.0, 2.0)), ('x', SRC)]
OPT = [('w', SINK), ('g', SRC)]
ENTRIES = {
    'mxf_softplus_fwd': [('dtype', F64), ('n', N), ('x', SRC), ('y', SINK)],
    'mxf_softplus_bwd': [('dtype', F64), ('n', N), ('x', SRC), ('dy', SRC), ('dx', SINK)],
    'mxf_normal_reparam': [('dtype', F64), ('S', S), ('n', N), ('mean', SRC), ('var', SRC), ('eps', SRC), ('x', SINK)],
    'mxf_normal_reparam_bwd': [('dtype', F64), ('S', S), ('n', N), ('var', SRC), ('eps', SRC), ('dx', SRC), ('dmean', SINK), ('dvar', SINK)],
    'mxf_normal_reparam_prec': [('dtype', F64), ('S', S), ('n', N), ('mean', SRC), ('prec', SRC), ('eps', SRC), ('x', SINK)],
    'mxf_normal_reparam_prec_bwd': [('dtype', F64), ('S', S), ('n', N), ('prec', SRC), ('eps', SRC), ('dx', SRC), ('dmean', SINK), ('dprec', SINK)],
    'mxf_normal_logpdf': [('dtype', F64), ('S', S), ('n', N), ('x', SRC), ('mean', SRC), ('n_mean', N), ('var', SRC), ('n_var', 1), ('scale', 1.0),
                          ('out', SINK), ('dx', SINK), ('dmean', SINK), ('dvar', SINK)],
    'mxf_normal_logpdf_ps': NORMAL_PS + [('scale', 1.0), ('out', SINK)],
    'mxf_normal_logpdf_ps_bwd': NORMAL_PS + [('w', SRC), ('scale', 1.0), ('dx', SINK), ('da', SINK), ('db', SINK)],
    'mxf_adam_step': [('dtype', F64), ('n', N)] + OPT + [('m', SINK), ('v', SINK), ('lr', 0.1), ('b1', 0.9), ('b2', 0.99), ('eps', 1e-8), ('rescale', 1.0), ('t', 1)],
    'mxf_uniform_sum': [('dtype', F64), ('n', N), ('g', SRC), ('out', SINK)],
    'mxf_sgd_step': [('dtype', F64), ('n', N)] + OPT + [('mom', SINK), ('lr', 0.1), ('momentum', 0.9), ('wd', 0.0), ('rescale', 1.0)],
    'mxf_opt_step': [('kind', 1), ('dtype', F64), ('n', N)] + OPT + [('s1', SINK), ('s2', SINK), ('lr', 0.1), ('p1', 0.9), ('eps', 1e-8), ('wd', 0.0), ('rescale', 1.0)],
    'mxf_coldot': [('dtype', F64), ('S', S), ('M', 64), ('N', N), ('A', SRC), ('lda', N), ('sA', 64 * N), ('B', SRC), ('ldb', N), ('sB', 64 * N), ('out', SINK)],
    'mxf_make_diagonal': [('dtype', F64), ('batch', B), ('n', 4), ('a', SRC), ('out', SINK)],
    'mxf_diag_of': [('dtype', F64), ('batch', B), ('n', 4), ('g', SRC), ('out', SINK)],
    'mxf_univariate_logpdf': [(k, v) for k, v in UNI if not k.startswith('ss_')] + [('scale', 1.0), ('out', SINK), ('dx', SINK), ('da', SINK), ('db', SINK)],
    'mxf_univariate_logpdf_elem': UNI + [('scale', 1.0), ('out', SINK)],
    'mxf_univariate_logpdf_bwd': UNI + [('cot', SRC), ('scale', 1.0), ('dx', SINK), ('da', SINK), ('db', SINK)],
    'mxf_univariate_logpdf_ps': UNI + [('scale', 1.0), ('out', SINK)],
    'mxf_univariate_logpdf_ps_bwd': UNI + [('w', SRC), ('scale', 1.0), ('dx', SINK), ('da', SINK), ('db', SINK)],
    'mxf_mvn_factor': [('dtype', F64), ('form', 0), ('S_A', S), ('B_A', B), ('n', 4), ('A', SRC), ('lda', 4), ('ss_A', 48), ('sb_A', 16), ('F', SINK),
                       ('logdet', SINK), ('info', SINK)],
    'mxf_mvn_logpdf': MVN + [('logdet', SRC), ('S_A', S), ('B_A', B), ('scale', 1.0), ('out', SINK)],
    'mxf_mvn_logpdf_bwd': MVN + [('S_A', S), ('B_A', B), ('cot', SRC), ('scale', 1.0), ('dx', SINK), ('dmean', SINK), ('dA', SINK)],
    'mxf_wishart_logpdf': WISH + [('scale', 1.0), ('out', SINK), ('info', SINK)],
    'mxf_wishart_logpdf_bwd': WISH + [('cot', SRC), ('scale', 1.0), ('dX', SINK), ('ddof', SINK), ('dV', SINK)],
    'mxf_categorical_logpdf': CAT + [('scale', 1.0), ('out', SINK)],
    'mxf_categorical_logpdf_bwd': CAT + [('cot', SRC), ('scale', 1.0), ('dlogp', SINK), ('dx', SINK)],
    'mxf_dirichlet_logpdf': DIR + [('scale', 1.0), ('out', SINK)],
    'mxf_dirichlet_logpdf_bwd': DIR + [('cot', SRC), ('scale', 1.0), ('dx', SINK), ('dalpha', SINK)],
    'mxf_dense_fwd': DENSE + [('b', SRC), ('ss_b', 4), ('Y', SINK)],
    'mxf_dense_bwd': DENSE + [('ss_b', 4), ('Y', SRC), ('dY', SRC), ('dX', SINK), ('dW', SINK), ('db', SINK)],
    'mxf_ewise_fwd': EW + [('z', SINK)],
    'mxf_ewise_bwd': EW + [('dz', SRC), ('dx', SINK), ('dy', SINK)],
    'mxf_reduce_fwd': RED + [('y', SINK)],
    'mxf_reduce_bwd': RED + [('dy', SRC), ('dx', SINK)],
    'mxf_transform_fwd': TR + [('y', SINK)],
    'mxf_transform_bwd': TR + [('dy', SRC), ('dx', SINK)],
}

ORDER_N = 'order n = 33 is outside 1..32 (larger matrices take mxf_potrf / mxf_trsm)'
UNI_STRIDE = "a parameter's sample stride must be 0, or n with n elements per sample"
NO_GRADS = {'mxf_mvn_logpdf_bwd': ('dx', 'dmean', 'dA'), 'mxf_wishart_logpdf_bwd': ('dX', 'ddof', 'dV'), 'mxf_categorical_logpdf_bwd': ('dlogp', 'dx'),
            'mxf_dirichlet_logpdf_bwd': ('dx', 'dalpha'), 'mxf_dense_bwd': ('dX', 'dW', 'db'), 'mxf_ewise_bwd': ('dx', 'dy'), 'mxf_reduce_bwd': ('dx',)}

# (entry, overrides, status, text after "<entry>: "); the first override is the check that wins where a case trips two
CASES = [
    ('mxf_softplus_fwd', dict(n=0, dtype=BAD), 0, None),
    ('mxf_softplus_bwd', dict(n=0, dtype=BAD), 0, None),
    ('mxf_normal_reparam', dict(S=0, dtype=BAD), 0, None),
    ('mxf_normal_reparam_bwd', dict(n=0, dtype=BAD), 0, None),
    ('mxf_normal_reparam_prec', dict(n=0, mean=NULL), 0, None),
    ('mxf_normal_reparam_prec', dict(mean=NULL, dtype=BAD), -2, 'null argument'),
    ('mxf_normal_reparam_prec', dict(x=NULL), -2, 'null argument'),
    ('mxf_normal_reparam_prec_bwd', dict(S=0, eps=NULL), 0, None),
    ('mxf_normal_reparam_prec_bwd', dict(eps=NULL, dtype=BAD), -2, 'null argument'),
    ('mxf_normal_logpdf', dict(n=0, n_mean=2), 0, None),
    ('mxf_normal_logpdf', dict(n_mean=2, dtype=BAD), -2, 'mean/var must have 1 or n elements'),
    ('mxf_normal_logpdf', dict(n_var=N + 1), -2, 'mean/var must have 1 or n elements'),
    ('mxf_normal_logpdf_ps', dict(n=0, out=NULL), 0, None),
    ('mxf_normal_logpdf_ps', dict(out=NULL, dtype=BAD), -2, 'null out'),
    ('mxf_normal_logpdf_ps', dict(dtype=BAD, x=NULL), -2, 'bad dtype 7'),
    ('mxf_normal_logpdf_ps', dict(x=NULL, n_a=2), -2, 'null x or parameter'),
    ('mxf_normal_logpdf_ps', dict(n_a=2, ss_a=3), -2, 'the parameters must have 1 or n elements'),
    ('mxf_normal_logpdf_ps', dict(ss_a=3), -2, UNI_STRIDE),
    ('mxf_normal_logpdf_ps', dict(ss_b=N), -2, UNI_STRIDE),
    ('mxf_normal_logpdf_ps_bwd', dict(S=0, w=NULL), 0, None),
    ('mxf_normal_logpdf_ps_bwd', dict(w=NULL, dtype=BAD), -2, 'null weights'),
    ('mxf_adam_step', dict(n=0, t=0), 0, None),
    ('mxf_adam_step', dict(t=0, dtype=BAD), -2, 't must be >= 1'),
    ('mxf_uniform_sum', dict(n=0), -2, 'bad argument'),
    ('mxf_uniform_sum', dict(g=NULL, dtype=BAD), -2, 'bad argument'),
    ('mxf_uniform_sum', dict(out=NULL), -2, 'bad argument'),
    ('mxf_sgd_step', dict(n=0, dtype=BAD), 0, None),
    ('mxf_opt_step', dict(n=0, kind=9), 0, None),
    ('mxf_opt_step', dict(s1=NULL, kind=9), -2, 'null argument'),
    ('mxf_opt_step', dict(kind=3, s2=NULL), -2, 'null argument'),
    ('mxf_opt_step', dict(kind=9, dtype=BAD), -2, 'unknown optimiser kind 9'),
    ('mxf_opt_step', dict(kind=0), -2, 'unknown optimiser kind 0'),
    ('mxf_opt_step', dict(kind=4, dtype=BAD), -2, 'bad dtype 7'),
    ('mxf_coldot', dict(S=0, dtype=BAD), 0, None),
    ('mxf_coldot', dict(N=0, dtype=BAD), 0, None),
    ('mxf_coldot', dict(M=5, dtype=BAD), -2, 'bad dtype 7'),
    ('mxf_make_diagonal', dict(batch=0, dtype=BAD), 0, None),
    ('mxf_diag_of', dict(n=0, dtype=BAD), 0, None),
    ('mxf_univariate_logpdf', dict(n=0, kind=9), 0, None),
    ('mxf_univariate_logpdf', dict(kind=7, dtype=BAD), -2, 'unknown distribution kind 7'),
    ('mxf_univariate_logpdf', dict(kind=-1), -2, 'unknown distribution kind -1'),
    ('mxf_univariate_logpdf', dict(dtype=BAD, x=NULL), -2, 'bad dtype 7'),
    ('mxf_univariate_logpdf', dict(b=NULL, n_b=2), -2, 'null x or parameter'),
    ('mxf_univariate_logpdf', dict(n_b=2), -2, 'the parameters must have 1 or n elements'),
    ('mxf_univariate_logpdf_elem', dict(S=0, out=NULL), 0, None),
    ('mxf_univariate_logpdf_elem', dict(out=NULL, kind=9), -2, 'null out'),
    ('mxf_univariate_logpdf_elem', dict(kind=9, ss_a=3), -2, 'unknown distribution kind 9'),
    ('mxf_univariate_logpdf_elem', dict(ss_a=3), -2, UNI_STRIDE),
    ('mxf_univariate_logpdf_bwd', dict(cot=NULL, kind=9), -2, 'null cotangent'),
    ('mxf_univariate_logpdf_ps', dict(out=NULL, dtype=BAD), -2, 'null out'),
    ('mxf_univariate_logpdf_ps_bwd', dict(w=NULL, dtype=BAD), -2, 'null weights'),
    ('mxf_univariate_logpdf_ps_bwd', dict(n=0, w=NULL), 0, None),
    ('mxf_mvn_factor', dict(dtype=BAD, form=2), -2, 'bad dtype 7'),
    ('mxf_mvn_factor', dict(form=2, n=33), -2, 'form is 0 (covariance) or 1 (precision), got 2'),
    ('mxf_mvn_factor', dict(n=33, S_A=0), -3, ORDER_N),
    ('mxf_mvn_factor', dict(n=0), -3, 'order n = 0 is outside 1..32 (larger matrices take mxf_potrf / mxf_trsm)'),
    ('mxf_mvn_factor', dict(S_A=0, A=NULL), 0, None),
    ('mxf_mvn_factor', dict(info=NULL, lda=3), -2, 'null operand'),
    ('mxf_mvn_factor', dict(lda=3), -2, 'lda 3 < n = 4, or a negative stride'),
    ('mxf_mvn_factor', dict(sb_A=-1), -2, 'lda 4 < n = 4, or a negative stride'),
    ('mxf_mvn_logpdf', dict(n=33, B=0), -3, ORDER_N),
    ('mxf_mvn_logpdf', dict(B=0, x=NULL), 0, None),
    ('mxf_mvn_logpdf', dict(x=NULL, S_A=5), -2, 'null operand'),
    ('mxf_mvn_logpdf', dict(S_A=5, ss_x=-1), -2, 'the matrices have 1 or S samples and 1 or B batch entries, got (5, 3)'),
    ('mxf_mvn_logpdf', dict(ss_x=-1, out=NULL), -2, 'negative stride'),
    ('mxf_mvn_logpdf', dict(out=NULL), -2, 'null out or logdet'),
    ('mxf_mvn_logpdf', dict(logdet=NULL), -2, 'null out or logdet'),
    ('mxf_mvn_logpdf_bwd', dict(form=3, cot=NULL), -2, 'form is 0 (covariance) or 1 (precision), got 3'),
    ('mxf_mvn_logpdf_bwd', dict(B_A=2, cot=NULL), -2, 'the matrices have 1 or S samples and 1 or B batch entries, got (2, 2)'),
    ('mxf_mvn_logpdf_bwd', dict(cot=NULL), -2, 'null cotangent'),
    ('mxf_wishart_logpdf', dict(dtype=BAD, n=33), -2, 'bad dtype 7'),
    ('mxf_wishart_logpdf', dict(n=33, S=0), -3, ORDER_N),
    ('mxf_wishart_logpdf', dict(S=0, X=NULL), 0, None),
    ('mxf_wishart_logpdf', dict(dof=NULL, S_V=5), -2, 'null operand'),
    ('mxf_wishart_logpdf', dict(S_V=5, ldx=3), -2, 'the scale matrices have 1 or S samples and 1 or B batch entries, got (5, 3)'),
    ('mxf_wishart_logpdf', dict(ldx=3, ss_X=-1), -2, 'ldx 3 or ldv 4 < n = 4'),
    ('mxf_wishart_logpdf', dict(sb_V=-1, out=NULL), -2, 'negative stride'),
    ('mxf_wishart_logpdf', dict(info=NULL), -2, 'null out or info'),
    ('mxf_wishart_logpdf_bwd', dict(ldv=3, cot=NULL), -2, 'ldx 4 or ldv 3 < n = 4'),
    ('mxf_wishart_logpdf_bwd', dict(cot=NULL), -2, 'null cotangent'),
    ('mxf_categorical_logpdf', dict(dtype=BAD, K=0), -2, 'bad dtype 7'),
    ('mxf_categorical_logpdf', dict(K=0, S=0), -2, 'K = 0 classes, at least 1 is needed'),
    ('mxf_categorical_logpdf', dict(S=0, x=NULL), 0, None),
    ('mxf_categorical_logpdf', dict(x=NULL, ss_x=5), -2, 'null operand'),
    ('mxf_categorical_logpdf', dict(ss_x=5, sb_lp=3), -2, 'the sample stride of x is 0 or 12 (dense), got 5'),
    ('mxf_categorical_logpdf', dict(one_hot=0), -2, 'the sample stride of x is 0 or 3 (dense), got 12'),
    ('mxf_categorical_logpdf', dict(sb_lp=3, ss_lp=5), -2, 'the batch stride of the parameter is 0 or K = 4, got 3'),
    ('mxf_categorical_logpdf', dict(sb_lp=0, out=NULL), -2, 'the sample stride of the parameter is 0 or 4 (dense), got 12'),
    ('mxf_categorical_logpdf', dict(out=NULL), -2, 'null out'),
    ('mxf_categorical_logpdf_bwd', dict(one_hot=0, B=0), -2, 'dx_acc must be null without one-hot encoding (a label has no gradient)'),
    ('mxf_categorical_logpdf_bwd', dict(K=-1, one_hot=0), -2, 'K = -1 classes, at least 1 is needed'),
    ('mxf_categorical_logpdf_bwd', dict(B=0, logp=NULL), 0, None),
    ('mxf_categorical_logpdf_bwd', dict(ss_lp=5, cot=NULL), -2, 'the sample stride of the parameter is 0 or 12 (dense), got 5'),
    ('mxf_categorical_logpdf_bwd', dict(cot=NULL), -2, 'null cotangent'),
    ('mxf_dirichlet_logpdf', dict(dtype=BAD), -2, 'bad dtype 7'),
    ('mxf_dirichlet_logpdf', dict(alpha=NULL), -2, 'null operand'),
    ('mxf_dirichlet_logpdf', dict(ss_x=4), -2, 'the sample stride of x is 0 or 12 (dense), got 4'),
    ('mxf_dirichlet_logpdf', dict(out=NULL), -2, 'null out'),
    ('mxf_dirichlet_logpdf_bwd', dict(K=0, cot=NULL), -2, 'K = 0 classes, at least 1 is needed'),
    ('mxf_dirichlet_logpdf_bwd', dict(cot=NULL), -2, 'null cotangent'),
    ('mxf_dense_fwd', dict(dtype=BAD, I=0), -2, 'bad dtype 7'),
    ('mxf_dense_fwd', dict(I=0, act=4), -3, 'widths I = 0, O = 4; 1 .. 128 are supported'),
    ('mxf_dense_fwd', dict(O=129), -3, 'widths I = 3, O = 129; 1 .. 128 are supported'),
    ('mxf_dense_fwd', dict(act=4, S=0), -2, 'activation 4 (0 identity, 1 tanh, 2 relu, 3 sigmoid)'),
    ('mxf_dense_fwd', dict(N=0, Y=NULL), 0, None),
    ('mxf_dense_fwd', dict(Y=NULL, X=NULL), -2, 'null Y'),
    ('mxf_dense_fwd', dict(W=NULL, ldx=2), -2, 'null operand'),
    ('mxf_dense_fwd', dict(ldx=2, ss_x=1), -2, 'ldx = 2 < I = 3'),
    ('mxf_dense_fwd', dict(ss_x=14, ss_w=5), -2, 'the sample stride of X is 0 or at least (N - 1) ldx + I = 15, got 14'),
    ('mxf_dense_fwd', dict(ss_w=5, ss_b=3), -2, 'the sample stride of W is 0 or O I = 12 (dense), got 5'),
    ('mxf_dense_fwd', dict(ss_b=3), -2, 'the sample stride of b is 0 or O = 4, got 3'),
    ('mxf_dense_bwd', dict(S=0, dY=NULL), 0, None),
    ('mxf_dense_bwd', dict(dY=NULL, X=NULL), -2, 'null Y or dY'),
    ('mxf_dense_bwd', dict(X=NULL), -2, 'null operand'),
    ('mxf_dense_bwd', dict(ss_b=3), -2, 'the sample stride of b is 0 or O = 4, got 3'),
    ('mxf_ewise_fwd', dict(dtype=BAD, op=9), -2, 'bad dtype 7'),
    ('mxf_ewise_fwd', dict(op=8, rank=0), -2, 'op 8 (0 add .. 7 log)'),
    ('mxf_ewise_fwd', dict(rank=0, extent=NULL), -2, 'rank 0'),
    ('mxf_ewise_fwd', dict(rank=6, extent=NULL), -3, 'rank 6 after merging; up to 5 axes are supported'),
    ('mxf_ewise_fwd', dict(extent=NULL, z=NULL), -2, 'null operand, extent or stride array'),
    ('mxf_ewise_fwd', dict(y=NULL), -2, 'null operand, extent or stride array'),
    ('mxf_ewise_fwd', dict(extent=i64s(3, -5), z=NULL), -2, 'axis 1 has extent -5, strides 0, 0'),
    ('mxf_ewise_fwd', dict(sx=i64s(-5, 1), z=NULL), -2, 'axis 0 has extent 3, strides -5, 0'),
    ('mxf_ewise_fwd', dict(extent=i64s(3, (1 << 35) + 1)), -3, 'axis 1 is beyond 2^35 elements'),
    ('mxf_ewise_fwd', dict(extent=i64s(1 << 20, 1 << 16), sx=i64s(0, 0), z=NULL), -3, 'more than 2^35 elements'),
    ('mxf_ewise_fwd', dict(sx=i64s(1 << 34, 1 << 34), z=NULL), -3, 'an operand spans more than 2^35 elements'),
    ('mxf_ewise_fwd', dict(extent=i64s(3, 0), z=NULL), 0, None),
    ('mxf_ewise_fwd', dict(z=NULL), -2, 'null z'),
    ('mxf_ewise_fwd', dict(op=6, y=NULL, sy=NULL, z=NULL), -2, 'null z'),
    ('mxf_ewise_bwd', dict(extent=i64s(0, 5), dz=NULL), 0, None),
    ('mxf_ewise_bwd', dict(dz=NULL, dx=NULL, dy=NULL), -2, 'null dz'),
    ('mxf_ewise_bwd', dict(op=5, dx=NULL), 0, None),
    ('mxf_reduce_fwd', dict(dtype=BAD, kind=3), -2, 'bad dtype 7'),
    ('mxf_reduce_fwd', dict(kind=3, R=0), -2, 'kind 3 (0 sum, 1 mean, 2 prod)'),
    ('mxf_reduce_fwd', dict(R=0, outer=0), -2, 'extents (0, 0, 3)'),
    ('mxf_reduce_fwd', dict(outer=1 << 20, inner=1 << 15, x=NULL), -3, 'more than 2^35 elements'),
    ('mxf_reduce_fwd', dict(outer=0, x=NULL), 0, None),
    ('mxf_reduce_fwd', dict(x=NULL), -2, 'null x or y'),
    ('mxf_reduce_fwd', dict(y=NULL), -2, 'null x or y'),
    ('mxf_reduce_bwd', dict(inner=-1, dx=NULL), -2, 'extents (2, 4, -1)'),
    ('mxf_reduce_bwd', dict(inner=0, dy=NULL), 0, None),
    ('mxf_reduce_bwd', dict(dy=NULL), -2, 'null x or dy'),
    ('mxf_reduce_bwd', dict(kind=2, x=NULL), -2, 'null x or dy'),
    ('mxf_transform_fwd', dict(nseg=0, dtype=BAD), 0, None),
    ('mxf_transform_fwd', dict(dtype=BAD, kinds=NULL), -2, 'bad dtype 7'),
    ('mxf_transform_fwd', dict(p1=NULL, x=NULL), -2, 'null segment table'),
    ('mxf_transform_fwd', dict(kinds=ints(0, 5), sizes=i64s(3, -1)), -2, 'unknown transformation kind 5 (segment 1)'),
    ('mxf_transform_fwd', dict(sizes=i64s(-1, 2), p0=dbls(math.nan, 0.0)), -2, 'negative size (segment 0)'),
    ('mxf_transform_fwd', dict(p0=dbls(0.0, math.inf)), -2, 'p0 is not finite (segment 1)'),
    ('mxf_transform_fwd', dict(p1=dbls(0.0, 0.0)), -2, 'the lower bound is not below the upper bound (segment 1)'),
    ('mxf_transform_fwd', dict(dtype=0, p0=dbls(0.0, 1.00000001), p1=dbls(0.0, 1e-8), x=NULL), -2, 'no value of the working dtype lies between the bounds (segment 1)'),
    ('mxf_transform_fwd', dict(sizes=i64s(0, 0), x=NULL), 0, None),
    ('mxf_transform_fwd', dict(y=NULL), -2, 'null buffer'),
    ('mxf_transform_bwd', dict(kinds=ints(2, 0)), -2, 'unknown transformation kind 2 (segment 0)'),
    ('mxf_transform_bwd', dict(dy=NULL), -2, 'null buffer'),
]
CASES += [(e, dict(dtype=BAD), -2, 'bad dtype 7') for e in ENTRIES]                              # every entry point refuses an unknown dtype
CASES += [(e, dict.fromkeys(g, NULL), 0, None) for e, g in NO_GRADS.items()]                      # no gradient is wanted: nothing to do
# every entry point returns 0 on an empty call (mxf_uniform_sum refuses n = 0; the broadcast map's empty extents are in the table above)
EMPTY_KEYS = ('S', 'S_A', 'batch', 'nseg', 'outer', 'n')
CASES += [(e, {next(k for k in EMPTY_KEYS if k in dict(spec)): 0}, 0, None) for e, spec in ENTRIES.items()
          if e != 'mxf_uniform_sum' and not e.startswith('mxf_ewise')]


@pytest.fixture(scope='module')
def abi():
    from mxfusion_amd import _lib
    raw, h, stream = _lib.load(), _lib.handle(torch.cuda.current_device()), torch.cuda.current_stream().cuda_stream
    bufs = {SRC: torch.full((8192,), 0.5, dtype=torch.float64, device='cuda'), SINK: torch.full((8192,), FILL, dtype=torch.float64, device='cuda'),
            OUT: torch.zeros(8192, dtype=torch.float64, device='cuda')}

    def call(entry, **over):
        names = [k for k, _ in ENTRIES[entry]]
        assert set(over) <= set(names), (entry, set(over) - set(names))
        args = [over.get(k, v) for k, v in ENTRIES[entry]]
        args = [bufs[a].data_ptr() if isinstance(a, str) else a for a in args]
        rc = getattr(raw, entry)(h, *args, stream)
        return rc, raw.mxf_last_error(h).decode()
    call.bufs = bufs
    return call


def test_the_table_names_every_entry_point_of_the_eight_files():
    from mxfusion_amd import _lib
    assert len(ENTRIES) == 38 and set(ENTRIES) <= set(_lib.SIGNATURES)
    for e, spec in ENTRIES.items():
        assert len(spec) + 1 == len(_lib.SIGNATURES[e]), e
        assert any(c[0] == e and c[2] < 0 for c in CASES) and (e == 'mxf_uniform_sum' or any(c[0] == e and c[2] == 0 for c in CASES)), e


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_refusals_empty_calls_and_their_order(abi, entry):
    for e, over, rc, why in CASES:
        if e != entry:
            continue
        got, text = abi(entry, **over)
        assert got == rc, (entry, over, got, text)
        if rc:
            assert text == '%s: %s' % (entry, why), (entry, over)
    torch.cuda.synchronize()
    assert bool((abi.bufs[SINK] == FILL).all()) and bool((abi.bufs[SRC] == 0.5).all())


def test_valid_calls_of_a_handful_of_elements_launch(abi):
    """the tables' own calls with the outputs redirected: status 0, and the guarded buffers stay as they were"""
    for entry, spec in ENTRIES.items():
        over = {k: OUT for k, v in spec if v == SINK}
        if entry == 'mxf_mvn_factor':
            continue                                                             # (a constant matrix is not positive definite: nothing to pin here)
        rc, text = abi(entry, **over)
        assert rc == 0, (entry, rc, text)
    torch.cuda.synchronize()
    assert bool((abi.bufs[SINK] == FILL).all()) and bool((abi.bufs[SRC] == 0.5).all())
