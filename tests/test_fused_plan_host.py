"""CPU test of the plans of the row-owned launchers and of the per-sample grid (mxfusion_amd/csrc/fused_plan.h: plain C++, no HIP).
tests/host/fused_plan_check.cpp, built with the system C++ compiler, prints the plan of every request it reads.  Checked here: the launch
shapes the GPU cases of rff, kmv and the psi contraction were chosen for, every plan column over a sweep against a numpy transcription of the
launchers' arithmetic as it stood before the plans were split out of them, the invariants the kernels rely on, and every refusal's code and text."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RFF_IN = 'esize bwd S N D Q J ss_X ss_Om ss_ph ss_W has_X has_Om has_ph has_W has_out has_G has_dX'.split()
RFF_OUT = ('rc qp jb npass ch rows g0 g1 g2 own_X summed scratch_sum n_prep n_out n_dx ss_om ss_ph ss_wb at_om at_ph at_wb at_acc zero_bytes '
           'bytes').split()
KMV_IN = ('esize bwd S N N2 Q J ard ss_X ss_X2 ss_ls ss_var ss_da ss_V ss_A has_X has_X2 has_ls has_var has_da has_V has_out has_A has_w has_dls '
          'has_dvar').split()
KMV_OUT = ('rc qp jb npass square N2 ss_Z S_z S_V ch rows g0 g1 g2 gp n_prep_z n_out ss_zs ss_vb n_zero at_zs at_vb at_zero at_dv bytes '
           'np0 items0 np_last items_last').split()
PSI_IN = ('call esize S N M Q ard ss_mu ss_s ss_Z ss_ls ss_var has_mu has_s has_Z has_ls has_var has_Psi1 has_Psi2 has_G1 has_G2 has_dmu has_ds has_dZ '
          'has_dls has_dvar J ss_A has_A has_R').split()
PSI_OUT = ('rc qp n_prep n_mm g1_0 g1_1 g1_2 rch gp_0 gp_1 gp_2 mch gr_0 gr_1 gr_2 pairs_pass rows_pass wide fold close own_mu own_s own_Z own_l own_v '
           'n_mu n_s n_Z npass n_out split at_z at_zh at_rows at_acc at_wt at_l2 at_dv at_big at_zero zero_bytes bytes').split()
COLS = {'rff': (RFF_IN, RFF_OUT), 'kmv': (KMV_IN, KMV_OUT), 'psi': (PSI_IN, PSI_OUT)}

SIZES = (1, 63, 64, 65, 127, 128, 129, 4096, 70000, 1 << 20)
QS, JS, SS = (1, 4, 5, 8, 9, 16), (1, 4, 5, 16, 17, 70), (1, 2, 64, 65535)


@pytest.fixture(scope='module')
def check(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler found'
    exe = str(tmp_path_factory.mktemp('fused_plan') / 'fused_plan_check')
    subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'mxfusion_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host', 'fused_plan_check.cpp'), '-o', exe], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    return run


def plans(check, what, req):
    """the plan columns, as a dict of int64 arrays, of the requests given as a dict of equally long arrays (or scalars)"""
    cin, cout = COLS[what]
    assert set(req) == set(cin), set(req) ^ set(cin)
    table = np.stack(np.broadcast_arrays(*[np.asarray(req[k], dtype=np.int64) for k in cin]), axis=-1).reshape(-1, len(cin))
    out = check('\n'.join(what + ' ' + ' '.join(map(str, row)) for row in table.tolist()))
    got = np.array(out.split(), dtype=np.int64).reshape(table.shape[0], len(cout))
    return {k: got[:, i] for i, k in enumerate(cout)}


def refusal(check, what, **req):
    """(rc, text) of one request"""
    line = check('text 1\n%s %s\n' % (what, ' '.join(str(int(req[k])) for k in COLS[what][0]))).rstrip('\n')
    rc, _, why = line.partition(' ')
    return int(rc), why


def cross(**axes):
    grid = np.meshgrid(*[np.array(v, dtype=np.int64) for v in axes.values()], indexing='ij')
    return {k: g.ravel() for k, g in zip(axes, grid)}


def cdiv(a, b):
    return -(-a // b)


def clampi(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def same(got, want):
    return np.array_equal(got, np.broadcast_to(np.asarray(want).astype(np.int64), got.shape))


def align(b):
    return (b + 255) // 256 * 256


class Takes:
    """the launchers' bump allocator on arrays: take(b) is the offset of a piece of b bytes, .bytes the running total"""
    def __init__(self):
        self.bytes = 0

    def take(self, b, present=True):      # (present: `cond ? sc.take(b) : 0`)
        at = np.where(present, self.bytes, 0)
        self.bytes = self.bytes + np.where(present, align(b), 0)
        return at


def qp_of(Q):
    return np.where(Q <= 4, 4, np.where(Q <= 8, 8, 16))


def base_request(what, **over):
    """a valid request: every operand present, owned sample axes"""
    if what == 'rff':
        r = dict(esize=8, bwd=0, S=2, N=129, D=70, Q=3, J=5)
        r.update(ss_X=r['N'] * r['Q'], ss_Om=r['D'] * r['Q'], ss_ph=r['D'], ss_W=r['D'] * r['J'], has_X=1, has_Om=1, has_ph=1, has_W=1, has_out=1, has_G=1, has_dX=1)
    elif what == 'kmv':
        r = dict(esize=8, bwd=0, S=2, N=129, N2=65, Q=3, J=5, ard=1)
        r.update(ss_X=r['N'] * r['Q'], ss_X2=r['N2'] * r['Q'], ss_ls=r['Q'], ss_var=1, ss_da=1, ss_V=r['N2'] * r['J'], ss_A=r['N'] * r['J'], has_X=1, has_X2=1,
                 has_ls=1, has_var=1, has_da=0, has_V=1, has_out=1, has_A=1, has_w=1, has_dls=1, has_dvar=1)
    else:
        r = dict(call=0, esize=8, S=2, N=129, M=17, Q=3, ard=1, J=5)
        r.update(ss_mu=r['N'] * r['Q'], ss_s=r['N'] * r['Q'], ss_Z=r['M'] * r['Q'], ss_ls=r['Q'], ss_var=1, ss_A=r['J'] * r['M'] * r['M'],
                 has_mu=1, has_s=1, has_Z=1, has_ls=1, has_var=1, has_Psi1=1, has_Psi2=1, has_G1=1, has_G2=1, has_dmu=1, has_ds=1, has_dZ=1, has_dls=1,
                 has_dvar=1, has_A=1, has_R=1)
    r.update(over)
    return r


# ---- (a) the launch shapes the GPU cases were chosen for -----------------------------------------------------------------------------------
def test_launch_shapes_of_the_rff_cases(check):
    """which cases of tests/test_gpu_rff.py split d, into how many rows, with what tail"""
    for (N, D, S), want in (((70000, 3, 1), (64, 1)), ((70000, 130, 1), (128, 2)), ((131073, 65, 1), (128, 1)), ((129, 130, 1), (64, 3)),
                            ((129, 70, 2), (64, 2)), ((129, 5, 2), (64, 1)), ((1, 65, 1), (64, 2))):
        p = plans(check, 'rff', base_request('rff', S=S, N=N, D=D, ss_X=0, ss_Om=0, ss_ph=0, ss_W=0))
        assert (p['rc'][0], p['ch'][0], p['rows'][0], p['g1'][0]) == (0,) + want + want[1:], (N, D, S)


def test_launch_shapes_of_the_kmv_cases(check):
    """which cases of tests/test_gpu_kmv.py split n2, into how many rows"""
    for (N, N2, S), want in (((100, 5000, 1), (64, 79)), ((140000, 3, 1), (64, 1)), ((129, 63, 1), (64, 1)), ((129, 65, 1), (64, 2)),
                             ((300, 200, 1), (64, 4)), ((300, 300, 2), (64, 5)), ((1, 1, 1), (64, 1))):
        p = plans(check, 'kmv', base_request('kmv', S=S, N=N, N2=N2, ss_X=0, ss_X2=0, ss_ls=0, ss_var=0, ss_V=0, ss_A=0))
        assert (p['rc'][0], p['ch'][0], p['rows'][0], p['g1'][0]) == (0,) + want + want[1:], (N, N2, S)


def test_launch_shapes_of_the_large_psi_quad_cases(check):
    """the two large cases of tests/test_gpu_psi_quad.py: workgroups over m, strides over m and the tail; every other case with M > 1 splits m"""
    from test_gpu_psi_quad import CASES

    def mch(N, M, S):
        p = plans(check, 'psi', base_request('psi', call=2, S=S, N=N, M=M, ss_mu=0, ss_s=0, ss_Z=0, ss_ls=0, ss_var=0, ss_A=0))
        assert p['rc'][0] == 0 and p['gr_1'][0] == p['mch'][0] and p['split'][0] == (p['mch'][0] > 1)
        return p['mch'][0]
    assert mch(43700, 13, 1) == 6 and 13 // 6 == 2 and 13 % 6 == 1
    assert mch(262100, 2, 1) == 1
    assert all(mch(n, m, s) > 1 for n, m, q, a, j, s, own in CASES[:-2] if m > 1)


# ---- (b) the sweep against the parent's formulas --------------------------------------------------------------------------------------------
def parent_split(S, N, R, rb, unit, target):
    """rff_split / kmv_split as they stood in the launchers"""
    want = clampi(cdiv(target, cdiv(N, rb) * S), 1, clampi(cdiv(R, unit), 1, 65535))
    ch = cdiv(cdiv(R, want), unit) * unit
    return ch, cdiv(R, ch)


def check_split(p, R, unit):
    assert np.all(p['ch'] % unit == 0) and np.all(p['rows'] * p['ch'] >= R) and np.all(R > (p['rows'] - 1) * p['ch'])


def check_grid(p, names):
    for k in names:
        assert np.all(p[k] >= 1), k
    for k in names[1:]:
        assert np.all(p[k] <= 65535), k


def check_pieces(p, names, absent=None):
    """the pieces [at, next at) in the order of `names`: 256-aligned, ascending, so disjoint; the zeroed range inside the allocation"""
    assert np.all(p['bytes'] % 256 == 0)
    last = np.zeros_like(p['bytes'])
    for k in names:
        here = np.ones_like(last, dtype=bool) if absent is None or k not in absent else ~absent[k]
        assert np.all(p[k] % 256 == 0) and np.all((p[k] >= last)[here]) and np.all((p[k] <= p['bytes'])[here]), k
        last = np.where(here, p[k], last)


def test_rff_plan_is_the_parent_launcher(check):
    r = cross(esize=(4, 8), bwd=(0, 1), own=(0, 1, 2), S=SS, N=SIZES, D=SIZES, Q=QS, J=JS)      # own: 0 shared, 1 owned, 2 only X owned
    S, N, D, Q, J, bwd = (r[k] for k in 'S N D Q J bwd'.split())
    ox, orest = r['own'] > 0, r['own'] == 1
    req = dict(esize=r['esize'], bwd=bwd, S=S, N=N, D=D, Q=Q, J=J, ss_X=ox * N * Q, ss_Om=orest * D * Q, ss_ph=orest * D, ss_W=orest * D * J,
               has_X=1, has_Om=1, has_ph=1, has_W=1, has_out=1 - bwd, has_G=bwd, has_dX=bwd)
    p = plans(check, 'rff', req)
    assert np.all(p['rc'] == 0)
    # run() and rff_run<T, QP, JB>() of the parent
    es, bw = r['esize'], bwd == 1
    QP, JB = qp_of(Q), np.where(J <= 4, 4, 16)
    npass, own_X = cdiv(J, JB), req['ss_X'] != 0
    S_om, S_ph, S_W = (np.where(req[k] != 0, S, 1) for k in ('ss_Om', 'ss_ph', 'ss_W'))
    ch, dch = parent_split(S, N, D, 128, 64, 1024)
    n_out, n_dx = S * N * J, np.where(own_X, S, 1) * N * Q
    summed = np.where(bw, (dch > 1) | (~own_X & (S > 1)), dch > 1)
    scratch_sum = summed & ~(bw & (es == 8))
    sc = Takes()
    at_om, at_ph = sc.take(S_om * D * QP * es), sc.take(S_ph * D * es)
    at_wb = sc.take(S_W * npass * D * JB * es)
    n_acc = np.where(scratch_sum, np.where(bw, n_dx, n_out), 0)
    at_acc = sc.take(n_acc * 8)
    want = dict(qp=QP, jb=JB, npass=npass, ch=ch, rows=dch, g0=cdiv(N, 128), g1=dch, g2=S, own_X=own_X, summed=summed, scratch_sum=scratch_sum,
                n_prep=(S_om + S_ph + S_W * npass) * D, n_out=n_out, n_dx=n_dx, ss_om=np.where(req['ss_Om'] != 0, D * QP, 0),
                ss_ph=np.where(req['ss_ph'] != 0, D, 0), ss_wb=np.where(req['ss_W'] != 0, npass * D * JB, 0), at_om=at_om, at_ph=at_ph, at_wb=at_wb,
                at_acc=at_acc, zero_bytes=n_acc * 8, bytes=sc.bytes)
    assert set(want) == set(RFF_OUT) - {'rc'}
    for k, v in want.items():
        assert same(p[k], v), k
    check_split(p, D, 64)
    check_grid(p, ('g0', 'g1', 'g2'))
    check_pieces(p, ('at_om', 'at_ph', 'at_wb', 'at_acc'))
    assert np.all(p['at_acc'] + p['zero_bytes'] <= p['bytes'])
    assert not np.any(p['scratch_sum'][bw & (es == 8)]) and p['scratch_sum'].any() and p['summed'][bw & (es == 8)].any()


def test_kmv_plan_is_the_parent_launcher(check):
    r = cross(esize=(4, 8), bwd=(0, 1), own=(0, 1, 2), S=SS, N=SIZES, N2=SIZES, Q=QS, J=JS)      # own: 0 shared, 1 owned, 2 only the lengthscale owned
    S, N, N2, Q, J, bwd = (r[k] for k in 'S N N2 Q J bwd'.split())
    o, ol = r['own'] == 1, r['own'] > 0
    req = dict(esize=r['esize'], bwd=bwd, S=S, N=N, N2=N2, Q=Q, J=J, ard=1, ss_X=o * N * Q, ss_X2=o * N2 * Q, ss_ls=ol * Q, ss_var=o, ss_da=0, ss_V=o * N2 * J,
               ss_A=o * N * J, has_X=1, has_X2=1, has_ls=1, has_var=1, has_da=0, has_V=1, has_out=1 - bwd, has_A=bwd, has_w=bwd, has_dls=bwd, has_dvar=bwd)
    p = plans(check, 'kmv', req)
    assert np.all(p['rc'] == 0)
    # run() and kmv_run<T, QP, JB, KIND>() of the parent
    es, bw = r['esize'], bwd == 1
    QP, JB = qp_of(Q), np.where(J <= 4, 4, 16)
    npass = cdiv(J, JB)
    ss_Z = req['ss_X2']
    S_z, S_V = np.where((ss_Z != 0) | (req['ss_ls'] != 0), S, 1), np.where(req['ss_V'] != 0, S, 1)
    ch, rows = parent_split(S, N, N2, 128, 64, 1024)
    n_out = S * N * J
    n_zero = np.where(bw, S * (QP + 1), np.where(rows > 1, n_out, 0))
    sc = Takes()
    at_zs, at_vb = sc.take(S_z * N2 * QP * es), sc.take(S_V * npass * N2 * JB * es)
    at_zero = sc.take(n_zero * 8)
    gp = 64 // JB
    step = np.where(bw, gp, npass)                                  # for (pass0 = 0; pass0 < npass; pass0 += bwd ? gp : npass)
    np_of = lambda pass0: np.where(bw, clampi(npass - pass0, 1, gp), npass)
    last0 = (npass - 1) // step * step
    want = dict(qp=QP, jb=JB, npass=npass, square=0 * S, N2=N2, ss_Z=ss_Z, S_z=S_z, S_V=S_V, ch=ch, rows=rows, g0=cdiv(N, 128), g1=rows, g2=S, gp=step,
                n_prep_z=S_z * N2, n_out=n_out, ss_zs=np.where(S_z > 1, N2 * QP, 0), ss_vb=np.where(S_V > 1, npass * N2 * JB, 0), n_zero=n_zero, at_zs=at_zs,
                at_vb=at_vb, at_zero=at_zero, at_dv=at_zero + S * QP * 8, bytes=sc.bytes, np0=np_of(0), items0=S_V * np_of(0) * N2, np_last=np_of(last0),
                items_last=S_V * np_of(last0) * N2)
    assert set(want) == set(KMV_OUT) - {'rc'}
    for k, v in want.items():
        assert same(p[k], v), k
    check_split(p, N2, 64)
    check_grid(p, ('g0', 'g1', 'g2'))
    check_pieces(p, ('at_zs', 'at_vb', 'at_zero'))
    assert np.all(p['at_zero'] + p['n_zero'] * 8 <= p['bytes']) and np.all((p['at_dv'] + S * 8 <= p['bytes'])[bw])
    # a square product: X in both roles, N2 = N whatever the request says
    sq = plans(check, 'kmv', dict(req, has_X2=0, has_da=1, ss_da=o, N2=N2 * 0 + 7, ss_V=o * N * J))
    ch, rows = parent_split(S, N, N, 128, 64, 1024)
    assert np.all(sq['rc'] == 0) and np.all(sq['square'] == 1) and np.array_equal(sq['N2'], N) and np.array_equal(sq['ss_Z'], req['ss_X'])
    assert np.array_equal(sq['ch'], ch) and np.array_equal(sq['rows'], rows)


def test_psi_plans_are_the_parent_launchers(check):
    r = cross(call=(0, 1, 2), esize=(4, 8), own=(0, 1, 2), opt=(0, 1, 2, 3), S=SS, N=SIZES, M=SIZES, Q=QS, J=(1, 4, 5, 70))      # own 2: only Z owned
    r = {k: v[np.where(r['call'] == 2, r['opt'] == 0, r['J'] == 1)] for k, v in r.items()}      # J enters the contraction only, the options the others
    call, S, N, M, Q, J, opt = (r[k] for k in 'call S N M Q J opt'.split())
    o, oz = r['own'] == 1, r['own'] > 0
    # opt: which optional outputs are present.  forward: Psi1 / Psi2; reverse: 0 all, 1 G1 only, 2 G2 with dmu ds (rows pass alone), 3 G2 with dZ dvar (pairs pass alone)
    has = dict(has_Psi1=opt != 2, has_Psi2=opt != 1, has_G1=opt <= 1, has_G2=opt != 1, has_dmu=opt <= 2, has_ds=opt <= 2, has_dZ=(opt == 0) | (opt == 3),
               has_dls=opt <= 1, has_dvar=(opt == 0) | (opt == 3))
    req = dict(call=call, esize=r['esize'], S=S, N=N, M=M, Q=Q, ard=1, ss_mu=o * N * Q, ss_s=o * N * Q, ss_Z=oz * M * Q, ss_ls=o * Q, ss_var=o, has_mu=1, has_s=1,
               has_Z=1, has_ls=1, has_var=1, J=J, ss_A=o * J * M * M, has_A=1, has_R=1, **has)
    p = plans(check, 'psi', req)
    assert np.all(p['rc'] == 0)
    es, QP = r['esize'], qp_of(Q)
    fwd, bwd, quad = call == 0, call == 1, call == 2
    SM = S * M
    # the two stride rules, as psi_fwd / psi_bwd / psi_quad wrote them out
    nt = cdiv(M, 16)
    pairs = nt * (nt + 1) // 2
    rch = clampi(cdiv(2048, pairs * S), 1, clampi(cdiv(N, 64), 1, 65535))
    bx = cdiv(N, 128)
    mch = clampi(cdiv(2048, bx * S), 1, clampi(M, 1, 65535))
    own = {k: req['ss_' + k] != 0 for k in ('mu', 's', 'Z', 'ls', 'var')}
    n_mu, n_s, n_Z = np.where(own['mu'], S, 1) * N * Q, np.where(own['s'], S, 1) * N * Q, np.where(own['Z'], S, 1) * M * Q
    h = {k: np.asarray(v, dtype=bool) for k, v in has.items()}
    pairs_pass = h['has_G2'] & (h['has_dZ'] | h['has_dls'] | h['has_dvar'])
    rows_pass = h['has_G2'] & (h['has_dmu'] | h['has_ds'] | h['has_dls'])
    wide = es == 4
    total = S * N * J
    sc = Takes()
    at_z, at_zh = sc.take(SM * QP * es), sc.take(SM * QP * es)
    need_rows = np.where(fwd, h['has_Psi2'], bwd & pairs_pass)
    at_rows = sc.take(S * N * (2 * QP + 2) * es, need_rows)
    at_acc_f = sc.take(SM * M * 8, fwd & h['has_Psi2'])                          # psi_fwd: acc2
    at_wt = sc.take(np.where(quad, SM * M * 4 * es, SM * M * es), quad | (bwd & rows_pass))      # psi_bwd: Wt; psi_quad: Wq
    at_zero_b = sc.bytes
    at_l2, at_dv = sc.take(S * QP * 8, bwd), sc.take(S * 8, bwd)
    at_big = sc.take(np.where(wide, (n_mu + n_s + n_Z) * 8, 0), bwd)
    at_acc_q = sc.take(np.where(mch > 1, total * 8, 0), quad)
    z = 0 * S
    want = dict(qp=QP, n_prep=S * (N + M), n_mm=SM * M, g1_0=np.where(quad, 1, cdiv(N, 256)), g1_1=np.where(quad, 1, cdiv(M, 32)), g1_2=np.where(quad, 1, S),
                rch=np.where(need_rows, rch, 1), gp_0=np.where(need_rows, pairs, 1), gp_1=np.where(need_rows, rch, 1), gp_2=np.where(need_rows, S, 1),
                pairs_pass=bwd & pairs_pass, rows_pass=bwd & rows_pass, wide=bwd & wide, fold=bwd & wide & (h['has_dmu'] | h['has_ds'] | h['has_dZ']),
                close=bwd & (h['has_dls'] | h['has_dvar']), n_mu=np.where(bwd, n_mu, 0), n_s=np.where(bwd, n_s, 0), n_Z=np.where(bwd, n_Z, 0),
                npass=np.where(quad, cdiv(J, 4), 0), n_out=np.where(quad, total, 0), split=quad & (mch > 1), at_z=at_z, at_zh=at_zh, at_rows=at_rows,
                at_acc=np.where(fwd, at_acc_f, np.where(quad, at_acc_q, 0)), at_wt=at_wt, at_l2=at_l2, at_dv=at_dv, at_big=at_big,
                at_zero=np.where(bwd, at_zero_b, np.where(fwd, at_acc_f, at_acc_q)),
                zero_bytes=np.where(bwd, sc.bytes - at_zero_b, np.where(fwd, np.where(h['has_Psi2'], SM * M * 8, 0), np.where(mch > 1, total * 8, 0))),
                bytes=sc.bytes)
    uses_rows = quad | (bwd & rows_pass)
    want.update(mch=np.where(uses_rows, mch, 1), gr_0=np.where(uses_rows, bx, 1), gr_1=np.where(uses_rows, mch, 1), gr_2=np.where(uses_rows, S, 1))
    want.update({'own_' + a: np.where(bwd, own[b], z) for a, b in (('mu', 'mu'), ('s', 's'), ('Z', 'Z'), ('l', 'ls'), ('v', 'var'))})
    assert set(want) == set(PSI_OUT) - {'rc'}
    for k, v in want.items():
        assert same(p[k], v), k
    check_grid(p, ('g1_0', 'g1_1', 'g1_2'))
    check_grid(p, ('gp_0', 'gp_1', 'gp_2'))
    check_grid(p, ('gr_0', 'gr_1', 'gr_2'))
    # (the contraction's at_acc lies behind its at_wt: out of this order, checked on its own below)
    absent = dict(at_rows=~need_rows, at_acc=~(fwd & h['has_Psi2']), at_wt=~uses_rows, at_l2=~bwd, at_dv=~bwd, at_big=~bwd)
    check_pieces(p, ('at_z', 'at_zh', 'at_rows', 'at_acc', 'at_wt', 'at_l2', 'at_dv', 'at_big'), absent)
    assert np.all((p['at_acc'] >= p['at_wt'])[quad]) and np.all(p['at_zero'] + p['zero_bytes'] <= p['bytes']) and np.all(p['at_zero'] % 256 == 0)
    for k in ('pairs_pass', 'rows_pass', 'fold', 'close', 'split'):
        assert p[k].any(), k


# ---- (c) refusals, each one its own request ---------------------------------------------------------------------------------------------------
STRIDE_TEXT = {
    'rff': 'a sample stride must be 0 or the elements of one sample (X: N Q; Omega: D Q; phase: D; W: D J)',
    'kmv': 'a sample stride must be 0 or the elements of one sample (X: N Q; X2: N2 Q; lengthscale: Q or 1; variance, diag_add: 1; V: N2 J; A: N J)',
    'psi': 'a sample stride must be 0 or the elements of one sample (mu, s: N Q; Z: M Q; lengthscale: Q or 1; variance: 1)'}
SIZES_TEXT = {'rff': '1 <= S <= 65535 samples, N, D, Q, J >= 1', 'kmv': '1 <= S <= 65535 samples, N, N2, Q, J >= 1', 'psi': '1 <= S <= 65535 samples, N, M, Q >= 1'}
REFUSALS = [(w, dict(Q=17), -3, 'Q = 17 above the limit of 16 input dimensions') for w in ('rff', 'kmv', 'psi')]
REFUSALS += [(w, over, -2, SIZES_TEXT[w]) for w in ('rff', 'kmv', 'psi') for over in (dict(S=0), dict(S=65536), dict(N=0))]
REFUSALS += [(w, over, -2, SIZES_TEXT[w]) for w, over in (('rff', dict(D=0)), ('rff', dict(J=0)), ('kmv', dict(N2=0)), ('kmv', dict(J=0)), ('psi', dict(M=0)),
                                                          ('rff', dict(Q=0)), ('kmv', dict(Q=0)), ('psi', dict(Q=0)), ('kmv', dict(has_X2=0, N=0)))]
REFUSALS += [('rff', dict(D=(1 << 24) + 1, ss_Om=0, ss_ph=0, ss_W=0), -2, 'N <= 2^31, D <= 2^24, J <= 2^16'),
             ('rff', dict(J=(1 << 16) + 1, ss_W=0), -2, 'N <= 2^31, D <= 2^24, J <= 2^16'),
             ('rff', dict(N=(1 << 31) + 1, ss_X=0), -2, 'N <= 2^31, D <= 2^24, J <= 2^16'),
             ('kmv', dict(J=(1 << 16) + 1, ss_V=0, ss_A=0), -2, 'N, N2 <= 2^31, J <= 2^16'),
             ('kmv', dict(N2=(1 << 31) + 1, ss_X2=0, ss_V=0), -2, 'N, N2 <= 2^31, J <= 2^16'),
             ('psi', dict(M=(1 << 20) + 1, ss_Z=0), -2, 'M <= 2^20, N <= 2^31'),
             ('psi', dict(N=(1 << 31) + 1, ss_mu=0, ss_s=0), -2, 'M <= 2^20, N <= 2^31')]
REFUSALS += [(w, {k: 5}, -2, STRIDE_TEXT[w]) for w, ks in (('rff', 'ss_X ss_Om ss_ph ss_W'), ('kmv', 'ss_X ss_X2 ss_ls ss_var ss_V'), ('psi', 'ss_mu ss_s ss_Z ss_ls ss_var'))
             for k in ks.split()]
REFUSALS += [('kmv', dict(bwd=1, ss_A=5), -2, STRIDE_TEXT['kmv']), ('kmv', dict(has_X2=0, has_da=1, ss_da=2, N2=129, ss_V=129 * 5), -2, STRIDE_TEXT['kmv']),
             ('psi', dict(call=2, ss_A=7), -2, 'the sample stride of A must be 0 or J M M')]
REFUSALS += [('rff', {k: 0}, -2, 'null X, Omega, phase or W') for k in ('has_X', 'has_Om', 'has_ph', 'has_W')]
REFUSALS += [('rff', dict(has_out=0), -2, 'null out'), ('rff', dict(bwd=1, has_G=0), -2, 'null G or dX_acc'), ('rff', dict(bwd=1, has_dX=0), -2, 'null G or dX_acc')]
REFUSALS += [('kmv', {k: 0}, -2, 'null X, lengthscale, variance or V') for k in ('has_X', 'has_ls', 'has_var', 'has_V')]
REFUSALS += [('kmv', dict(has_out=0), -2, 'null out'), ('kmv', dict(bwd=1, has_A=0), -2, 'null A or w'), ('kmv', dict(bwd=1, has_w=0), -2, 'null A or w'),
             ('kmv', dict(bwd=1, has_dls=0, has_dvar=0), -2, 'null dls_acc and dvar_acc')]
REFUSALS += [('psi', {k: 0}, -2, 'null mu, s, Z, lengthscale or variance') for k in ('has_mu', 'has_s', 'has_Z', 'has_ls', 'has_var')]
REFUSALS += [('psi', dict(call=2, **over), -2, 'J >= 1 weight matrices, A and R not null') for over in (dict(J=0), dict(has_A=0), dict(has_R=0))]
# where two checks fire, the earlier one of the parent's run() wins
REFUSALS += [('rff', dict(Q=17, S=0), -2, SIZES_TEXT['rff']), ('kmv', dict(Q=17, has_X=0), -3, 'Q = 17 above the limit of 16 input dimensions'),
             ('psi', dict(has_mu=0, ss_Z=5), -2, 'null mu, s, Z, lengthscale or variance'), ('kmv', dict(has_out=0, ss_X=5), -2, 'null out')]


@pytest.mark.parametrize('what,over,rc,why', REFUSALS, ids=['%s-%s' % (w, '-'.join('%s=%s' % kv for kv in o.items())) for w, o, _, _ in REFUSALS])
def test_refusals(check, what, over, rc, why):
    """the codes tests/test_gpu_{rff,kmv,psi,psi_quad}.py expect of the entry points (Q above the limit: -3; everything else: -2) and the
    message texts of the launchers' checks before they moved into the plans"""
    assert refusal(check, what, **base_request(what)) == (0, '')
    assert refusal(check, what, **base_request(what, **over)) == (rc, why)


def test_partial_requests_are_accepted(check):
    """one of the two kmv gradients, any subset of the psi outputs: not refusals"""
    assert refusal(check, 'kmv', **base_request('kmv', bwd=1, has_dls=0))[0] == 0 and refusal(check, 'kmv', **base_request('kmv', bwd=1, has_dvar=0))[0] == 0
    for call in (0, 1):
        none = {k: 0 for k in PSI_IN if k.startswith('has_') and k[4:] in ('Psi1', 'Psi2', 'G1', 'G2', 'dmu', 'ds', 'dZ', 'dls', 'dvar', 'A', 'R')}
        assert refusal(check, 'psi', **base_request('psi', call=call, **none))[0] == 0


# ---- (d) the per-sample grid --------------------------------------------------------------------------------------------------------------
def test_per_sample_plan(check):
    """uni_ps_plan, lik_plan and rm_plan as they stood: up to 512 chunks of 256 rows, at most 8192 workgroups' worth per S, a grid of at most 65 536"""
    r = cross(n=(1, 256, 257, 131072, 10 ** 7), S=(1, 16, 17, 8192, 8193, 70000))
    got = np.array(check('\n'.join('ps %d %d' % (s, n) for s, n in zip(r['S'], r['n']))).split(), dtype=np.int64).reshape(-1, 2)
    c = np.maximum(np.minimum(np.minimum((r['n'] + 255) // 256, 512), 8192 // r['S']), 1)
    assert np.array_equal(got[:, 0], c) and np.array_equal(got[:, 1], np.minimum(r['S'] * c, 65536))
    assert np.all(got >= 1) and np.all(got[:, 0] * 256 >= np.minimum(r['n'], 256))


def test_reduce_split_is_both_parent_formulas(check):
    r = cross(S=SS, N=SIZES, R=SIZES)
    got = np.array(check('\n'.join('split %d %d %d 128 64 1024' % t for t in zip(r['S'], r['N'], r['R']))).split(), dtype=np.int64).reshape(-1, 2)
    ch, rows = parent_split(r['S'], r['N'], r['R'], 128, 64, 1024)
    assert np.array_equal(got[:, 0], ch) and np.array_equal(got[:, 1], rows)
