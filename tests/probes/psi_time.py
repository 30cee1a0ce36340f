"""Times of the RBF psi statistics (HIP events, median of 5 windows after a warm-up, each window long enough to pass 0.2 s; random operands):
  (a) mxf_psi_rbf_fwd (Psi1 and Psi2) and mxf_psi_rbf_bwd (both cotangents, all five gradients) at N = 65 536, Q = 8, M = 1 024, both dtypes,
      with the rate in psi2n terms per second (N M (M + 1) / 2 terms a pass; the reverse mode makes two passes);
  (b) the same at N = 4 096, Q = 8, M = 128, where the torch expression over the (N, M, M, Q) intermediate of tests/_psi_ref.py still fits on
      the device, against that expression and autograd through it, with the largest difference between the two results;
  (c) one bound-plus-gradient evaluation of BayesianGPLVM at N = 65 536, Q = 8, M = 1 024, P = 1, both dtypes.
usage: psi_time.py"""
import os
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from mxfusion_amd import ops  # noqa: E402
import _psi_ref as R  # noqa: E402


def timed(fn, min_window=0.2):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps, out = 2, []
    while len(out) < 5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms < 1e3 * min_window and reps < 1 << 16:
            reps *= 2
            continue
        out.append(ms / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def operands(N, M, Q, dt, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=dt, generator=g)
    mu = r(1, N, Q) * 6 - 3
    return dict(mu=mu, s=r(1, N, Q) * 1.5, Z=mu[:, :M].clone() + 0.1 * (r(1, M, Q) - 0.5), ls=r(1, Q) + 1.5, var=r(1, 1) + 0.5,
                G1=r(1, M, N) - 0.5, G2=r(1, M, M) - 0.5)


def kernels(N, M, Q, dt):
    p = operands(N, M, Q, dt)
    args = [p[k] for k in ('mu', 's', 'Z', 'ls', 'var')] + [True]
    acc = [torch.zeros_like(t) for t in args[:5]]
    fwd = timed(lambda: ops.psi_rbf(*args))
    bwd = timed(lambda: ops.psi_rbf_bwd_(*args, p['G1'], p['G2'], *acc))
    terms = N * M * (M + 1) / 2
    print('N=%d Q=%d M=%d %s: forward %.3f ms [%.3f, %.3f] (%.3g terms/s)   reverse %.3f ms [%.3f, %.3f] (%.3g terms/s)'
          % (N, Q, M, str(dt)[6:], *fwd, terms / fwd[0] * 1e3, *bwd, 2 * terms / bwd[0] * 1e3), flush=True)
    return p, args


def against_torch(N, M, Q, dt):
    p, args = kernels(N, M, Q, dt)
    lv = [p[k][0].clone().requires_grad_(True) for k in ('mu', 's', 'Z', 'ls', 'var')]
    expr = lambda: (R.psi1(*lv), R.psi2(*lv))
    with torch.no_grad():
        tf = timed(expr)

    def both():
        P1, P2 = expr()
        return torch.autograd.grad((p['G1'][0] * P1).sum() + (p['G2'][0] * P2).sum(), lv)
    tb = timed(both)
    P1, P2 = ops.psi_rbf(*args)
    acc = [torch.zeros_like(t) for t in args[:5]]
    ops.psi_rbf_bwd_(*args, p['G1'], p['G2'], *acc)
    with torch.no_grad():
        R1, R2 = expr()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print('   torch expression: forward %.3f ms [%.3f, %.3f]   forward + autograd %.3f ms [%.3f, %.3f]   largest difference / largest entry: Psi1 %.1e '
          'Psi2 %.1e gradients %s' % (*tf, *tb, rel(P1[0], R1), rel(P2[0], R2), ' '.join('%.1e' % rel(a[0], b) for a, b in zip(acc, both()))), flush=True)


def module_step(dtype):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import BayesianGPLVM
    from mxfusion_amd.util.inference import VariablesDict
    N, Q, M, P = 65536, 8, 1024, 1
    dt = torch.float64 if dtype == 'float64' else torch.float32
    mdl = Model()
    mdl.Z = Variable(shape=(M, Q))
    mdl.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.5)
    mdl.Y = BayesianGPLVM.define_variable(kernel=RBF(Q, ARD=True, dtype=dtype), noise_var=mdl.noise_var, shape=(N, P), inducing_inputs=mdl.Z, dtype=dtype)
    gp = mdl.Y.factor
    graph, kp = gp._module_graph, gp.kernel.parameters
    p = operands(N, M, Q, dt, seed=1)
    leaves = {graph.X.uuid: p['mu'], graph.X_var.uuid: p['s'] + 0.01, mdl.Z.uuid: p['Z'], mdl.noise_var.uuid: torch.full((1, 1), 0.5, device='cuda', dtype=dt),
              kp['rbf_lengthscale'].uuid: p['ls'], kp['rbf_variance'].uuid: p['var']}
    for t in leaves.values():
        t.requires_grad_(True)
    vs = VariablesDict(dict(leaves))
    vs[mdl.Y.uuid] = torch.sin(p['mu'].detach().sum(-1, keepdim=True))
    alg = gp.gplvm_log_pdf
    alg.jitter = 1e-6

    def step():
        torch.autograd.grad(alg.compute(None, vs).sum(), list(leaves.values()))
    c = timed(step, min_window=0.5)
    print('(c) BayesianGPLVM bound + gradients, N=%d Q=%d M=%d P=%d %s: %.2f ms [%.2f, %.2f]  info %d'
          % (N, Q, M, P, dtype, *c, int(alg._last_info.abs().sum())), flush=True)


def main():
    print(torch.cuda.get_device_name(0))
    for dt in (torch.float32, torch.float64):
        print('(a)', end=' ')
        kernels(65536, 1024, 8, dt)
    for dt in (torch.float32, torch.float64):
        print('(b)', end=' ')
        against_torch(4096, 128, 8, dt)
    for dtype in ('float32', 'float64'):
        module_step(dtype)


if __name__ == '__main__':
    main()
