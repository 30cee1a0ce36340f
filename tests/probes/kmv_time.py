"""Times of the matrix-free kernel product (HIP events, median of 5 windows after a warm-up, each window long enough to pass 0.2 s; random
operands):
  (a) mxf_kmv and mxf_kmv_bwd at N = N2 = 65 536, Q = 8, J in {1, 16, 64}, RBF with ARD, both dtypes, with the rate in pairs per second
      (N N2 a pass; J = 64 takes four passes) and the peak device memory of a call, beside ops.gram + torch.matmul at the same size (the
      N x N matrix is 17 GB in float32 and 34 GB in float64) with the largest difference between the two results;
  (b) one log_pdf + gradient evaluation of IterativeGPRegression (10 probes, rank 15, cg_tol 1e-8: the defaults) at N = 65 536, Q = 8, both
      dtypes, and at N = 8 192 in float64 beside one of GPRegression on the same data, with the CG iterations taken.
usage: kmv_time.py [a|b]"""
import os
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mxfusion_amd import ops  # noqa: E402


def timed(fn, min_window=0.2):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps, out = 1, []
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


def peak(fn):
    """peak device memory of one call above what is allocated before it, in MiB"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def kernels(N, Q, J, dt):
    g = torch.Generator(device='cuda').manual_seed(J)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=dt, generator=g)
    X, ls, var, noise = r(1, N, Q) * 4 - 2, r(1, Q) + 1.0, r(1, 1) + 0.5, r(1, 1) * 0.1 + 0.05
    V, A = torch.randn(1, N, J, device='cuda', dtype=dt, generator=g), torch.randn(1, N, J, device='cuda', dtype=dt, generator=g)
    dls, dvar = torch.zeros_like(ls), torch.zeros_like(var)
    fwd = lambda: ops.kernel_matvec('rbf', X, None, ls, var, True, V, noise)
    bwd = lambda: ops.kernel_matvec_bwd_('rbf', X, None, ls, var, True, A, V, None, dls, dvar)
    dense = lambda: torch.matmul(ops.gram('rbf', X, None, ls, var, True, diag_add=noise), V)
    passes = -(-J // (4 if J <= 4 else 16))
    tf, tb, td = timed(fwd), timed(bwd), timed(dense)
    mf, mb, md = peak(fwd), peak(bwd), peak(dense)
    a, b = fwd(), dense()
    print('N=N2=%d Q=%d J=%d %s' % (N, Q, J, str(dt)[6:]))
    print('   fused: forward %.3f ms [%.3f, %.3f] (%.3g pairs/s, peak %.0f MiB)   reverse %.3f ms [%.3f, %.3f] (%.3g pairs/s, peak %.0f MiB)'
          % (*tf, passes * N * N / tf[0] * 1e3, mf, *tb, passes * N * N / tb[0] * 1e3, mb))
    print('   gram + matmul: %.3f ms [%.3f, %.3f] (peak %.0f MiB)   largest difference / largest entry %.1e'
          % (*td, md, float((a - b).abs().max() / b.abs().max())), flush=True)


def module_call(N, dt, beside=False):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import GPRegression, IterativeGPRegression
    from mxfusion_amd.util.inference import VariablesDict
    Q, P = 8, 1
    dts = str(dt)[6:]
    g = torch.Generator(device='cuda').manual_seed(0)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=dt, generator=g)
    X = r(1, N, Q) * 4 - 2
    Y = torch.sin(X.sum(-1, keepdim=True)) + 0.3 * torch.randn(1, N, P, device='cuda', dtype=dt, generator=g)
    for cls, alg in ((IterativeGPRegression, 'iterative_gp_log_pdf'),) + (((GPRegression, 'gp_log_pdf'),) if beside else ()):
        mdl = Model()
        mdl.X = Variable(shape=(N, Q))
        mdl.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
        mdl.Y = cls.define_variable(X=mdl.X, kernel=RBF(Q, ARD=True, dtype=dts), noise_var=mdl.noise_var, shape=(N, P), dtype=dts)
        gp = mdl.Y.factor
        kp = gp.kernel.parameters
        leaves = [torch.full((1, 1), 0.1, device='cuda', dtype=dt).requires_grad_(True), torch.full((1, Q), 1.5, device='cuda', dtype=dt).requires_grad_(True),
                  torch.ones(1, 1, device='cuda', dtype=dt).requires_grad_(True)]
        vs = VariablesDict({gp._module_graph.X.uuid: X, mdl.Y.uuid: Y, mdl.noise_var.uuid: leaves[0], kp['rbf_lengthscale'].uuid: leaves[1],
                            kp['rbf_variance'].uuid: leaves[2]})
        a = getattr(gp, alg)

        def call():
            return torch.autograd.grad(a.compute(None, vs).sum(), leaves)
        t = timed(call, min_window=0.0 if cls is IterativeGPRegression and N > 10000 else 0.2)
        mem = peak(call)
        extra = '' if cls is GPRegression else ', %d CG iterations, rank %d' % (int(a.cfg.last.iterations.max()), a.cfg.last.rank)
        print('(b) %s N=%d Q=%d %s log_pdf + gradient: %.1f ms [%.1f, %.1f], peak %.0f MiB%s' % (cls.__name__, N, Q, dts, *t, mem, extra), flush=True)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else 'ab'
    print(torch.cuda.get_device_name(0))
    if 'a' in what:
        for dt in (torch.float32, torch.float64):
            for J in (1, 16, 64):
                kernels(65536, 8, J, dt)
    if 'b' in what:
        module_call(8192, torch.float64, beside=True)
        module_call(65536, torch.float32)
        module_call(65536, torch.float64)


if __name__ == '__main__':
    main()
