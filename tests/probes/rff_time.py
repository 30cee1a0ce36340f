"""Times of the random Fourier feature kernels (HIP events, median of 5 windows after a warm-up, each window long enough to pass 0.2 s;
random operands):
  (a) mxf_rff_eval and mxf_rff_eval_bwd at N = 262 144, Q = 8, D = 4 096, J in {1, 16, 64}, both dtypes, with the rate in cosines per second
      (N D a pass; J = 64 takes four passes) and the peak device memory of a call, against the torch expression cos(X Omega^T + b) W and
      autograd through it on the same device, with the largest difference between the two results;
  (b) one SVGPRegressionPathwiseSampling call at Nt = 1e6, M = 1 024, Q = 8, 16 samples of 1 024 features, float32.
usage: rff_time.py"""
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


def kernels(N, Q, D, J, dt):
    g = torch.Generator(device='cuda').manual_seed(J)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=dt, generator=g)
    X, Om, ph = r(1, N, Q) * 4 - 2, torch.randn(1, D, Q, device='cuda', dtype=dt, generator=g), r(1, D) * 2 * np.pi
    W, G = torch.randn(1, D, J, device='cuda', dtype=dt, generator=g), torch.randn(1, N, J, device='cuda', dtype=dt, generator=g)
    dX = torch.zeros_like(X)
    fwd, bwd = lambda: ops.rff_eval(X, Om, ph, W), lambda: ops.rff_eval_bwd_(X, Om, ph, W, G, dX)
    Xl = X[0].clone().requires_grad_(True)
    expr = lambda: torch.cos(Xl @ Om[0].T + ph[0]) @ W[0]

    def expr_fwd():
        with torch.no_grad():
            return expr()

    def expr_both():
        return torch.autograd.grad((expr() * G[0]).sum(), Xl)[0]
    passes = -(-J // (4 if J <= 4 else 16))
    tf, tb, ef, eb = timed(fwd), timed(bwd), timed(expr_fwd), timed(expr_both)
    mf, mb, mef, meb = peak(fwd), peak(bwd), peak(expr_fwd), peak(expr_both)
    dX.zero_()
    bwd()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print('N=%d Q=%d D=%d J=%d %s' % (N, Q, D, J, str(dt)[6:]))
    print('   fused: forward %.3f ms [%.3f, %.3f] (%.3g cosines/s, peak %.0f MiB)   reverse %.3f ms [%.3f, %.3f] (%.3g sines/s, peak %.0f MiB)'
          % (*tf, passes * N * D / tf[0] * 1e3, mf, *tb, passes * N * D / tb[0] * 1e3, mb))
    print('   torch: forward %.3f ms [%.3f, %.3f] (peak %.0f MiB)   forward + autograd %.3f ms [%.3f, %.3f] (peak %.0f MiB)   largest difference / '
          'largest entry: forward %.1e gradient %.1e' % (*ef, mef, *eb, meb, rel(fwd()[0], expr_fwd()), rel(dX[0], expr_both())), flush=True)


def module_call():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.components.variables import PositiveTransformation
    from mxfusion_amd.modules.gp_modules import SVGPRegression, SVGPRegressionPathwiseSampling
    from mxfusion_amd.util.inference import VariablesDict
    Nt, M, Q, P, S, D = 1000000, 1024, 8, 1, 16, 1024
    dt = torch.float32
    g = torch.Generator(device='cuda').manual_seed(0)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=dt, generator=g)
    mdl = Model()
    mdl.X = Variable(shape=(Nt, Q))
    mdl.Z = Variable(shape=(M, Q))
    mdl.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    mdl.Y = SVGPRegression.define_variable(X=mdl.X, kernel=RBF(Q, ARD=True, dtype='float32'), noise_var=mdl.noise_var, inducing_inputs=mdl.Z, shape=(Nt, P),
                                           dtype='float32')
    gp = mdl.Y.factor
    graph, post, kp = gp._module_graph, gp._extra_graphs[0], gp.kernel.parameters
    vs = VariablesDict({graph.X.uuid: r(1, Nt, Q) * 6 - 3, mdl.Z.uuid: r(1, M, Q) * 6 - 3, mdl.noise_var.uuid: torch.full((1, 1), 0.1, device='cuda', dtype=dt),
                        kp['rbf_lengthscale'].uuid: r(1, Q) + 1.5, kp['rbf_variance'].uuid: r(1, 1) + 0.5, post.qU_mean.uuid: r(1, M, P) - 0.5,
                        post.qU_cov_W.uuid: 0.01 * (r(1, M, M) - 0.5), post.qU_cov_diag.uuid: r(1, M) * 0.1 + 0.05})
    alg = SVGPRegressionPathwiseSampling(graph, post, [graph.X], num_features=D, jitter=1e-4)
    alg.num_samples = S
    call = lambda: alg.compute(None, vs)
    with torch.no_grad():
        t = timed(call, min_window=0.5)
        mem = peak(call)
        out = call()[mdl.Y.uuid]
    print('(b) SVGPRegressionPathwiseSampling Nt=%d M=%d Q=%d %d samples of %d features float32: %.1f ms [%.1f, %.1f], peak %.0f MiB, output %s finite %s'
          % (Nt, M, Q, S, D, *t, mem, tuple(out.shape), bool(torch.isfinite(out).all())), flush=True)


def main():
    print(torch.cuda.get_device_name(0))
    for dt in (torch.float32, torch.float64):
        for J in (1, 16, 64):
            kernels(262144, 8, 4096, J, dt)
    module_call()


if __name__ == '__main__':
    main()
