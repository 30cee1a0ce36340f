"""Times of the nearest-neighbour (Vecchia) GP kernels (HIP events, median of 5 windows after a warm-up, each window long enough to pass
0.2 s) at N = 65 536, Q = 8, P = 1, k in {8, 32}, both dtypes; X uniform on (-2, 2)^Q, Y = sin(sum x) + 0.1 normal:
  (a) mxf_knn, causal, with the rate in (row, candidate) pairs per second (N (N - 1) / 2 pairs);
  (b) mxf_vecchia_logpdf and mxf_vecchia_logpdf_bwd on those neighbour sets, with the rate in rows per second;
  (c) one MAP step of VecchiaGPRegression (value, reverse mode, Adam; the neighbour sets cached), wall clock over 20 steps;
  (d) for orientation only, one MAP step of IterativeGPRegression at the same N (10 probes, rank-15 preconditioner, cg_tol 1e-8) -- an exact
      method with a stochastic value, not a like-for-like comparison.
usage: vecchia_time.py [abcd]"""
import os
import sys
import time

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mxfusion_amd import Model, Variable, ops  # noqa: E402
from mxfusion_amd.components.variables import PositiveTransformation  # noqa: E402
from mxfusion_amd.components.distributions.gp.kernels import RBF  # noqa: E402
from mxfusion_amd.inference import GradBasedInference, MAP  # noqa: E402
from mxfusion_amd.modules.gp_modules import IterativeGPRegression, VecchiaGPRegression  # noqa: E402

N, Q = 65536, 8


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


def data(dt):
    g = torch.Generator(device='cuda').manual_seed(1)
    X = torch.rand(N, Q, device='cuda', dtype=dt, generator=g) * 4 - 2
    Y = torch.sin(X.sum(1, keepdim=True)) + 0.1 * torch.randn(N, 1, device='cuda', dtype=dt, generator=g)
    return X.contiguous(), Y.contiguous()


def kernels(dt, k, what):
    X, Y = data(dt)
    one = lambda v, n=1: torch.full((n,), v, device='cuda', dtype=dt)
    ls, var, noise, g = one(1.0, Q), one(1.2), one(0.05), one(1.0)
    nbr, _ = ops.knn(X, None, k, causal=True, want_d2=False)
    print('N=%d Q=%d k=%d %s' % (N, Q, k, str(dt)[6:]))
    if 'a' in what:
        t = timed(lambda: ops.knn(X, None, k, causal=True, want_d2=False))
        print('   knn, causal: %.3f ms [%.3f, %.3f] (%.3g pairs/s)' % (*t, 0.5 * N * (N - 1) / t[0] * 1e3), flush=True)
    if 'b' in what:
        tf = timed(lambda: ops.vecchia_logpdf('rbf', X, Y, nbr, ls, var, noise, True, want_terms=False))
        tb = timed(lambda: ops.vecchia_logpdf_bwd('rbf', X, Y, nbr, ls, var, noise, True, g))
        print('   logpdf: %.3f ms [%.3f, %.3f] (%.3g rows/s)   bwd: %.3f ms [%.3f, %.3f] (%.3g rows/s)'
              % (*tf, N / tf[0] * 1e3, *tb, N / tb[0] * 1e3), flush=True)


def map_step(cls, dt, steps, **kw):
    X, Y = data(dt)
    dts = str(dt)[6:]
    m = Model()
    m.X = Variable(shape=(N, Q))
    m.noise_var = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=0.1)
    m.Y = cls.define_variable(X=m.X, kernel=RBF(Q, ARD=True, dtype=dts), noise_var=m.noise_var, shape=(N, 1), dtype=dts, **kw)
    infr = GradBasedInference(MAP(model=m, observed=[m.X, m.Y]), dtype=dts)
    infr.initialize(X=(N, Q), Y=(N, 1))
    infr.run(X=X, Y=Y, learning_rate=0.01, max_iter=2)            # warm-up: library handle, scratch, the neighbour search
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    infr.run(X=X, Y=Y, learning_rate=0.01, max_iter=steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else 'abcd'
    print(torch.cuda.get_device_name(0))
    for dt in (torch.float32, torch.float64):
        for k in (8, 32):
            if 'a' in what or 'b' in what:
                kernels(dt, k, what)
            if 'c' in what:
                print('   (c) VecchiaGPRegression MAP step, N=%d k=%d %s: %.2f ms wall clock' % (N, k, str(dt)[6:], map_step(VecchiaGPRegression, dt, 20, num_neighbours=k)),
                      flush=True)
        if 'd' in what:
            print('   (d) IterativeGPRegression MAP step, N=%d %s: %.1f ms wall clock' % (N, str(dt)[6:], map_step(IterativeGPRegression, dt, 2)), flush=True)


if __name__ == '__main__':
    main()
