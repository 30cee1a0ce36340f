"""Times of the fused coregionalisation Gram pass and its reverse mode (mxf_gram_icm / mxf_gram_icm_bwd, through _GramICMFn) next to the
generic path on the same operands in the same process: HIP events, 5 windows each after a warm-up, every window long enough to pass 0.2 s,
the windows of the two routes ALTERNATING so that a drift of the clocks or of a neighbour's load falls on both.  Per line: the median of
each route, the generic route's run-to-run spread (max - min over its windows, in % of its median), the ratio generic / fused, and the
implied fraction of 8 TB/s of HBM of the fused pass (forward: bytes of K written; reverse: bytes of dK read).  "faster" in DESIGN.md
section 18 means: the fused median is below the generic median by more than that spread.

The generic path is what MultiplyKernel evaluates without the fused branch: the stationary Gram through its autograd function (_GramFn:
mxf_gram / mxf_gram_bwd), the torch gather B[:, idx[:, None], idx2[None, :]], their product, and torch autograd through all three.  The
"reverse" line is each route's forward + reverse median minus its own forward median.
Shapes: N = N2 = 8192 (rectangular call), Q = 8, RBF with ARD, T in {2, 8, 32}, both dtypes; before timing the two routes' outputs are compared.
usage: gram_icm_time.py [T ...]"""
import os
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mxfusion_amd import ops  # noqa: E402
from mxfusion_amd.components.distributions.gp.kernels import kernel as impl  # noqa: E402

HBM = 8e12
N, Q = 8192, 8


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(fn, min_window=0.2):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps = 1
    while window(fn, reps) * reps < 1e3 * min_window and reps < 1 << 16:
        reps *= 2
    return reps


def timed_pair(a, b):
    """5 alternating windows of each: (median a, median b, spread of b in % of its median)"""
    ra, rb = reps_for(a), reps_for(b)
    ta, tb = [], []
    for _ in range(5):
        ta.append(window(a, ra))
        tb.append(window(b, rb))
    return float(np.median(ta)), float(np.median(tb)), 100 * (max(tb) - min(tb)) / float(np.median(tb))


def run(T, dt):
    g = torch.Generator(device='cuda').manual_seed(1)
    u = lambda lo, hi, *shape: torch.rand(*shape, device='cuda', dtype=dt, generator=g) * (hi - lo) + lo
    X, X2, ls, var = u(-2, 2, 1, N, Q), u(-2, 2, 1, N, Q), u(0.8, 1.8, 1, Q), u(0.5, 1.5, 1, 1)
    W = torch.randn(1, T, 2, device='cuda', dtype=dt, generator=g)
    B = (W @ W.transpose(-1, -2) + torch.diag_embed(u(0.5, 1.5, 1, T))).contiguous()
    idx, idx2 = (torch.randint(0, T, (N,), device='cuda', generator=g).to(torch.int32) for _ in range(2))
    i, j = idx.long(), idx2.long()
    dK = torch.randn(1, N, N, device='cuda', dtype=dt, generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (X, X2, ls, var, B)]

    def gram(fused, x, x2, l, v, b):
        if fused:
            return impl._GramICMFn.apply('rbf', True, x, x2, idx, idx2, l, v, b)
        return impl._GramFn.apply('rbf', True, x, x2, l, v) * b[:, i[:, None], j[None, :]]

    def fwd(fused):
        def f():
            with torch.no_grad():
                return gram(fused, X, X2, ls, var, B)
        return f

    def both(fused):
        return lambda: torch.autograd.grad(gram(fused, *leaves), leaves, dK)
    tol = 1e-4 if dt == torch.float32 else 1e-10
    assert torch.allclose(fwd(True)(), fwd(False)(), rtol=tol, atol=tol * float(B.abs().max()))
    for a, b in zip(both(True)(), both(False)()):
        assert torch.allclose(a, b, rtol=10 * tol, atol=10 * tol * max(1.0, float(b.abs().max()))), (a, b)
    nbytes, es = N * N * dK.element_size(), str(dt)[6:]
    tfw, tfb = timed_pair(fwd(True), fwd(False)), timed_pair(both(True), both(False))
    rows = (('forward', tfw[0], tfw[1], tfw[2], nbytes), ('fwd+reverse', tfb[0], tfb[1], tfb[2], 2 * nbytes),
            ('reverse', tfb[0] - tfw[0], tfb[1] - tfw[1], tfb[2] * tfb[1] / (tfb[1] - tfw[1]), nbytes))
    for what, tf, tg, spread, nb in rows:
        verdict = 'fused faster' if tf < tg * (1 - spread / 100) else ('generic faster' if tg < tf * (1 - spread / 100) else 'within the spread')
        print('icm rbf %d x %d Q=%d T=%-2d %-7s %-11s: fused %8.3f ms  generic %8.3f ms (spread %4.1f %%)  generic/fused %5.2f  HBM %5.1f %%  %s'
              % (N, N, Q, T, es, what, tf, tg, spread, tg / tf, 100 * nb / (tf * 1e-3) / HBM, verdict), flush=True)


if __name__ == '__main__':
    Ts = [int(a) for a in sys.argv[1:]] or [2, 8, 32]
    for dt in (torch.float32, torch.float64):
        for T in Ts:
            run(T, dt)
