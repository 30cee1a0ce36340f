"""Times of the wide-input Gram passes (mxf_gram_wide / mxf_gram_wide_bwd; csrc/gram_wide.hip) next to the route they replace, on the same
operands in the same process, on the protocol of gram_icm_time.py: HIP events, 5 windows each after a warm-up, every window long enough to
pass 0.2 s, the windows of the two routes ALTERNATING.  The two routes are the SAME calls, ops.gram and ops.gram_bwd, with ops.WIDE_GRAM on
and off: off is the parent commit's code (gram_generic_kernel, gram_bwd_generic_kernel).  Per line: the median of each route, the old
route's run-to-run spread (max - min over its windows, in % of its median), the ratio old / new and the fraction of 8 TB/s of HBM that the
new pass reaches (forward: bytes of K written; reverse: bytes of dK read).  "faster" means: the new median is below the old median by more
than that spread.  An old-route call that takes more than SLOW seconds is timed ONCE (after one warm-up call of the new route only) and the
line says "single call": it has no spread, and the verdict is the plain comparison.
The "reverse" line is each route's forward + reverse median minus its own forward median.
Shapes 8192 x 8192 and 1024 x 65536 (rectangular calls), Q in {32, 128, 784}, RBF with ARD and Matern52, both dtypes; length-scales scaled
by sqrt(Q / 4) so that K stays away from underflow.  Before timing the two routes' outputs are compared.
usage: gram_wide_time.py [--budget SECONDS] [--q Q ...] [--dtype f32|f64 ...] [--kind rbf|matern52 ...] [--shape NxN2 ...]
--budget: no new case is started after that many seconds; the cases not run are listed."""
import argparse
import os
import sys
import time

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mxfusion_amd import ops  # noqa: E402

HBM = 8e12
SLOW = 2.0


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(fn, first, min_window=0.2):
    """first: the time (ms) of one call, already measured"""
    reps, t = 1, first
    while t * reps < 1e3 * min_window and reps < 1 << 16:
        reps *= 2
        t = window(fn, reps)
    return reps


def timed_pair(fn, dt):
    """(median new, median old, spread of old in % of its median or None for a single call)"""
    def route(on):
        def f():
            ops.WIDE_GRAM[dt] = on
            fn()
        return f
    new, old = route(True), route(False)
    new()
    new()
    first_old = window(old, 1)
    if first_old > 1e3 * SLOW:
        rn = reps_for(new, window(new, 1))
        return float(np.median([window(new, rn) for _ in range(5)])), first_old, None
    old()
    rn, ro = reps_for(new, window(new, 1)), reps_for(old, window(old, 1))
    tn, to = [], []
    for _ in range(5):
        tn.append(window(new, rn))
        to.append(window(old, ro))
    return float(np.median(tn)), float(np.median(to)), 100 * (max(to) - min(to)) / float(np.median(to))


def run(kind, ard, N, N2, Q, dt):
    g = torch.Generator(device='cuda').manual_seed(1)
    u = lambda lo, hi, *shape: torch.rand(*shape, device='cuda', dtype=dt, generator=g) * (hi - lo) + lo
    X, X2, var = u(-2, 2, 1, N, Q), u(-2, 2, 1, N2, Q), u(0.5, 1.5, 1, 1)
    ls = u(0.8, 1.8, 1, Q if ard else 1) * (Q / 4.0) ** 0.5
    dK = torch.randn(1, N, N2, device='cuda', dtype=dt, generator=g)
    K = torch.empty(1, N, N2, device='cuda', dtype=dt)
    fwd = lambda: ops.gram(kind, X, X2, ls, var, ard, out=K)

    def both():
        fwd()
        return ops.gram_bwd(kind, X, X2, ls, var, ard, dK)
    tol = 1e-4 if dt == torch.float32 else 1e-10
    tfw = timed_pair(fwd, dt)
    ops.WIDE_GRAM[dt] = True
    Kn, gn = fwd().clone(), both()
    ops.WIDE_GRAM[dt] = False
    Ko, go = fwd().clone(), both()
    assert torch.allclose(Kn, Ko, rtol=tol, atol=tol * float(var.max()))
    for a, b in zip(gn, go):
        assert torch.allclose(a, b, rtol=10 * tol, atol=10 * tol * max(1.0, float(b.abs().max()))), (a, b)
    tfb = timed_pair(both, dt)
    nbytes, es = N * N2 * dK.element_size(), str(dt)[6:]
    single = tfb[2] is None or tfw[2] is None
    rows = (('forward', tfw[0], tfw[1], tfw[2], nbytes), ('fwd+reverse', tfb[0], tfb[1], tfb[2], 2 * nbytes),
            ('reverse', tfb[0] - tfw[0], tfb[1] - tfw[1], None if single else tfb[2] * tfb[1] / (tfb[1] - tfw[1]), nbytes))
    for what, tn, to, spread, nb in rows:
        s = 0.0 if spread is None else spread
        verdict = 'new faster' if tn < to * (1 - s / 100) else ('old faster' if to < tn * (1 - s / 100) else 'within the spread')
        print('wide %-8s ard=%d %5d x %5d Q=%-3d %-7s %-11s: new %9.3f ms  old %10.3f ms (%s)  old/new %8.2f  HBM %5.1f %%  %s'
              % (kind, ard, N, N2, Q, es, what, tn, to, 'single call' if spread is None else 'spread %4.1f %%' % spread, to / tn,
                 100 * nb / (tn * 1e-3) / HBM, verdict), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--budget', type=float, default=1e9)
    ap.add_argument('--q', type=int, nargs='*', default=[32, 128, 784])
    ap.add_argument('--dtype', nargs='*', default=['f32', 'f64'])
    ap.add_argument('--kind', nargs='*', default=['rbf', 'matern52'])
    ap.add_argument('--shape', nargs='*', default=['8192x8192', '1024x65536'])
    a = ap.parse_args()
    before, t0, skipped = dict(ops.WIDE_GRAM), time.time(), []
    for Q in a.q:
        for shape in a.shape:
            for kind in a.kind:
                for d in a.dtype:
                    case = (kind, int(kind == 'rbf'), int(shape.split('x')[0]), int(shape.split('x')[1]), Q, torch.float32 if d == 'f32' else torch.float64)
                    if time.time() - t0 > a.budget:
                        skipped.append(case)
                    else:
                        run(*case)
    for dt, on in before.items():
        ops.WIDE_GRAM[dt] = on
    for case in skipped:
        print('not run (budget):', case, flush=True)
