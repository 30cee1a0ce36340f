"""Times of the nearest-centre kernels (HIP events, median of 5 windows after a warm-up, each window long enough to pass 0.2 s; standard
normal operands):
  (a) mxf_nearest and mxf_kmeans_step at N = 65 536, Q = 8, M in {16, 1 024}, both dtypes, with the rate in (row, centre) pairs per second
      and the peak device memory of a call above the operands, beside the dense form on the same device: torch.cdist(X, C).argmin(1), and
      for the step that plus index_add_ of the rows and the counts;
  (b) one full util.inducing.kmeans(X, 1024) at N = 65 536, Q = 8 (k-means++ and the Lloyd iterations to tol = 1e-4), wall clock.
usage: kmeans_time.py [a|b]"""
import os
import sys
import time

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mxfusion_amd import ops  # noqa: E402
from mxfusion_amd.util.inducing import kmeans  # noqa: E402


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


def dense_step(X, C):
    idx = torch.cdist(X, C).argmin(1)
    sums = torch.zeros_like(C).index_add_(0, idx, X)
    counts = torch.zeros(C.shape[0], dtype=X.dtype, device=X.device).index_add_(0, idx, torch.ones_like(X[:, 0]))
    return torch.where(counts[:, None] > 0, sums / counts[:, None].clamp_min(1), C), idx


def kernels(N, Q, M, dt):
    g = torch.Generator(device='cuda').manual_seed(M)
    X, C = torch.randn(N, Q, device='cuda', dtype=dt, generator=g), torch.randn(M, Q, device='cuda', dtype=dt, generator=g)
    near, step = (lambda: ops.nearest(X, C)), (lambda: ops.kmeans_step(X, C))
    dnear, dstep = (lambda: torch.cdist(X, C).argmin(1)), (lambda: dense_step(X, C))
    tn, ts, tdn, tds = timed(near), timed(step), timed(dnear), timed(dstep)
    mn, ms, mdn, mds = peak(near), peak(step), peak(dnear), peak(dstep)
    same = float((near()[0].long() == dnear()).double().mean())
    print('N=%d Q=%d M=%d %s' % (N, Q, M, str(dt)[6:]))
    print('   fused: nearest %.4f ms [%.4f, %.4f] (%.3g pairs/s, peak %.2f MiB)   step %.4f ms [%.4f, %.4f] (peak %.2f MiB)'
          % (*tn, N * M / tn[0] * 1e3, mn, *ts, ms))
    print('   cdist + argmin: %.4f ms [%.4f, %.4f] (peak %.2f MiB)   + index_add_: %.4f ms [%.4f, %.4f] (peak %.2f MiB)   rows assigned alike %.6f'
          % (*tdn, mdn, *tds, mds, same), flush=True)


def full(N, Q, M, dt):
    g = torch.Generator(device='cuda').manual_seed(1)
    X = torch.randn(N, Q, device='cuda', dtype=dt, generator=g)
    kmeans(X, 8, num_iter=2)           # warm-up: library handle, scratch
    torch.cuda.synchronize()
    for num_iter in (0, 25):
        t0 = time.perf_counter()
        Z, info = kmeans(X, M, num_iter=num_iter)
        torch.cuda.synchronize()
        print('(b) kmeans(X, %d) N=%d Q=%d %s num_iter=%d: %.1f ms wall clock, %d iterations, converged %s, inertia %.6g -> %.6g'
              % (M, N, Q, str(dt)[6:], num_iter, 1e3 * (time.perf_counter() - t0), info['iterations'], info['converged'],
                 info['inertia'][0] if info['inertia'] else float('nan'), info['inertia'][-1] if info['inertia'] else float('nan')), flush=True)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else 'ab'
    print(torch.cuda.get_device_name(0))
    if 'a' in what:
        for dt in (torch.float32, torch.float64):
            for M in (16, 1024):
                kernels(65536, 8, M, dt)
    if 'b' in what:
        full(65536, 8, 1024, torch.float32)
        full(65536, 8, 1024, torch.float64)


if __name__ == '__main__':
    main()
