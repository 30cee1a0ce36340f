"""Wall time per call of the pointwise and per-row entry points, straight through the C ABI (no torch wrapper in the way): one representative
entry of each of elementwise.hip, ewise.hip, simplex.hip, univariate.hip, mvn.hip, wishart.hip, dense.hip and transform.hip at a launch-bound
size (n = 1024 elements or rows: what is timed is the host side of the launch), and the flat kernels at a bandwidth-bound one (n = 2^24).
Each figure is the median of 7 windows of calls queued back to back and closed by a synchronise, every window at least 0.1 s long, after a
warm-up; float32.  MXF_GP_LIB selects the library (A/B runs of two builds in one session).
usage: pointwise_time.py [label [small]]      small: the launch-bound size only"""
import ctypes
import os
import sys
import time

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mxfusion_amd import _lib  # noqa: E402


def timed(fn, min_window=0.1):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps, out = 16, []
    while len(out) < 7:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt < min_window and reps < 1 << 20:
            reps *= 2
            continue
        out.append(1e6 * dt / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(_lib.LIB_PATH)
    raw, h, st = _lib.load(), _lib.handle(0), torch.cuda.current_stream().cuda_stream
    F32 = _lib.F32
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)
    buf = lambda n, v=0.5: torch.full((n,), v, dtype=torch.float32, device='cuda')
    print('%s on %s' % (label, torch.cuda.get_device_name(0)))
    for n in (1024,) if 'small' in sys.argv[2:] else (1024, 1 << 24):
        x, y, z = buf(n), buf(n), buf(n)
        p = lambda t: t.data_ptr()
        cases = [('elementwise softplus_fwd', lambda: raw.mxf_softplus_fwd(h, F32, n, p(x), p(y), st)),
                 ('elementwise sgd_step', lambda: raw.mxf_sgd_step(h, F32, n, p(z), p(x), None, 1e-9, 0.0, 0.0, 1.0, st)),
                 ('ewise add (n)', lambda: raw.mxf_ewise_fwd(h, 0, F32, 1, i64s(n), p(x), i64s(1), p(y), i64s(1), p(z), st)),
                 ('univariate gamma elem', lambda: raw.mxf_univariate_logpdf_elem(h, 0, F32, 1, n, p(x), p(y), 1, 0, p(y), 1, 0, 1.0, p(z), st)),
                 ('transform softplus', lambda: raw.mxf_transform_fwd(h, F32, 1, (ctypes.c_int * 1)(0), i64s(n), (ctypes.c_double * 1)(0.0),
                                                                      (ctypes.c_double * 1)(0.0), p(x), p(z), st))]
        if n == 1024:
            K, I, nn = 4, 8, 4
            lp, lab, out = buf(n * K), buf(n, 1.0), buf(n)
            X, W, b, Y = buf(n * I), buf(I * I), buf(I), buf(n * I)
            A = torch.eye(nn, dtype=torch.float32, device='cuda').repeat(n, 1, 1).contiguous()
            F, ld, info = torch.empty_like(A), buf(n), torch.zeros(n, dtype=torch.int32, device='cuda')
            xs, nu = buf(n * nn), buf(n, 6.0)
            raw.mxf_mvn_factor(h, F32, 0, 1, n, nn, p(A), nn, 0, nn * nn, p(F), p(ld), p(info), st)
            cases += [('ewise reduce sum (n, 8, 1)', lambda: raw.mxf_reduce_fwd(h, 0, F32, n, 8, 1, p(X), p(out), st)),
                      ('elementwise coldot (8 x n)', lambda: raw.mxf_coldot(h, F32, 1, 8, n, p(X), n, 0, p(X), n, 0, p(out), st)),
                      ('simplex categorical (n, 4)', lambda: raw.mxf_categorical_logpdf(h, F32, 1, n, K, p(lp), 0, K, p(lab), 0, 0, 1, 1.0, p(out), st)),
                      ('mvn logpdf (n, 4)', lambda: raw.mxf_mvn_logpdf(h, F32, 0, 1, n, nn, p(xs), 0, p(xs), 0, nn, p(F), p(ld), 1, n, 1.0, p(out), st)),
                      ('wishart logpdf (n, 4)', lambda: raw.mxf_wishart_logpdf(h, F32, 1, n, nn, p(A), nn, 0, p(nu), 0, 1, p(A), nn, 0, nn * nn, 1, n, 1.0,
                                                                                p(out), p(info), st)),
                      ('dense fwd (n, 8, 8)', lambda: raw.mxf_dense_fwd(h, F32, 1, n, I, I, 1, p(X), I, 0, p(W), 0, p(b), 0, p(Y), st))]
        for name, fn in cases:
            assert fn() == 0, (name, raw.mxf_last_error(h))
            med, lo, hi = timed(fn)
            print('  n=%-9d %-30s %9.3f us per call [%.3f, %.3f]' % (n, name, med, lo, hi), flush=True)


if __name__ == '__main__':
    main()
