"""Times of the matrix-free kernel product on wide inputs, mxf_kmv_wide and mxf_kmv_wide_bwd through ops (HIP events, median of 5 windows
after a warm-up, each window long enough to pass 0.2 s, min and max beside it; random operands): N = N2 = 65 536, Q in {32, 128}, J in
{1, 16}, RBF with ARD, both dtypes, forward and reverse, beside ops.gram + torch.matmul at the same size (the N x N matrix is 17 GB in
float32 and 34 GB in float64), with the peak device memory of a call and the largest difference between the two results.  The figure of
merit is the forward rate in lane-instructions per second at 3.05 Q instructions per pair and pass (what the wide Gram pass
spends, 53 T/s in float32 and 26.5 T/s in float64 there), as a fraction of that pass's rate.
usage: kmv_wide_time.py [f32|f64]"""
import os
import sys

import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mxfusion_amd import ops  # noqa: E402
from kmv_time import timed, peak  # noqa: E402

GRAM_WIDE_RATE = {torch.float32: 53e12, torch.float64: 26.5e12}


def kernels(N, Q, J, dt):
    g = torch.Generator(device='cuda').manual_seed(Q + J)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=dt, generator=g)
    X, ls, var, noise = r(1, N, Q) * 4 - 2, (r(1, Q) + 0.8) * (Q / 3.0) ** 0.5, r(1, 1) + 0.5, r(1, 1) * 0.1 + 0.05
    V, A = torch.randn(1, N, J, device='cuda', dtype=dt, generator=g), torch.randn(1, N, J, device='cuda', dtype=dt, generator=g)
    dls, dvar = torch.zeros_like(ls), torch.zeros_like(var)
    fwd = lambda: ops.kernel_matvec('rbf', X, None, ls, var, True, V, noise)
    bwd = lambda: ops.kernel_matvec_bwd_('rbf', X, None, ls, var, True, A, V, None, dls, dvar)
    dense = lambda: torch.matmul(ops.gram('rbf', X, None, ls, var, True, diag_add=noise), V)
    passes = -(-J // (4 if J <= 4 else (16 if dt == torch.float32 else 8)))
    tf, tb, td = timed(fwd), timed(bwd), timed(dense)
    mf, mb, md = peak(fwd), peak(bwd), peak(dense)
    a, b = fwd(), dense()
    rate = passes * N * N * 3.05 * Q / tf[0] * 1e3
    print('N=N2=%d Q=%d J=%d %s' % (N, Q, J, str(dt)[6:]))
    print('   fused: forward %.3f ms [%.3f, %.3f] (%d passes, %.3g lane-instructions/s = %.2f of the wide Gram pass, peak %.0f MiB)   '
          'reverse %.3f ms [%.3f, %.3f] (peak %.0f MiB)' % (*tf, passes, rate, rate / GRAM_WIDE_RATE[dt], mf, *tb, mb))
    print('   gram + matmul: %.3f ms [%.3f, %.3f] (peak %.0f MiB)   largest difference / largest entry %.1e'
          % (*td, md, float((a - b).abs().max() / b.abs().max())), flush=True)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else 'f32f64'
    print(torch.cuda.get_device_name(0))
    for name, dt in (('f32', torch.float32), ('f64', torch.float64)):
        if name in what:
            for Q in (32, 128):
                for J in (1, 16):
                    kernels(65536, Q, J, dt)


if __name__ == '__main__':
    main()
