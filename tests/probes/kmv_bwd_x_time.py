"""Times of the reverse mode of the matrix-free kernel product in its inputs (HIP events, median of 5 windows after a warm-up, each window long
enough to pass 0.2 s; random operands, RBF with ARD, square):
  mxf_kmv_bwd_x beside mxf_kmv_bwd at N = N2 = 65 536, Q = 8, J in {1, 16}, both dtypes, with the device memory the first call of each shape
  takes above the operands (the handle's scratch included: free device memory before and after), and at N = 16 384 beside ops.gram_bwd on
  the written-out cotangent dK = A V^T with the largest difference between the two gradients.
usage: kmv_bwd_x_time.py"""
import os
import sys

import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mxfusion_amd import ops  # noqa: E402
from kmv_time import timed  # noqa: E402


def shape(N, Q, J, dt, dense):
    g = torch.Generator(device='cuda').manual_seed(J)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=dt, generator=g)
    X, ls, var = r(1, N, Q) * 4 - 2, r(1, Q) + 1.0, r(1, 1) + 0.5
    V, A = torch.randn(1, N, J, device='cuda', dtype=dt, generator=g), torch.randn(1, N, J, device='cuda', dtype=dt, generator=g)
    dls, dvar, dX = torch.zeros_like(ls), torch.zeros_like(var), torch.zeros_like(X)
    bwd = lambda: ops.kernel_matvec_bwd_('rbf', X, None, ls, var, True, A, V, None, dls, dvar)
    bwd_x = lambda: ops.kernel_matvec_bwd_x_('rbf', X, None, ls, var, True, A, V, None, dX)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    bwd_x()
    torch.cuda.synchronize()
    took = (free0 - torch.cuda.mem_get_info()[0]) / 2.0 ** 20
    tx, tb = timed(bwd_x), timed(bwd)
    print('N=N2=%d Q=%d J=%d %s' % (N, Q, J, str(dt)[6:]))
    print('   mxf_kmv_bwd_x %.3f ms [%.3f, %.3f] (%.3g pairs/s, first call took %.0f MiB)   mxf_kmv_bwd %.3f ms [%.3f, %.3f]'
          % (*tx, N * N / tx[0] * 1e3, took, *tb), flush=True)
    if dense:
        dK = torch.matmul(A, V.transpose(1, 2)).contiguous()
        dn = lambda: ops.gram_bwd('rbf', X, None, ls, var, True, dK, need=('X',))
        td = timed(dn)
        dX.zero_()
        bwd_x()
        ref = dn()[0]
        print('   ops.gram_bwd on dK (%.0f MiB) %.3f ms [%.3f, %.3f]   largest difference / largest entry %.1e'
              % (dK.numel() * dK.element_size() / 2.0 ** 20, *td, float((dX - ref).abs().max() / ref.abs().max())), flush=True)


def main():
    print(torch.cuda.get_device_name(0))
    for dt in (torch.float32, torch.float64):
        for J in (1, 16):
            shape(65536, 8, J, dt, False)
        shape(16384, 8, 16, dt, True)


if __name__ == '__main__':
    main()
