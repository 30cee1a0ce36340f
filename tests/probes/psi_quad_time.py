"""Times of the per-row contraction of the Psi2 terms, mxf_psi_rbf_quad (HIP events, median of 5 windows after a warm-up, each window long
enough to pass 0.2 s; random operands), at N = 65 536, Q = 8, M = 1 024 with J = 1 and J = 4 weight matrices, both dtypes, beside
mxf_psi_rbf_fwd's Psi2 at the same shape; the rate is in psi2n terms per second (N M (M + 1) / 2 terms a pass).
usage: psi_quad_time.py"""
import os
import sys

import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mxfusion_amd import ops  # noqa: E402
from psi_time import operands, timed  # noqa: E402


def main():
    print(torch.cuda.get_device_name(0))
    N, M, Q = 65536, 1024, 8
    terms = N * M * (M + 1) / 2
    for dt in (torch.float32, torch.float64):
        p = operands(N, M, Q, dt)
        args = [p[k] for k in ('mu', 's', 'Z', 'ls', 'var')] + [True]
        t2 = timed(lambda: ops.psi_rbf(*args, want_psi1=False))
        print('N=%d Q=%d M=%d %s: Psi2 forward %.3f ms [%.3f, %.3f] (%.3g terms/s)' % (N, Q, M, str(dt)[6:], *t2, terms / t2[0] * 1e3), flush=True)
        for J in (1, 4):
            A = torch.rand(1, J, M, M, device='cuda', dtype=dt, generator=torch.Generator(device='cuda').manual_seed(2)) - 0.5
            tq = timed(lambda: ops.psi_rbf_quad(*args, A))
            print('   contraction J=%d %.3f ms [%.3f, %.3f] (%.3g terms/s, %.2f of the Psi2 forward)'
                  % (J, *tq, terms / tq[0] * 1e3, tq[0] / t2[0]), flush=True)


if __name__ == '__main__':
    main()
