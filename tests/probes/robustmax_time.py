"""Times of the robust-max expectation beside the nearest existing kernel (HIP events, median of 5 windows after a warm-up, each window long
enough to pass 0.2 s -- the method of lik_time.py), at n = 65 536, 20 nodes, S = 1, both dtypes, value and gradients:
  (a) mxf_robustmax_expect at C = 10: n nq (C - 1) evaluations of log Phi;
  (b) mxf_lik_expect, Bernoulli probit, at P = 10: n nq P evaluations of the same log Phi;
and mxf_robustmax_probs at C = 10 (n nq C (C - 1) evaluations).  usage: robustmax_time.py"""
import os
import sys

import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mxfusion_amd import ops  # noqa: E402
from lik_time import timed  # noqa: E402


def main():
    n, C, nq = 65536, 10, 20
    for dt in (torch.float32, torch.float64):
        g = torch.Generator(device='cuda').manual_seed(0)
        m = torch.rand(1, n, C, device='cuda', dtype=dt, generator=g) * 6 - 3
        v = torch.rand(1, n, device='cuda', dtype=dt, generator=g) * 2 + 0.01
        y = torch.randint(0, C, (1, n, 1), device='cuda', generator=g).to(dt)
        yb = torch.randint(0, 2, (1, n, C), device='cuda', generator=g).to(dt)
        out, dm, dv = torch.zeros(1, device='cuda', dtype=dt), torch.zeros_like(m), torch.zeros_like(v)
        a = timed(lambda: ops.robustmax_expect_(y, m, v, 1e-3, 1.0, out, dm_acc=dm, dv_acc=dv, num_nodes=nq))
        b = timed(lambda: ops.lik_expect_('bernoulli_probit', yb, m, v, 1.0, out, dm_acc=dm, dv_acc=dv, num_nodes=nq))
        c = timed(lambda: ops.robustmax_probs(m, v, num_nodes=nq))
        name = str(dt)[6:]
        print('(a) robustmax_expect C=%d %s: %.4f ms [%.4f, %.4f]' % (C, name, *a), flush=True)
        print('(b) lik_expect probit P=%d %s: %.4f ms [%.4f, %.4f]   ratio (a)/(b) %.3f, (C - 1) / P = %.3f' % (C, name, *b, a[0] / b[0], (C - 1) / C),
              flush=True)
        print('    robustmax_probs C=%d %s: %.4f ms [%.4f, %.4f]' % (C, name, *c), flush=True)


if __name__ == '__main__':
    main()
