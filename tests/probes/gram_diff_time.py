"""Times of the difference-form Gram pass and its reverse mode (mxf_gram_diff / mxf_gram_diff_bwd; HIP events, median of 5 windows after a
warm-up, each window long enough to pass 0.2 s) for Periodic, RQ and SpectralMixture (A = 4) in both dtypes at
  N = N2 = 8192 (rectangular call: two operands), Q in {1, 8};   M x N = 1024 x 65 536, Q = 8 (what SVGP forms),
next to the same Gram and the same gradients from the torch broadcast expression (tests/_gram_diff_ref.components and autograd) on the same
device in the same process.  Per line: ms of the HIP pass, ms of the torch expression, their ratio, and the implied fraction of 8 TB/s of HBM
(forward: bytes of K written; reverse: bytes of dK read).  For SpectralMixture the rate in (pair, component) evaluations per second is printed
as well, and for float32 at Q = 8 the implied fraction of VALU issue: that rate times the VALU instructions per (pair, component) counted in the
gfx950 assembly of the shipped build (hipcc -S of csrc/gram_diff.hip, Q tile 8: the forward component loop is one block of 60 VALU
instructions, 9 of them transcendental; the reverse row loop 140, 17 transcendental, plus 64 for the reduce-scatter and its LDS atomics and
22 for the loop head and the dK load = 226) over 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz, every instruction counted as one issue slot.
usage: gram_diff_time.py [periodic|rq|sm ...]"""
import os
import sys

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from mxfusion_amd import ops  # noqa: E402
import _gram_diff_ref as R  # noqa: E402

HBM = 8e12
A = 4
VALU_SLOTS = 256 * 4 * 16 * 2.4e9                     # lane-instructions per second
SM_VALU = {'forward': 60, 'reverse': 226}              # per (pair, component), float32, Q tile 8 (module docstring)


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
    return float(np.median(out))


def operands(kind, N, N2, Q, dt):
    g = torch.Generator(device='cuda').manual_seed(1)
    u = lambda lo, hi, *shape: torch.rand(*shape, device='cuda', dtype=dt, generator=g) * (hi - lo) + lo
    X, X2 = u(-2, 2, N, Q), u(-2, 2, N2, Q)
    if kind == 'sm':
        return X, X2, u(0.3, 1.0, A), u(0.05, 0.6, A, Q), u(0.05, 0.4, A, Q)
    return X, X2, u(0.5, 1.5, 1), u(0.8, 1.8, Q), (u(0.7, 2.5, Q) if kind == 'periodic' else u(0.5, 3.0, 1))


def torch_gram(kind, X, X2, p0, p1, p2):
    if kind != 'sm':
        return R.components(kind, X, X2, p0, p1, p2)[0]
    K = 0                                   # one component at a time: the (A, N, N2, Q) temporary would not fit beside its reverse mode
    for a in range(p0.shape[0]):
        K = K + R.components(kind, X, X2, p0[a:a + 1], p1[a:a + 1], p2[a:a + 1])[0]
    return K


def run(kind, N, N2, Q, dt):
    o = operands(kind, N, N2, Q, dt)
    b = [t[None] for t in o]
    dK = torch.randn(1, N, N2, device='cuda', dtype=dt)
    out = torch.empty(1, N, N2, device='cuda', dtype=dt)
    nbytes, es = N * N2 * dK.element_size(), str(dt)[6:]
    leaves = [t.clone().requires_grad_(True) for t in o]

    def torch_bwd():
        torch.autograd.grad((torch_gram(kind, *leaves) * dK[0]).sum(), leaves)

    def torch_fwd():
        with torch.no_grad():
            torch_gram(kind, *o)
    rows = (('forward', lambda: ops.gram_diff(kind, *b, True, out=out), torch_fwd), ('reverse', lambda: ops.gram_diff_bwd(kind, *b, True, dK), torch_bwd))
    for what, hip, ref in rows:
        th, tt = timed(hip), timed(ref)
        rate = N * N2 * A / (th * 1e-3)
        extra = '  %.3g pair-components/s' % rate if kind == 'sm' else ''
        if kind == 'sm' and Q == 8 and dt == torch.float32:
            extra += '  VALU %.0f %%' % (100 * rate * SM_VALU[what] / VALU_SLOTS)
        print('%-8s %5d x %-6d Q=%d %-7s %s: hip %8.3f ms  torch %9.3f ms  torch/hip %6.1f  HBM %5.1f %%%s'
              % (kind, N, N2, Q, es, what, th, tt, tt / th, 100 * nbytes / (th * 1e-3) / HBM, extra), flush=True)


if __name__ == '__main__':
    kinds = sys.argv[1:] or list(R.KINDS)
    for kind in kinds:
        for dt in (torch.float32, torch.float64):
            for N, N2, Q in ((8192, 8192, 1), (8192, 8192, 8), (1024, 65536, 8)):
                run(kind, N, N2, Q, dt)
