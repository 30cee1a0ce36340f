"""Times of the likelihood expectation (HIP events, median of 5 windows after a warm-up, each window long enough to pass 0.2 s):
  (a) mxf_lik_expect with gradients at n = 65 536, P = 1, 20 nodes, S in {1, 32}, both dtypes, three kinds;
  (b) the same value and gradients as a torch expression on the device (autograd through the (S, n, P, K) intermediate; logit and Poisson
      only -- the float32 torch log_ndtr is not finite over the tails, which is why (a) exists);
  (c) one bound-plus-gradient evaluation of SVGPLikelihood at N = 65 536, Q = 8, M = 1 024 in float64.
usage: lik_time.py"""
import math
import os
import sys

import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mxfusion_amd import ops  # noqa: E402


def timed(fn, min_window=0.2):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps, out = 4, []
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


def torch_expect(kind, y, m, v, x, w):
    f = m.unsqueeze(-1) + torch.sqrt(2.0 * v.clamp(min=0.0))[..., None, None] * x
    yy = y.unsqueeze(-1)
    g = torch.nn.functional.logsigmoid((2.0 * yy - 1.0) * f) if kind == 'bernoulli_logit' else yy * f - torch.exp(f) - torch.lgamma(yy + 1.0)
    return (g * w).sum(-1).sum((-1, -2))


def main():
    n, P, nq = 65536, 1, 20
    xs, ws = np.polynomial.hermite.hermgauss(nq)
    for dt in (torch.float32, torch.float64):
        x, w = torch.as_tensor(xs, dtype=dt).cuda(), torch.as_tensor(ws / math.sqrt(math.pi), dtype=dt).cuda()
        for S in (1, 32):
            g = torch.Generator(device='cuda').manual_seed(0)
            m = torch.rand(S, n, P, device='cuda', dtype=dt, generator=g) * 6 - 3
            v = torch.rand(S, n, device='cuda', dtype=dt, generator=g) * 2 + 0.01
            for kind in ('bernoulli_logit', 'bernoulli_probit', 'poisson_exp'):
                y = torch.randint(0, 2, (1, n, P), device='cuda', generator=g).to(dt)
                out, dm, dv = torch.zeros(S, device='cuda', dtype=dt), torch.zeros_like(m), torch.zeros_like(v)
                a = timed(lambda: ops.lik_expect_(kind, y, m, v, 1.0, out, dm_acc=dm, dv_acc=dv, num_nodes=nq))
                line = '(a) %s %s S=%d: %.4f ms [%.4f, %.4f]' % (kind, str(dt)[6:], S, *a)
                if kind != 'bernoulli_probit':
                    mm, vv = m.clone().requires_grad_(True), v.clone().requires_grad_(True)
                    b = timed(lambda: torch.autograd.grad(torch_expect(kind, y, mm, vv, x, w).sum(), [mm, vv]))
                    line += '   (b) torch: %.4f ms [%.4f, %.4f]' % b
                print(line, flush=True)
    module_step()


def module_step():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions.gp.kernels import RBF
    from mxfusion_amd.modules.gp_modules import SVGPLikelihood, BernoulliLogit
    from mxfusion_amd.util.inference import VariablesDict
    N, Q, M = 65536, 8, 1024
    mdl = Model()
    mdl.N = Variable()
    mdl.X = Variable(shape=(mdl.N, Q))
    mdl.Z = Variable(shape=(M, Q))
    mdl.Y = SVGPLikelihood.define_variable(X=mdl.X, kernel=RBF(Q, ARD=True, dtype='float64'), likelihood=BernoulliLogit(), inducing_inputs=mdl.Z,
                                           shape=(mdl.N, 1), dtype='float64')
    gp = mdl.Y.factor
    post, kp = gp._extra_graphs[0], gp.kernel.parameters
    g = torch.Generator(device='cuda').manual_seed(1)
    r = lambda *s: torch.rand(*s, device='cuda', dtype=torch.float64, generator=g)
    X = r(1, N, Q) * 6 - 3
    leaves = {mdl.Z.uuid: X[:, :M].clone(), post.qU_mean.uuid: r(1, M, 1) - 0.5, post.qU_cov_W.uuid: 0.01 * (r(1, M, M) - 0.5),
              post.qU_cov_diag.uuid: r(1, M) + 0.5, kp['rbf_lengthscale'].uuid: torch.full((1, Q), 2.0, device='cuda', dtype=torch.float64),
              kp['rbf_variance'].uuid: torch.ones(1, 1, device='cuda', dtype=torch.float64)}
    for t in leaves.values():
        t.requires_grad_(True)
    vs = VariablesDict(dict(leaves))
    vs[mdl.X.uuid], vs[mdl.Y.uuid] = X, (r(1, N, 1) < 0.5).double()
    alg = gp.svgp_log_pdf
    alg.jitter = 1e-6

    def step():
        torch.autograd.grad(alg.compute(None, vs).sum(), list(leaves.values()))
    c = timed(step, min_window=0.5)
    print('(c) SVGPLikelihood bound + gradients, N=%d Q=%d M=%d float64: %.2f ms [%.2f, %.2f]  info %d' % (N, Q, M, *c, int(alg._last_info.abs().sum())))


if __name__ == '__main__':
    main()
