"""A Bayesian neural network on the MI355X: the reference's bnn_regression notebook at N = 32, hidden width 8 (tanh, tanh, linear),
num_samples = 3 -- MXFusionTorchFunction, priors on every weight, a Gaussian mean field, the Monte-Carlo ELBO.

The noise is injected through the rand_gen seam (one MockRandomGenerator per posterior factor), so that a float64 CPU restatement of the
ELBO (torch.func.functional_call on a float64 copy of the network, closed-form Normal log-densities, autograd) sees the same draws; the
code under test never supplies an expected value.  Inputs are rounded to the dtype under test before either side sees them.  Errors are
normwise per output.  float64: 1e-9.  float32: max(4 x the error of the restatement evaluated in float32 on the CPU,
8 * 2^-24 * M / |want|); M is, for the loss, the sum of the absolute values of the three groups of terms (likelihood, prior, entropy), each
of which is a sum of same-signed magnitudes |log N|, and for a gradient the norm of the sum of the absolute gradients of the three groups --
a lower bound of the sum over the individual terms, hence no wider than that rule allows."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, S = 32, 8, 3
F64_BAR = 1e-9
EPS32 = 2.0 ** -24
NOISE_RAW, Q_VAR_RAW = -4.5, -3.0          # the stored (unconstrained) noise and posterior variances: softplus gives 0.011 and 0.049


def _tdt(dtype):
    return torch.float64 if dtype == 'float64' else torch.float32


def _round(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype=np.float32 if dtype == 'float32' else np.float64).astype(np.float64))


def nerr(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), np.finfo(np.float64).tiny))


def make_net(kind='plain'):
    torch.manual_seed(3)
    layers = [torch.nn.Linear(1, H), torch.nn.Tanh(), torch.nn.Linear(H, H), torch.nn.Softsign() if kind == 'softsign' else torch.nn.Tanh(),
              torch.nn.Linear(H, 1)]
    return torch.nn.Sequential(*layers).double()


@functools.lru_cache(maxsize=None)
def data(dtype):
    r = np.random.RandomState(11)
    x = r.rand(N, 1)
    y = np.sin(6 * x) + 0.1 * r.randn(N, 1)
    net = make_net()
    eps = {n.replace('.', '_'): _round(r.randn(S, *p.shape), dtype) for n, p in net.named_parameters()}
    return _round(x, dtype), _round(y, dtype), eps


def _logn(x, mean, var):
    return -0.5 * np.log(2 * np.pi) - 0.5 * torch.log(var) - (x - mean) ** 2 / (2 * var)


def restatement(kind, dtype_in, dtype, priors=True):
    """loss, {name: gradient} and their magnitudes in torch `dtype` on the CPU; the leaves are the stored (unconstrained) values"""
    x, y, eps = data(dtype_in)
    net = make_net(kind)
    tt = lambda t: t.to(dtype)
    leaves = {'noise_raw': torch.full((1,), NOISE_RAW, dtype=dtype).requires_grad_(True)}
    for n, p in net.named_parameters():
        k = n.replace('.', '_')
        leaves[k + '_mean'] = tt(_round(p.detach(), dtype_in)).requires_grad_(True)
        if priors:
            leaves[k + '_var_raw'] = torch.full(p.shape, Q_VAR_RAW, dtype=dtype).requires_grad_(True)
    sp = torch.nn.functional.softplus
    noise = sp(leaves['noise_raw'])
    ll, prior, ent = 0.0, 0.0, 0.0
    n_s = S if priors else 1
    ws = {}
    for n, p in net.named_parameters():
        k = n.replace('.', '_')
        if priors:
            var = sp(leaves[k + '_var_raw'])
            ws[n] = leaves[k + '_mean'] + torch.sqrt(var) * tt(eps[k])
            prior = prior + _logn(ws[n], torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)).sum() / n_s
            ent = ent + _logn(ws[n], leaves[k + '_mean'], var).sum() / n_s
        else:
            ws[n] = leaves[k + '_mean'][None]
    net = net.to(dtype)
    for s in range(n_s):
        r = torch.func.functional_call(net, {n: w[s] for n, w in ws.items()}, (tt(x),))
        ll = ll + _logn(tt(y), r, noise).sum() / n_s
    groups = [ll] + ([prior, -ent] if priors else [])
    loss = -sum(groups)
    names = list(leaves)
    g = torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)
    gmag = [np.zeros(tuple(leaves[k].shape)) for k in names]
    for part in groups:
        for i, gi in enumerate(torch.autograd.grad(part, [leaves[k] for k in names], retain_graph=True, allow_unused=True)):
            if gi is not None:
                gmag[i] = gmag[i] + np.abs(gi.detach().double().numpy())
    return (float(loss.detach()), {k: gi.detach().double().numpy() for k, gi in zip(names, g)},
            sum(abs(float(p.detach())) for p in groups), dict(zip(names, gmag)))


@functools.lru_cache(maxsize=None)
def expected(kind, dtype, priors=True):
    """(loss, gradients, bar of the loss, bars of the gradients)"""
    loss, grads, mloss, mgrads = restatement(kind, dtype, torch.float64, priors)
    tiny = np.finfo(np.float64).tiny
    if dtype == 'float64':
        return loss, grads, F64_BAR, {k: F64_BAR for k in grads}
    loss32, grads32, _, _ = restatement(kind, dtype, torch.float32, priors)
    floor = lambda w, m: 8 * EPS32 * float(np.linalg.norm(m)) / max(float(np.linalg.norm(w)), tiny)
    return (loss, grads, max(4 * nerr(loss32, loss), floor(loss, mloss)),
            {k: max(4 * nerr(grads32[k], grads[k]), floor(grads[k], mgrads[k])) for k in grads})


def build(kind, dtype, priors=True, broadcastable=False, algorithm=None):
    """the notebook's model and its inference, initialised, the posterior at the network's values with the stored variance Q_VAR_RAW, the noise injected"""
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Normal
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    from mxfusion_amd.components.functions import MXFusionTorchFunction
    from mxfusion_amd.components.functions.operators import broadcast_to
    from mxfusion_amd.components.variables.var_trans import PositiveTransformation
    from mxfusion_amd.inference import GradBasedInference, StochasticVariationalInference, create_Gaussian_meanfield, BatchInferenceLoop, MAP
    x, y, eps = data(dtype)
    dev = lambda t: t.to(_tdt(dtype)).cuda()
    net = make_net(kind)
    m = Model()
    m.N = Variable()
    m.f = MXFusionTorchFunction(net, num_outputs=1, name='nn', broadcastable=broadcastable)
    m.x = Variable(shape=(m.N, 1))
    m.v = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=torch.tensor([0.01], dtype=torch.float64))
    m.r = m.f(m.x)
    if priors:
        for v in m.r.factor.parameters.values():
            v.set_prior(Normal(mean=broadcast_to(torch.tensor([0.]), v.shape), variance=broadcast_to(torch.tensor([1.]), v.shape)))
    m.y = Normal.define_variable(mean=m.r, variance=broadcast_to(m.v, (m.N, 1)), shape=(m.N, 1))
    observed = [m.y, m.x]
    if priors:
        q = create_Gaussian_meanfield(model=m, observed=observed)
        alg = StochasticVariationalInference(num_samples=S, model=m, posterior=q, observed=observed)
    else:
        q = None
        alg = MAP(model=m, observed=observed)
    infr = GradBasedInference(inference_algorithm=alg, grad_loop=BatchInferenceLoop(), dtype=dtype)
    infr.initialize(y=dev(y), x=dev(x))
    infr.params.raw(m.v).fill_(NOISE_RAW)
    if priors:
        for name, v in m.r.factor.parameters.items():
            k = name[len('nn_'):]
            infr.params[q[v].factor.mean] = dev(dict(net.named_parameters())[m.f.torch_name(name)].detach())
            infr.params.raw(q[v].factor.variance).fill_(Q_VAR_RAW)
            q[v].factor._rand_gen = MockRandomGenerator(dev(eps[k]))
    return m, q, infr, net, (dev(y), dev(x))


def loss_and_grads(m, q, infr, batch):
    infr.params.zero_grad()
    loss, loss_for_gradient = infr.create_executor()(*batch)
    loss_for_gradient.backward()
    torch.cuda.synchronize()
    got = {'noise_raw': infr.params.grad(m.v)}
    for name, v in m.r.factor.parameters.items():
        k = name[len('nn_'):]
        if q is not None:
            got[k + '_mean'] = infr.params.grad(q[v].factor.mean)
            got[k + '_var_raw'] = infr.params.grad(q[v].factor.variance)
        else:
            got[k + '_mean'] = infr.params.grad(v)
    return float(loss.detach()), {k: g.detach().double().cpu().numpy().copy() for k, g in got.items()}


def check(what, got, want):
    loss, grads = got
    wloss, wgrads, bloss, bgrads = want
    e = nerr(loss, wloss)
    errs = {k: nerr(grads[k], wgrads[k]) for k in wgrads}
    worst = max(errs, key=lambda k: errs[k] / bgrads[k])
    print('bnn %s: loss %.9g (want %.9g) error %.3g (bar %.3g); worst gradient %s %.3g (bar %.3g); widest bar %.3g'
          % (what, loss, wloss, e, bloss, worst, errs[worst], bgrads[worst], max(bgrads.values())))
    assert e <= bloss, (what, 'loss', e, bloss)
    for k in wgrads:
        assert grads[k].shape == wgrads[k].shape, (k, grads[k].shape, wgrads[k].shape)
        assert errs[k] <= bgrads[k], (what, k, errs[k], bgrads[k])


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bnn_elbo_and_gradients_match_the_restatement(dtype):
    m, q, infr, net, batch = build('plain', dtype)
    assert m.f.plan is not None and len(m.f.plan) == 3
    check('fused ' + dtype, loss_and_grads(m, q, infr, batch), expected('plain', dtype))
    for name, p in net.named_parameters():                 # the parameters are passed in, never written into the module
        assert torch.equal(p, dict(make_net().named_parameters())[name])


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bnn_fused_path_matches_the_generic_loop(dtype, monkeypatch):
    from mxfusion_amd.components.functions import torch_function
    m, q, infr, net, batch = build('plain', dtype)
    fused = loss_and_grads(m, q, infr, batch)
    monkeypatch.setattr(torch_function, 'FUSED_DENSE', False)
    generic = loss_and_grads(m, q, infr, batch)
    want = expected('plain', dtype)
    check('generic loop ' + dtype, generic, want)
    check('fused against the generic loop ' + dtype, fused, (generic[0], generic[1]) + want[2:])


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bnn_unsupported_layer_takes_the_generic_path(dtype, monkeypatch):
    from mxfusion_amd import ops
    m, q, infr, net, batch = build('softsign', dtype)
    assert m.f.plan is None
    monkeypatch.setattr(ops, 'dense', lambda *a, **k: pytest.fail('the fused layer ran for a module that does not qualify'))
    check('softsign ' + dtype, loss_and_grads(m, q, infr, batch), expected('softsign', dtype))


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bnn_free_parameters_under_map(dtype):
    """no priors: every network parameter is a free parameter at the module's value; broadcastable=True (one call) gives the same"""
    want = expected('plain', dtype, priors=False)
    m, q, infr, net, batch = build('plain', dtype, priors=False)
    for name, v in m.r.factor.parameters.items():
        assert nerr(infr.params[v].double().cpu().numpy(), dict(net.named_parameters())[m.f.torch_name(name)].detach().numpy()) <= (1e-15 if dtype == 'float64' else EPS32)
    fused = loss_and_grads(m, q, infr, batch)
    check('free parameters ' + dtype, fused, want)
    mb, qb, infrb, _, batchb = build('plain', dtype, priors=False, broadcastable=True)
    assert mb.r.factor.broadcastable
    one_call = loss_and_grads(mb, qb, infrb, batchb)
    check('broadcastable ' + dtype, one_call, want)
    check('fused against broadcastable ' + dtype, fused, (one_call[0], one_call[1]) + want[2:])
    infr.run(max_iter=50, learning_rate=1e-2, y=batch[0], x=batch[1])
    after = float(infr.create_executor()(*batch)[0].detach())
    print('bnn MAP %s: loss %.6g -> %.6g after 50 Adam steps' % (dtype, fused[0], after))
    assert after < fused[0]


def test_bnn_prediction_at_a_collapsed_posterior():
    from mxfusion_amd.inference import VariationalPosteriorForwardSampling
    m, q, infr, net, batch = build('plain', 'float32')
    for v in m.r.factor.parameters.values():
        infr.params[q[v].factor.variance] = torch.full(v.shape, 1e-12, dtype=torch.float64)
    xt = torch.linspace(0, 1, 17, dtype=torch.float64)[:, None]
    infr2 = VariationalPosteriorForwardSampling(10, [m.x], infr, [m.r])
    res = infr2.run(x=xt.float().cuda())[0]
    assert tuple(res.shape) == (10, 17, 1)
    want = net(xt.float().double()).detach().numpy()
    err = max(nerr(res[i].double().cpu().numpy(), want) for i in range(10))
    print('bnn prediction: worst relative error of 10 draws %.3g' % err)
    assert err <= 1e-5


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_bnn_checkpoint_round_trip(dtype, tmp_path):
    m, q, infr, net, batch = build('plain', dtype)
    r = np.random.RandomState(5)
    for v in m.r.factor.parameters.values():               # away from the values a fresh build starts at
        infr.params[q[v].factor.mean] = torch.as_tensor(r.randn(*v.shape))
    loss = loss_and_grads(m, q, infr, batch)[0]
    path = str(tmp_path / 'bnn.zip')
    infr.save(path)
    m2, q2, infr2, _, batch2 = build('plain', dtype)
    assert nerr(loss_and_grads(m2, q2, infr2, batch2)[0], loss) > 1e-3
    infr2.load(path)
    again = loss_and_grads(m2, q2, infr2, batch2)[0]
    print('bnn checkpoint %s: loss %.17g, after the round trip %.17g' % (dtype, loss, again))
    assert nerr(again, loss) <= 8 * (2.0 ** -52 if dtype == 'float64' else EPS32)       # (the log-density sums add their workgroups' parts in any order)
    c = m.clone()
    assert type(c.r.factor).__name__ == 'TorchFunctionEvaluation' and c.r.factor.function.module is net
    assert 'TorchFunctionEvaluation(nn_input_0=' in repr(c)
