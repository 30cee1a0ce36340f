"""ScoreFunctionInference / ScoreFunctionRBInference on the MI355X against float64 CPU restatements (tests/_score_ref.py; tolerances there).

Deterministic: the noise is injected through one MockRandomGenerator per posterior factor.  (a) Normal-Normal: K = 3 scalar latent
variables z_k ~ N(0, 1), N = 5 observations x_n ~ N(z_1 + z_2 + z_3, v) with v a PositiveTransformation parameter, the Gaussian mean field,
S = 4.  (b) Bernoulli latent: z ~ Bernoulli(pi) of shape (3,), x ~ N(dot(z, w), v) built with the operators, q(z) = Bernoulli(prob
parameter), the 0/1 draws injected.  The loss and the model parameter's gradient are compared with StochasticVariationalInference on the
same noise, the posterior parameters' gradients with the restatement's (1/S) sum_s (f_s - b_s) grad log q(z_s).

Statistical (float64): model (b) with the real generator, torch.manual_seed(0), S = 4096.  The exact ELBO gradient and the per-component
variance of the baseline=None per-sample term come from enumerating the 8 configurations on the CPU; the bound is 6 sqrt(var / S).  The
inputs give |E f| >= 3 std(f) (asserted), so the leave-one-out baseline cannot widen the spread.  With a float64 CPU restatement of the
sampler (torch.manual_seed(0), uniform < prob) the worst component sat at 1.6 (None) and 0.22 ('loo') of the bound's sigma; |E f| = 4.9 std(f)."""
import functools

import numpy as np
import pytest
import torch

import _score_ref as R

pytestmark = pytest.mark.gpu

K, N, S = 3, 5, 4
V_RAW = 0.3


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=R.tdt(dtype)).cuda()


# ---- (a) Normal-Normal ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def nn_data(dtype):
    r = np.random.RandomState(4)
    return dict(x=R.rnd(0.8 + 0.5 * r.randn(N), dtype), eps=[R.rnd(r.randn(S, 1), dtype) for _ in range(K)],
                mean=[R.rnd(0.3 * r.randn(1), dtype) for _ in range(K)], var_raw=[R.rnd(r.uniform(-1.5, -0.5, 1), dtype) for _ in range(K)])


def nn_restatement(dtype_in, rb, baseline, dtype=torch.float64):
    """f (S,) and the posterior gradients [(d mean_k, d var_raw_k)] with their magnitudes, of the ELBO (not of the loss)"""
    d = nn_data(dtype_in)
    t = lambda a: torch.as_tensor(a, dtype=dtype)
    means = [t(m).requires_grad_(True) for m in d['mean']]
    raws = [t(v).requires_grad_(True) for v in d['var_raw']]
    with torch.no_grad():
        z = [m + torch.sqrt(R.softplus(v)) * t(e) for m, v, e in zip(means, raws, d['eps'])]          # (S, 1) each, detached draws
    v = R.softplus(t([V_RAW]))
    lik = R.lognormal(t(d['x'])[None, :], z[0] + z[1] + z[2], v).sum(dim=1)
    prior = [R.lognormal(zk, t(0.0), t(1.0)).sum(dim=1) for zk in z]
    qk = lambda k: R.lognormal(z[k], means[k], R.softplus(raws[k])).sum(dim=1)
    q = sum(qk(k) for k in range(K))
    f = (lik + sum(prior) - q).detach()
    grads, mags = [], []
    for k in range(K):
        fk = (lik + prior[k] - qk(k)).detach() if rb else f
        w = fk - (R.loo(fk) if baseline == 'loo' else 0.0)
        g = torch.autograd.grad((qk(k) * w).mean(), [means[k], raws[k]])
        per = [torch.autograd.grad(qk(k)[s] * w[s] / S, [means[k], raws[k]]) for s in range(S)]
        grads.append([x.double().numpy() for x in g])
        mags.append([sum(abs(p[j].double().numpy()) for p in per) for j in range(2)])
    return f.double().numpy(), grads, mags


def nn_build(cls, dtype, **kw):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.distributions import Normal
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    from mxfusion_amd.components.variables.var_trans import PositiveTransformation
    from mxfusion_amd.inference import GradBasedInference, BatchInferenceLoop, create_Gaussian_meanfield
    d = nn_data(dtype)
    m = Model()
    m.v = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=torch.tensor([1.0], dtype=torch.float64))
    m.z0 = Normal.define_variable(mean=0., variance=1., shape=(1,))
    m.z1 = Normal.define_variable(mean=0., variance=1., shape=(1,))
    m.z2 = Normal.define_variable(mean=0., variance=1., shape=(1,))
    m.x = Normal.define_variable(mean=m.z0 + m.z1 + m.z2, variance=m.v, shape=(N,))
    q = create_Gaussian_meanfield(model=m, observed=[m.x])
    alg = cls(num_samples=S, model=m, posterior=q, observed=[m.x], **kw)
    infr = GradBasedInference(inference_algorithm=alg, grad_loop=BatchInferenceLoop(), dtype=dtype)
    batch = (_dev(d['x'], dtype),)
    infr.initialize(x=batch[0])
    infr.params.raw(m.v).fill_(V_RAW)
    zs = [m.z0, m.z1, m.z2]
    for k, zv in enumerate(zs):
        infr.params[q[zv].factor.mean] = _dev(d['mean'][k], dtype)
        infr.params.raw(q[zv].factor.variance).copy_(_dev(d['var_raw'][k], dtype))
        q[zv].factor._rand_gen = MockRandomGenerator(_dev(d['eps'][k], dtype))
    return m, q, infr, batch, zs


def run(infr, batch, variables):
    infr.params.zero_grad()
    loss, for_gradient = infr.create_executor()(*batch)
    for_gradient.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), [infr.params.grad(v).detach().double().cpu().numpy().copy() for v in variables]


def close_to_svi(what, got, want, dtype):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bar = R.F64_BAR * np.abs(want) if dtype == 'float64' else R.F32_ATOL + R.F32_RTOL * np.abs(want)
    assert (np.abs(got - want) <= bar).all(), (what, got, want)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('baseline', [None, 'loo'])
@pytest.mark.parametrize('rb', [False, True])
def test_normal_normal_against_svi_and_the_restatement(rb, baseline, dtype):
    from mxfusion_amd.inference import ScoreFunctionInference, ScoreFunctionRBInference, StochasticVariationalInference
    m, q, infr, batch, zs = nn_build(ScoreFunctionRBInference if rb else ScoreFunctionInference, dtype, baseline=baseline)
    post = [p for zv in zs for p in (q[zv].factor.mean, q[zv].factor.variance)]
    loss, grads = run(infr, batch, [m.v] + post)
    ms, qs, infr_s, batch_s, _ = nn_build(StochasticVariationalInference, dtype)
    loss_svi, grads_svi = run(infr_s, batch_s, [ms.v])
    # (SVI's loss is a sum of per-factor means, this one a mean of per-sample sums: the same addends in another order)
    f, want, mags = nn_restatement(dtype, rb, baseline)
    mag_loss = np.abs(f).mean()
    if dtype == 'float64':
        assert abs(loss - loss_svi) <= R.F64_BAR * max(mag_loss, abs(loss_svi)), (loss, loss_svi)
        assert abs(loss + f.mean()) <= R.F64_BAR * mag_loss
    else:
        close_to_svi('loss', loss, loss_svi, dtype)
    close_to_svi('model parameter', grads[0], grads_svi[0], dtype)
    if dtype == 'float32':
        _, want32, _ = nn_restatement(dtype, rb, baseline, torch.float32)
        R.assert_float32_formula_meets_the_bar(('normal-normal', rb, baseline), [g for pair in want32 for g in pair], [g for pair in want for g in pair])
    for k in range(K):
        for j, name in enumerate(('mean', 'variance (stored)')):
            R.assert_close(('posterior', k, name, rb, baseline), -grads[1 + 2 * k + j], want[k][j], mags[k][j], dtype)


def test_rao_blackwellised_gradient_differs_on_the_normal_normal_model():
    """otherwise the test above could not tell the two classes apart"""
    for baseline in (None, 'loo'):
        _, plain, _ = nn_restatement('float64', False, baseline)
        _, rb, _ = nn_restatement('float64', True, baseline)
        assert max(abs(plain[k][j] - rb[k][j]).max() / abs(plain[k][j]).max() for k in range(K) for j in range(2)) > 1e-2


# ---- (b) Bernoulli latent ------------------------------------------------------------------------------------------------------------

PRIOR = np.array([0.3, 0.5, 0.6])
Q0 = np.array([0.35, 0.6, 0.45])


@functools.lru_cache(maxsize=None)
def bern_data(dtype):
    r = np.random.RandomState(9)
    w = R.rnd(0.3 * r.randn(K, N), dtype)
    return dict(w=w, x=R.rnd(0.4 + 0.3 * r.randn(N), dtype), z=(r.rand(S, K) < 0.5).astype(np.float64), prior=R.rnd(PRIOR, dtype), q0=R.rnd(Q0, dtype))


def bern_f(z, qp, d, v, dtype=torch.float64):
    """(f, log q) for configurations z (C, K); f = log p(x, z) - log q(z)"""
    t = lambda a: torch.as_tensor(a, dtype=dtype)
    pri = t(d['prior'])
    lp = (z * torch.log(pri) + (1 - z) * torch.log1p(-pri)).sum(dim=1) + R.lognormal(t(d['x'])[None, :], z @ t(d['w']), v).sum(dim=1)
    lq = (z * torch.log(qp) + (1 - z) * torch.log1p(-qp)).sum(dim=1)
    return lp - lq, lq


def bern_restatement(dtype_in, baseline, dtype=torch.float64):
    d = bern_data(dtype_in)
    qp = torch.as_tensor(d['q0'], dtype=dtype).requires_grad_(True)
    v = R.softplus(torch.as_tensor([V_RAW], dtype=dtype))
    z = torch.as_tensor(d['z'], dtype=dtype)
    f, lq = bern_f(z, qp, d, v, dtype)
    f = f.detach()
    w = f - (R.loo(f) if baseline == 'loo' else 0.0)
    g = torch.autograd.grad((lq * w).mean(), qp, retain_graph=True)[0]
    mag = sum(abs(torch.autograd.grad(lq[s] * w[s] / S, qp, retain_graph=True)[0].double().numpy()) for s in range(S))
    return f.double().numpy(), g.double().numpy(), mag


def bern_build(cls, dtype, num_samples=S, mock=True, **kw):
    from mxfusion_amd import Model, Variable, Posterior
    from mxfusion_amd.components.distributions import Normal, Bernoulli
    from mxfusion_amd.components.distributions.random_gen import MockRandomGenerator
    from mxfusion_amd.components.functions.operators import dot, reshape
    from mxfusion_amd.components.variables.var_trans import PositiveTransformation
    from mxfusion_amd.inference import GradBasedInference, BatchInferenceLoop
    d = bern_data(dtype)
    m = Model()
    m.v = Variable(shape=(1,), transformation=PositiveTransformation(), initial_value=torch.tensor([1.0], dtype=torch.float64))
    m.z = Bernoulli.define_variable(prob_true=torch.as_tensor(d['prior']), shape=(K,))
    m.x = Normal.define_variable(mean=dot(reshape(m.z, (1, K)), torch.as_tensor(d['w'])), variance=m.v, shape=(1, N))
    q = Posterior(m)
    q.prob = Variable(shape=(K,), initial_value=torch.as_tensor(d['q0']))
    q[m.z].set_prior(Bernoulli(prob_true=q.prob))
    alg = cls(num_samples=num_samples, model=m, posterior=q, observed=[m.x], **kw)
    infr = GradBasedInference(inference_algorithm=alg, grad_loop=BatchInferenceLoop(), dtype=dtype)
    batch = (_dev(d['x'][None, :], dtype),)
    infr.initialize(x=batch[0])
    infr.params.raw(m.v).fill_(V_RAW)
    infr.params[q.prob] = _dev(d['q0'], dtype)
    if mock:
        q[m.z].factor._rand_gen = MockRandomGenerator(_dev(d['z'], dtype))
    return m, q, infr, batch


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('baseline', [None, 'loo'])
@pytest.mark.parametrize('rb', [False, True])
def test_bernoulli_latent_against_svi_and_the_restatement(rb, baseline, dtype):
    from mxfusion_amd.inference import ScoreFunctionInference, ScoreFunctionRBInference, StochasticVariationalInference
    m, q, infr, batch = bern_build(ScoreFunctionRBInference if rb else ScoreFunctionInference, dtype, baseline=baseline)
    loss, grads = run(infr, batch, [m.v, q.prob])
    ms, qs, infr_s, batch_s = bern_build(StochasticVariationalInference, dtype)
    loss_svi, grads_svi = run(infr_s, batch_s, [ms.v])
    f, want, mag = bern_restatement(dtype, baseline)
    if dtype == 'float64':
        assert abs(loss - loss_svi) <= R.F64_BAR * np.abs(f).mean(), (loss, loss_svi)
        assert abs(loss + f.mean()) <= R.F64_BAR * np.abs(f).mean()
    else:
        close_to_svi('loss', loss, loss_svi, dtype)
        R.assert_float32_formula_meets_the_bar(('bernoulli', baseline), [bern_restatement(dtype, baseline, torch.float32)[1]], [want])
    close_to_svi('model parameter', grads[0], grads_svi[0], dtype)
    R.assert_close(('posterior probabilities', rb, baseline), -grads[1], want, mag, dtype)


def test_rb_rejects_a_posterior_that_is_not_mean_field():
    from mxfusion_amd import Model, Variable, Posterior
    from mxfusion_amd.common.exceptions import InferenceError
    from mxfusion_amd.components.distributions import Normal
    from mxfusion_amd.components.variables.var_trans import PositiveTransformation
    from mxfusion_amd.inference import ScoreFunctionInference, ScoreFunctionRBInference
    m = Model()
    m.a = Normal.define_variable(mean=0., variance=1., shape=(1,))
    m.b = Normal.define_variable(mean=m.a, variance=1., shape=(1,))
    m.x = Normal.define_variable(mean=m.b, variance=1., shape=(1,))
    q = Posterior(m)
    q.ma, q.va = Variable(shape=(1,)), Variable(shape=(1,), transformation=PositiveTransformation())
    q.vb = Variable(shape=(1,), transformation=PositiveTransformation())
    q[m.a].set_prior(Normal(mean=q.ma, variance=q.va))
    q[m.b].set_prior(Normal(mean=q[m.a], variance=q.vb))            # q(b | a): not mean-field
    ScoreFunctionInference(num_samples=2, model=m, posterior=q, observed=[m.x])
    with pytest.raises(InferenceError):
        ScoreFunctionRBInference(num_samples=2, model=m, posterior=q, observed=[m.x])


def test_baseline_arguments():
    from mxfusion_amd.common.exceptions import InferenceError
    from mxfusion_amd.inference import ScoreFunctionInference, ScoreFunctionRBInference
    for cls in (ScoreFunctionInference, ScoreFunctionRBInference):
        with pytest.raises(InferenceError):
            bern_build(cls, 'float64', num_samples=1, baseline='loo')
        with pytest.raises(InferenceError):
            bern_build(cls, 'float64', baseline='mean')


# ---- statistical -------------------------------------------------------------------------------------------------------------------

def enumeration():
    """exact ELBO gradient w.r.t. the posterior probabilities, the per-component variance of f(z) d log q(z) / d prob, E f and std f"""
    d = bern_data('float64')
    qp = torch.as_tensor(d['q0'], dtype=torch.float64).requires_grad_(True)
    v = R.softplus(torch.as_tensor([V_RAW], dtype=torch.float64))
    Z = R.bernoulli_configs(K)
    f, lq = bern_f(Z, qp, d, v)
    exact = torch.autograd.grad((torch.exp(lq) * f).sum(), qp, retain_graph=True)[0].numpy()
    prob = torch.exp(lq).detach().numpy()
    score = np.stack([torch.autograd.grad(lq[c], qp, retain_graph=True)[0].numpy() for c in range(Z.shape[0])])      # (8, K)
    g = f.detach().numpy()[:, None] * score
    Eg = (prob[:, None] * g).sum(axis=0)
    var = (prob[:, None] * g ** 2).sum(axis=0) - Eg ** 2
    Ef = float((prob * f.detach().numpy()).sum())
    sf = float(np.sqrt((prob * (f.detach().numpy() - Ef) ** 2).sum()))
    return exact, Eg, var, Ef, sf


@pytest.mark.parametrize('baseline', [None, 'loo'])
def test_estimate_is_within_six_sigma_of_the_exact_gradient(baseline):
    from mxfusion_amd.inference import ScoreFunctionInference
    exact, Eg, var, Ef, sf = enumeration()
    assert np.abs(exact - Eg).max() <= 1e-12 * np.abs(exact).max()           # E[f grad log q] is the ELBO gradient (E[grad log q] = 0)
    assert abs(Ef) >= 3 * sf, (Ef, sf)
    S_big = 4096
    m, q, infr, batch = bern_build(ScoreFunctionInference, 'float64', num_samples=S_big, mock=False, baseline=baseline)
    torch.manual_seed(0)
    _, grads = run(infr, batch, [q.prob])
    est = -grads[0]
    sigma = np.sqrt(var / S_big)
    print('score-function estimate, baseline %s: %s exact %s, in sigmas %s' % (baseline, est, exact, (est - exact) / sigma))
    assert (np.abs(est - exact) <= 6 * sigma).all(), (est, exact, sigma)
