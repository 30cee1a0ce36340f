"""MXFusionTorchFunction, TorchFunctionEvaluation and broadcast_to: what can be checked while a model is put together, without a GPU."""
import numpy as np
import pytest
import torch


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(2, 5), torch.nn.Tanh(), torch.nn.Linear(5, 1))


def _model(**kw):
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.functions import MXFusionTorchFunction
    net = _net()
    m = Model()
    m.N = Variable()
    m.f = MXFusionTorchFunction(net, num_outputs=1, name='nn', **kw)
    m.x = Variable(shape=(m.N, 2))
    return m, net


def test_parameter_variables_follow_the_module():
    from mxfusion_amd.components.variables.variable import VariableType
    m, net = _model()
    assert m.f.parameter_names == ['nn_0_bias', 'nn_0_weight', 'nn_2_bias', 'nn_2_weight']
    assert sorted(m.f.parameters) == m.f.parameter_names
    for name, v in m.f.parameters.items():
        p = net.get_parameter(m.f.torch_name(name))
        assert v.shape == tuple(p.shape) and v.isInherited and v.inherited_name == name and v.type == VariableType.PARAMETER
        assert torch.equal(v.initial_value, p.detach()) and v.initial_value is not p
    assert m.f.output_names == ['nn_output_0'] and m.f.input_names is None
    m.r = m.f(m.x)
    assert m.f.input_names == ['nn_input_0'] + m.f.parameter_names
    fe = m.r.factor
    assert fe.input_names == m.f.input_names and fe.output_names == ['nn_output_0']
    assert fe.nn_input_0 is m.x and fe.nn_0_weight is m.f.parameters['nn_0_weight']
    assert fe.parameters == m.f.parameters and fe.broadcastable is False
    assert m.r.type == VariableType.FUNCVAR
    assert all(v.uuid in m for v in m.f.parameters.values())
    assert {v.uuid for v in m.get_parameters()} >= {v.uuid for v in m.f.parameters.values()}


def test_set_prior_makes_a_parameter_a_random_variable():
    from mxfusion_amd.components.distributions import Normal
    from mxfusion_amd.components.functions.operators import broadcast_to
    from mxfusion_amd.components.variables.variable import VariableType
    m, _ = _model()
    m.r = m.f(m.x)
    w = m.r.factor.parameters['nn_0_weight']
    prior = Normal(mean=broadcast_to(torch.tensor([0.]), w.shape), variance=broadcast_to(torch.tensor([1.]), w.shape))
    w.set_prior(prior)
    assert w.type == VariableType.RANDVAR and w.factor is prior
    assert any(f is prior for f in m._factors)
    assert prior.mean.uuid in m and prior.mean.factor.inputs[0][1].uuid in m
    assert w.uuid in {v.uuid for v in m.get_latent_variables([m.x])}
    assert m.r.factor.parameters['nn_0_bias'].type == VariableType.PARAMETER
    order = m.ordered_factors
    assert [f is prior for f in order].index(True) < [f is m.r.factor for f in order].index(True)


def test_keyword_overrides_a_parameter():
    from mxfusion_amd import Variable
    from mxfusion_amd.common.exceptions import ModelSpecificationError
    from mxfusion_amd.components.distributions import Normal
    m, _ = _model(broadcastable=True)
    m.w = Variable(shape=(5, 2))
    m.r = m.f(m.x, nn_0_weight=m.w)
    assert m.r.factor.nn_0_weight is m.w and m.r.factor.parameters['nn_0_weight'] is m.w
    assert m.r.factor.broadcastable is True                     # a free parameter: still one call
    m.b = Normal.define_variable(mean=0., variance=1., shape=(5,))
    m.r2 = m.f(m.x, nn_0_bias=m.b)
    assert m.r2.factor.nn_0_bias is m.b and m.r2.factor.broadcastable is False      # a random variable differs from sample to sample
    with pytest.raises(ModelSpecificationError):
        m.f(m.x, nn_9_weight=m.w)
    with pytest.raises(ModelSpecificationError):
        from mxfusion_amd.components.functions import MXFusionTorchFunction
        MXFusionTorchFunction(lambda x: x, num_outputs=1)


def test_broadcast_to_shapes():
    from mxfusion_amd import Model, Variable
    from mxfusion_amd.components.functions.operators import broadcast_to
    from mxfusion_amd.components.variables.variable import VariableType
    m = Model()
    m.N = Variable()
    m.v = Variable(shape=(1,))
    m.b = broadcast_to(m.v, (m.N, 3))
    assert m.b.type == VariableType.FUNCVAR and m.b.factor.inputs[0][1] is m.v
    variables = {m.v.uuid: torch.tensor([[2.0]]), m.N.uuid: 4}
    out = m.b.factor.eval(None, variables)
    assert tuple(out.shape) == (1, 4, 3) and out.stride() == (1, 0, 0) and float(out[0, 3, 2]) == 2.0
    variables[m.v.uuid] = torch.tensor([[1.0], [2.0]])          # two samples: the sample axis stays in front
    out = m.b.factor.eval(None, variables, always_return_tuple=True)[0]
    assert tuple(out.shape) == (2, 4, 3) and float(out[1, 0, 0]) == 2.0
    c = broadcast_to(np.array([0.5, 1.5]), (3, 2))
    const = c.factor.inputs[0][1]
    assert const.type == VariableType.CONSTANT
    out = c.factor.eval(None, {const.uuid: torch.as_tensor(const.constant)[None]})
    assert tuple(out.shape) == (1, 3, 2) and out[0, 2].tolist() == [0.5, 1.5]
    with pytest.raises(TypeError):
        broadcast_to('x', (2,))


def test_replicate_self_shares_the_module():
    m, net = _model()
    m.r = m.f(m.x)
    rep = m.f.replicate_self()
    assert rep is not m.f and rep.module is net and rep.name == 'nn' and rep.num_outputs == 1
    assert rep.parameter_names == m.f.parameter_names and rep.input_names == m.f.input_names and rep.output_names == m.f.output_names
    for k, v in m.f.parameters.items():
        r = rep.parameters[k]
        assert r is not v and r.uuid == v.uuid and r.shape == v.shape and r.isInherited and r.inherited_name == k and r.factor is None


def test_repr_and_clone():
    m, net = _model()
    m.r = m.f(m.x)
    line = [l for l in repr(m).splitlines() if 'TorchFunctionEvaluation' in l]
    assert len(line) == 1
    assert line[0].startswith('Variable(r, ') and ' = TorchFunctionEvaluation(nn_input_0=Variable(x, ' in line[0]
    for k in m.f.parameter_names:
        assert k + '=Variable(' in line[0]
    c = m.clone()
    assert c.r.factor is not m.r.factor and c.r.factor.uuid == m.r.factor.uuid
    assert c.r.factor.function.module is net and c.r.factor.broadcastable is False
    assert [k for k, _ in c.r.factor.inputs] == [k for k, _ in m.r.factor.inputs]
    assert all(a.uuid == b.uuid and a is not b for (_, a), (_, b) in zip(c.r.factor.inputs, m.r.factor.inputs))


def test_gluon_aliases_and_the_qualifying_rule():
    from mxfusion_amd.components import functions
    from mxfusion_amd.components.functions.torch_function import dense_plan
    assert functions.MXFusionGluonFunction is functions.MXFusionTorchFunction
    assert functions.GluonFunctionEvaluation is functions.TorchFunctionEvaluation
    L, Seq = torch.nn.Linear, torch.nn.Sequential
    assert dense_plan(_net()) == [('0', True, 1), ('2', True, 0)]
    assert dense_plan(Seq(torch.nn.Flatten(), L(3, 4, bias=False), torch.nn.Identity(), torch.nn.ReLU(), L(4, 2), torch.nn.Sigmoid())) == [('1', False, 2), ('4', True, 3)]
    assert dense_plan(Seq(L(3, 4), torch.nn.Softsign(), L(4, 2))) is None          # an unsupported layer
    assert dense_plan(Seq(torch.nn.Tanh(), L(3, 4))) is None                        # an activation with no Linear in front
    assert dense_plan(Seq(L(3, 4), torch.nn.Tanh(), torch.nn.Tanh())) is None
    assert dense_plan(Seq(L(3, 129), L(129, 1))) is None                            # beyond the kernel's widths
    assert dense_plan(Seq(L(128, 128))) == [('0', True, 0)]
    assert dense_plan(L(3, 4)) is None and dense_plan(Seq()) is None
