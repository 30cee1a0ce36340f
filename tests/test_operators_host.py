"""The model operators and Variable arithmetic without a GPU: what each operator puts into the graph, that a model holding one survives clone
and extract_distribution_of, that the operators that compute refuse CPU tensors (there is no CPU path) and that the shape-only ones give
the per-sample result."""
import numpy as np
import pytest
import torch

from mxfusion_amd import Model, Variable
from mxfusion_amd._lib import MXFError
from mxfusion_amd.common.exceptions import ModelSpecificationError
from mxfusion_amd.components.functions import operators as O
from mxfusion_amd.components.functions.operators import Operator

BINARY = ['add', 'subtract', 'multiply', 'divide', 'power', 'dot']
UNARY = ['square', 'exp', 'log']
ALL = BINARY + UNARY + ['sum', 'mean', 'prod', 'diag', 'reshape', 'transpose', 'broadcast_to']


def test_the_package_exports_the_sixteen_operators():
    assert len(ALL) == 16
    for name in ALL:
        assert callable(getattr(O, name)), name
    assert O.MXNetOperatorDecorator is O.OperatorDecorator


@pytest.mark.parametrize('name', BINARY)
def test_binary_operator_factor(name):
    a, b = Variable(shape=(3, 2)), Variable(shape=(2, 3))
    out = getattr(O, name)(a, b)
    f = out.factor
    assert isinstance(out, Variable) and isinstance(f, Operator)
    assert f.operator_name == name and f.properties == {}
    assert [(n, v.uuid) for n, v in f.inputs] == [('x', a.uuid), ('y', b.uuid)]
    assert [n for n, _ in f.outputs] == ['output_0'] and f.outputs[0][1] is out


@pytest.mark.parametrize('name', UNARY)
def test_elementwise_operator_factor(name):
    a = Variable(shape=(3, 2))
    f = getattr(O, name)(a).factor
    assert isinstance(f, Operator) and f.operator_name == name and f.properties == {}
    assert [(n, v.uuid) for n, v in f.inputs] == [('data', a.uuid)]


def test_operators_with_properties():
    a = Variable(shape=(3, 2))
    for name in ('sum', 'mean', 'prod'):
        f = getattr(O, name)(a, axis=1).factor
        assert (f.operator_name, f.properties, [n for n, _ in f.inputs]) == (name, {'axis': 1}, ['data'])
        assert getattr(O, name)(a).factor.properties == {}
        assert getattr(O, name)(a, (0, 1)).factor.properties == {'axis': (0, 1)}
    f = O.diag(a, k=0).factor
    assert (f.operator_name, f.properties) == ('diag', {'k': 0})
    f = O.reshape(a, (2, 3)).factor
    assert (f.operator_name, f.properties, [n for n, _ in f.inputs]) == ('reshape', {'shape': (2, 3)}, ['data'])
    f = O.reshape(data=a, shape=(6,), reverse=False).factor
    assert f.properties == {'shape': (6,), 'reverse': False}
    f = O.transpose(a, axes=(1, 0)).factor
    assert (f.operator_name, f.properties) == ('transpose', {'axes': (1, 0)})
    f = O.broadcast_to(a, (4, 3, 2)).factor
    assert isinstance(f, Operator) and (f.operator_name, f.properties) == ('broadcast_to', {'shape': (4, 3, 2)})
    assert [n for n, _ in f.inputs] == ['data']


def test_missing_inputs_raise():
    with pytest.raises(ModelSpecificationError):
        O.add()
    with pytest.raises(ModelSpecificationError):
        O.reshape()
    with pytest.raises(ModelSpecificationError):
        O.add(Variable())
    with pytest.raises(ModelSpecificationError):
        O.reshape(shape=(2,))


def test_variable_arithmetic_builds_the_named_operators():
    v1, v2 = Variable(shape=(3,)), Variable(shape=(3,))
    for expr, name in ((lambda: v1 + v2, 'add'), (lambda: v1 - v2, 'subtract'), (lambda: v1 * v2, 'multiply'), (lambda: v1 / v2, 'divide'),
                       (lambda: v1 ** v2, 'power')):
        f, named = expr().factor, getattr(O, name)(v1, v2).factor
        assert type(f) is type(named) and f.operator_name == name and f.properties == named.properties
        assert [(n, v.uuid) for n, v in f.inputs] == [('x', v1.uuid), ('y', v2.uuid)]
    f = (2 * v1).factor
    assert type(f) is type(O.multiply(v1, v2).factor) and f.operator_name == 'multiply' and f.properties == {}
    assert f.inputs[1][1] is v1 and f.inputs[0][1].isConstant and f.inputs[0][1].constant == 2
    f = (v1 + 1.0).factor
    assert type(f) is type(O.add(v1, v2).factor) and f.operator_name == 'add' and f.properties == {}
    assert f.inputs[0][1] is v1 and f.inputs[1][1].isConstant and f.inputs[1][1].constant == 1.0 and f.inputs[1][1].shape == (1,)
    for expr, name in ((lambda: 1.0 - v1, 'subtract'), (lambda: 1.0 / v1, 'divide'), (lambda: 2.0 ** v1, 'power'), (lambda: 1 + v1, 'add')):
        f = expr().factor
        assert f.operator_name == name and f.inputs[1][1] is v1 and f.inputs[0][1].isConstant
    f = (v1 * np.array([1.0, 2.0, 3.0])).factor
    assert f.inputs[1][1].isConstant and f.inputs[1][1].shape == (3,)
    f = (np.array([1.0, 2.0, 3.0]) * v1).factor               # the array on the left reaches the reflected form as a whole
    assert f.operator_name == 'multiply' and f.inputs[1][1] is v1 and f.inputs[0][1].isConstant and f.inputs[0][1].shape == (3,)
    f = (np.array([1.0, 2.0, 3.0]) - v1).factor
    assert f.operator_name == 'subtract' and f.inputs[1][1] is v1 and f.inputs[0][1].shape == (3,)
    f = (np.float64(2.0) ** v1).factor
    assert f.operator_name == 'power' and f.inputs[1][1] is v1 and f.inputs[0][1].isConstant
    with pytest.raises(TypeError):
        v1 + 'a'
    assert v1 == v1 and v1 != v2 and hash(v1) == hash(v1.uuid) and len({v1, v2, v1}) == 2      # __eq__ and __hash__ stay


def _model():
    from mxfusion_amd.components.distributions import Normal
    m = Model()
    m.N = Variable()
    m.x = Variable(shape=(m.N, 2))
    m.w = Variable(shape=(2, 1))
    m.b = Variable(shape=(1,))
    m.log_s = Variable(shape=(1,))
    m.s = O.exp(m.log_s)
    m.y = Normal.define_variable(mean=O.dot(m.x, m.w) + m.b, variance=O.broadcast_to(m.s * m.s, (m.N, 1)), shape=(m.N, 1))
    return m


def _operator_names(factors):
    return sorted(f.operator_name for f in factors if isinstance(f, Operator))


def test_a_model_with_operators_survives_clone():
    m = _model()
    want = ['add', 'broadcast_to', 'dot', 'exp', 'multiply']
    assert _operator_names(m._factors) == want
    c = m.clone()
    assert _operator_names(c._factors) == want
    mean = c.y.factor.mean
    assert mean.uuid == m.y.factor.mean.uuid and mean is not m.y.factor.mean
    f = mean.factor
    assert isinstance(f, Operator) and f is not m.y.factor.mean.factor and (f.operator_name, f.properties) == ('add', {})
    assert f.inputs[0][1].factor.operator_name == 'dot' and f.inputs[1][1].uuid == m.b.uuid
    assert c.y.factor.variance.factor.properties['shape'][0].uuid == m.N.uuid
    assert ' = exp(data=' in repr(c) and ' = dot(x=' in repr(c)


def test_a_model_with_operators_survives_extract_distribution_of():
    m = _model()
    y = m.extract_distribution_of(m.y)
    assert y is not m.y and y.uuid == m.y.uuid and y.graph is None
    mean = y.factor.mean
    assert mean.factor.operator_name == 'add' and mean.factor is not m.y.factor.mean.factor
    assert mean.factor.inputs[0][1].factor.operator_name == 'dot'
    assert [v.uuid for _, v in mean.factor.inputs[0][1].factor.inputs] == [m.x.uuid, m.w.uuid]
    var = y.factor.variance.factor
    assert var.operator_name == 'broadcast_to' and var.inputs[0][1].factor.operator_name == 'multiply'
    assert var.inputs[0][1].factor.inputs[0][1].factor.operator_name == 'exp'
    assert m.y.graph is m and m.y.factor.mean.graph is m     # the model itself is left as it was


def _eval(var, *arrays):
    f = var.factor
    return f.eval(torch, {v.uuid: a for (_, v), a in zip(f.inputs, arrays)})


@pytest.mark.parametrize('name', ['add', 'subtract', 'multiply', 'divide', 'power', 'square', 'exp', 'log', 'sum', 'mean', 'prod'])
def test_computing_operators_refuse_cpu_tensors(name):
    a, b = Variable(shape=(3, 2)), Variable(shape=(3, 2))
    x = torch.rand(2, 3, 2, dtype=torch.float64) + 0.5
    with pytest.raises(MXFError):
        if name in BINARY:
            _eval(getattr(O, name)(a, b), x, x)
        else:
            _eval(getattr(O, name)(a), x)


def test_shape_only_operators_give_the_per_sample_result_on_cpu():
    r = np.random.RandomState(0)
    x = r.randn(3, 2, 4, 5)
    a = Variable(shape=(2, 4, 5))
    t = torch.as_tensor(x)
    cases = [(O.reshape(a, (8, 5)), lambda s: s.reshape(8, 5)), (O.reshape(a, (-1, 10)), lambda s: s.reshape(-1, 10)),
             (O.reshape(a, shape=(40,)), lambda s: s.reshape(40)), (O.transpose(a), lambda s: s.transpose()),
             (O.transpose(a, axes=(1, 0, 2)), lambda s: s.transpose(1, 0, 2)), (O.transpose(a, axes=(2, 0, 1)), lambda s: s.transpose(2, 0, 1)),
             (O.transpose(a, axes=[]), lambda s: s.transpose())]
    for var, per_sample in cases:
        got = _eval(var, t)
        want = np.stack([per_sample(x[s]) for s in range(3)])
        assert tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want), var.factor
    got = var.factor.eval(torch, {a.uuid: t}, always_return_tuple=True)
    assert isinstance(got, tuple) and len(got) == 1
    for bad in (O.reshape(a, (0, -1)), O.reshape(a, (-2,)), O.reshape(a, (-3, 5)), O.reshape(a, (-4, 1, 2, -2)), O.reshape(a, (8, 5), reverse=True)):
        with pytest.raises(NotImplementedError, match='not implemented'):
            _eval(bad, t)
    for bad in (O.diag(a, k=1), O.diag(a, axis1=0), O.diag(a, axis2=1)):
        with pytest.raises(NotImplementedError):
            _eval(bad, t)


def test_a_decorated_function_becomes_an_operator():
    @O.MXNetOperatorDecorator(name='shift', args=['data', 'by'], inputs=['data'])
    def shift(F, data, by=1.0):
        return data + by
    a = Variable(shape=(2,))
    f = shift(a, by=2.5).factor
    assert (f.operator_name, f.properties) == ('shift', {'by': 2.5})
    t = torch.zeros(3, 2)
    assert torch.equal(_eval(shift(a, by=2.5), t), t + 2.5) and torch.equal(_eval(shift(a), t), t + 1.0)
    m = Model()
    m.a = a
    m.c = shift(m.a, 3.0)
    assert m.clone().c.factor.properties == {'by': 3.0}
