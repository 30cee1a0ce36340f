"""Operators on model variables (mxfusion/components/functions/operators/): only `broadcast_to`, which the priors of a Bayesian neural
network need (a prior Normal(0, 1) over a weight matrix is written with a one-element mean and variance broadcast to the weight's shape).
The other operators of the reference are not here."""
import numpy as np
import torch

from ..function_evaluation import FunctionEvaluation
from ...factor import Factor
from ...variables.variable import Variable
from ....util.inference import realize_shape


class BroadcastToOperator(FunctionEvaluation):
    """output = data broadcast to `shape` by the numpy rule, behind the sample axis: data (S|1, ...) -> (S|1,) + shape.  The result is a
    stride-0 view (`expand`), never a copy.  `shape` may hold symbolic dimensions (m.N)."""

    def __init__(self, data, shape):
        Factor.__init__(self, [('data', data)], [('output_0', Variable(shape=shape))], ['data'], ['output_0'])
        self.operator_name = 'broadcast_to'
        self.properties = {'shape': tuple(shape)}
        self.broadcastable = True

    def eval(self, F, variables, always_return_tuple=False):
        data = variables[self.inputs[0][1].uuid]
        shape = realize_shape(self.properties['shape'], variables)
        missing = len(shape) + 1 - data.dim()
        if missing > 0:
            data = data.reshape((data.shape[0],) + (1,) * missing + tuple(data.shape[1:]))
        out = data.expand((data.shape[0],) + shape)
        return (out,) if always_return_tuple else out


def broadcast_to(data, shape):
    """m.x = Normal.define_variable(mean=broadcast_to(torch.tensor([0.]), (2,)), variance=broadcast_to(torch.tensor([1.]), (2,)), shape=(2,))
    (operators/operator_impl.py).  data: a Variable, or a number / array, which becomes a constant."""
    if not isinstance(data, Variable):
        if not isinstance(data, (int, float, np.ndarray, torch.Tensor)):
            raise TypeError('broadcast_to: a Variable or an array is expected, not %s' % type(data).__name__)
        data = Variable(value=data, shape=tuple(np.shape(data)) or (1,))
    return BroadcastToOperator(data, shape).outputs[0][1]
