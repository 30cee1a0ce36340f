"""Operators on model variables (mxfusion/components/functions/operators/operators.py and operator_impl.py): `m.mean = dot(m.x, m.w) + m.b`,
`m.var = exp(m.log_var)`.  The reference's sixteen: add, subtract, multiply, divide, power; square, exp, log; sum, mean, prod; dot, diag;
reshape, transpose; broadcast_to.  Variable's `+ - * / **` build the first five.

What an operator computes is what the reference's per-sample loop computes (function_evaluation.py:72-96): the operator applied to each
sample without its sample axis, the results stacked -- so `axis`, `axes` and `shape` refer to the per-sample array.  How it computes it
differs: every operator here takes all samples at once.  By default (FUSED_OPERATORS below) the arithmetic, elementwise and reduction
operators evaluate the torch expression on the device.  Their HIP path is one launch of the broadcast map (ops.ewise, reverse mode
ops.ewise_bwd_: the gradient of an operand that is shared over the samples or broadcast over rows -- a bias, a scale, any parameter that is
not a random variable -- is summed over its shared axes in double inside that launch) and ops.reduce / ops.reduce_bwd_ for sum, mean and
prod.  dot is the batched GEMM, diag the diagonal kernels; reshape and transpose are views, broadcast_to a stride-0
view that the map reads without materialising it.  Only device tensors are taken: there is no CPU path for the operators that compute.

FUSED_OPERATORS chooses, for the arithmetic, elementwise and reduction operators, between those HIP entry points (True) and the plain
torch expression on the device (False).  It is False: at every shape measured -- a bias add, a same-shape multiply and a last-axis sum, each at a likelihood's size (32, 8192,
64) and at a prior's (3, 50, 50), float32 and float64 -- forward plus reverse through the HIP path took 1.2 to 3.4
times as long as torch's: the large shapes pay for a zero fill and a read-modify-write of every gradient, the small ones for launches and
host work.  Shapes between those two sizes, and the other ops, were not measured and follow the same default.  A map of more than five axes after merging goes through torch in any case.  ops.ewise and
ops.reduce are the HIP path whatever this says."""
import numpy as np
import torch

from .... import ops
from ....common.exceptions import ModelSpecificationError
from ....util.customop import make_diagonal
from ....util.inference import realize_shape
from ...distributions._fused import carved_grads
from ...distributions.gp._linalg import matmul
from ...factor import Factor
from ...variables.variable import Variable
from ..function_evaluation import FunctionEvaluation

# The HIP map and reductions against the torch expressions they replace: DESIGN.md section 9 holds the measurement behind this default
# (HIP slower at every shape measured).
FUSED_OPERATORS = False


class Operator(FunctionEvaluation):
    """A function evaluation that is one named operator (operators.py:21-50): `operator_name`, and `properties` -- the arguments that are
    not variables (an axis, a shape).  A subclass implements eval, or eval_impl(F, **inputs and properties), on arrays that carry the
    sample axis."""

    def __init__(self, inputs, outputs, operator_name, properties=None, broadcastable=False):
        Factor.__init__(self, inputs, outputs, [n for n, _ in inputs], [n for n, _ in outputs])
        self.operator_name = operator_name
        self.properties = dict(properties or {})
        self.broadcastable = broadcastable

    def __repr__(self):
        return '%s(%s)' % (self.__dict__.get('operator_name', type(self).__name__),
                           ', '.join('%s=%s' % (n, v) for n, v in self.__dict__.get('_inputs') or []))

    def eval(self, F, variables, always_return_tuple=False):
        kws = {n: variables[v.uuid] for n, v in self.inputs}
        for k, p in self.properties.items():
            kws[k] = realize_shape(p, variables) if k == 'shape' and p is not None else p
        out = self.eval_impl(F, **kws)
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        return out if always_return_tuple or len(out) > 1 else out[0]

    def eval_impl(self, F, **kws):
        raise NotImplementedError


class CustomOperator(Operator):
    """the operator an OperatorDecorator makes of a function (under the class name the reference's saved graphs carry)"""

    def __init__(self, func, **kws):
        Operator.__init__(self, **kws)
        self._func = func

    def eval_impl(self, F, **kws):
        return self._func(F, **kws)


def _as_variable(what, data):
    """a number or an array on an operator's input becomes a constant Variable, as in broadcast_to"""
    if isinstance(data, Variable):
        return data
    if isinstance(data, bool) or not isinstance(data, (int, float, np.ndarray, torch.Tensor)):
        raise TypeError('%s: a Variable, a number or an array is expected, not %s' % (what, type(data).__name__))
    return Variable(value=data, shape=tuple(np.shape(data)) or (1,))


class OperatorDecorator(object):
    """@OperatorDecorator(name='add', args=['x', 'y'], inputs=['x', 'y']) over `def add(F, x, y)` gives `add(m.a, m.b)`, which puts an
    Operator into the graph and returns its output Variable (operators.py:53-108).  args: the function's argument names in order; inputs:
    those that are variables; the others become the operator's properties.  Unlike the reference's, the function receives and returns
    arrays that carry the sample axis (S|1, ...), as every function here does, and is called once for all samples."""

    def __init__(self, name, args, inputs, num_outputs=1, broadcastable=False):
        self.operator_name = name
        self.arg_names = list(args)
        self.input_names = list(inputs)
        self.property_names = [v for v in args if v not in inputs]
        self.num_outputs = num_outputs
        self.broadcastable = broadcastable

    def _parse_arguments(self, args, kwargs):
        free = [v for v in self.arg_names if v not in kwargs]
        arguments = dict(kwargs)
        arguments.update(zip(free, args))
        return arguments

    def __call__(self, func):
        def create_operator(*args, **kwargs):
            given = self._parse_arguments(args, kwargs)
            if any(n not in given for n in self.input_names):
                raise ModelSpecificationError('Must pass in arguments matching the input names %s but received %s.'
                                              % (self.input_names, sorted(given)))
            op = CustomOperator(func, inputs=[(n, _as_variable(self.operator_name, given[n])) for n in self.input_names],
                                outputs=[('output_%d' % i, Variable(shape=None)) for i in range(self.num_outputs)],
                                operator_name=self.operator_name, properties={n: given[n] for n in self.property_names if n in given},
                                broadcastable=self.broadcastable)
            outs = [v for _, v in op.outputs]
            return outs[0] if self.num_outputs == 1 else tuple(outs)
        create_operator.__name__ = self.operator_name
        create_operator.__doc__ = func.__doc__
        return create_operator


MXNetOperatorDecorator = OperatorDecorator      # the reference's name


# ---- the autograd functions over ops.ewise / ops.reduce ----------------------------------------------------------------------------------

class _EwiseFn(torch.autograd.Function):
    """z = op(x, y) for all samples: ops.ewise forward, ops.ewise_bwd_ reverse.  x and y are ewise_operands' (one rank, no expanded axis),
    so a gradient has its operand's shape: a shared axis stays at extent 1 and its sum is formed inside the launch."""

    @staticmethod
    def forward(ctx, op, x, y):
        ctx.op = op
        ctx.save_for_backward(x, y)
        return ops.ewise(op, x, y)

    @staticmethod
    def backward(ctx, dz):
        x, y = ctx.saved_tensors
        need = [ctx.needs_input_grad[1], y is not None and ctx.needs_input_grad[2]]
        grads = carved_grads((x.shape, () if y is None else y.shape), need, dz)
        if any(g is not None for g in grads):
            ops.ewise_bwd_(ctx.op, x, y, dz.contiguous(), *grads)
        return None, grads[0], grads[1]


class _ReduceFn(torch.autograd.Function):
    """sum / mean / prod over per-sample axes for all samples: ops.reduce forward, ops.reduce_bwd_ reverse"""

    @staticmethod
    def forward(ctx, kind, x, axes):
        ctx.kind, ctx.axes = kind, axes
        ctx.save_for_backward(x)
        return ops.reduce(kind, x, axes)

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dx, = carved_grads((x.shape,), (True,), dy)
        ops.reduce_bwd_(ctx.kind, x, ctx.axes, dy.contiguous(), dx)
        return None, dx, None


class _DiagOfFn(torch.autograd.Function):
    """(..., n, n) -> (..., n): ops.diag_of, with ops.make_diagonal as its reverse"""

    @staticmethod
    def forward(ctx, a):
        return ops.diag_of(a)

    @staticmethod
    def backward(ctx, g):
        return ops.make_diagonal(g.contiguous())


def _floating(*ts):
    return all(t is None or t.dtype == ts[0].dtype for t in ts) and ts[0].dtype in (torch.float32, torch.float64)


def _ewise(op, x, y=None):
    ops._require_gpu(x)
    if y is not None:
        ops._require_gpu(y)
    x, y = ops.ewise_operands(x, y)
    if FUSED_OPERATORS and _floating(x, y) and ops.ewise_fits(x, y):
        return _EwiseFn.apply(op, x, y)
    return ops._EW_TORCH[ops.EW_OP[op]](x, y) if y is not None else ops._EW_TORCH[ops.EW_OP[op]](x)


def _axes_of(axis):
    return None if axis is None else ((int(axis),) if isinstance(axis, (int, np.integer)) else tuple(int(a) for a in axis))


def _reduce(kind, data, axis):
    ops._require_gpu(data)
    axes = _axes_of(axis)
    if FUSED_OPERATORS and _floating(data):
        return _ReduceFn.apply(kind, data, axes)
    if axes is None:
        return getattr(torch, kind)(data.reshape(data.shape[0], -1), 1, keepdim=True)
    nd = data.dim() - 1
    for a in sorted((a + nd if a < 0 else a for a in axes), reverse=True):
        data = getattr(torch, kind)(data, a + 1)
    return data


def _unexpand(t):
    return ops._shared_axes(t, (0,), None)[0]


# ---- the sixteen (operator_impl.py:27-169) ---------------------------------------------------------------------------------------------

@OperatorDecorator(name='add', args=['x', 'y'], inputs=['x', 'y'])
def add(F, x, y):
    """x + y, broadcast by the numpy rule behind the sample axis"""
    return _ewise('add', x, y)


@OperatorDecorator(name='subtract', args=['x', 'y'], inputs=['x', 'y'])
def subtract(F, x, y):
    """x - y"""
    return _ewise('subtract', x, y)


@OperatorDecorator(name='multiply', args=['x', 'y'], inputs=['x', 'y'])
def multiply(F, x, y):
    """x * y"""
    return _ewise('multiply', x, y)


@OperatorDecorator(name='divide', args=['x', 'y'], inputs=['x', 'y'])
def divide(F, x, y):
    """x / y"""
    return _ewise('divide', x, y)


@OperatorDecorator(name='power', args=['x', 'y'], inputs=['x', 'y'])
def power(F, x, y):
    """x ** y; the gradient of y needs x > 0"""
    return _ewise('power', x, y)


@OperatorDecorator(name='square', args=['data'], inputs=['data'])
def square(F, data):
    return _ewise('square', data)


@OperatorDecorator(name='exp', args=['data'], inputs=['data'])
def exp(F, data):
    return _ewise('exp', data)


@OperatorDecorator(name='log', args=['data'], inputs=['data'])
def log(F, data):
    return _ewise('log', data)


@OperatorDecorator(name='sum', args=['data', 'axis'], inputs=['data'])
def sum(F, data, axis=None):
    """over the per-sample axis or axes `axis`, which are dropped; axis=None: over all of them, giving (S, 1)"""
    return _reduce('sum', data, axis)


@OperatorDecorator(name='mean', args=['data', 'axis'], inputs=['data'])
def mean(F, data, axis=None):
    """as sum"""
    return _reduce('mean', data, axis)


@OperatorDecorator(name='prod', args=['data', 'axis'], inputs=['data'])
def prod(F, data, axis=None):
    """as sum"""
    return _reduce('prod', data, axis)


@OperatorDecorator(name='dot', args=['x', 'y'], inputs=['x', 'y'])
def dot(F, x, y):
    """linalg.gemm2 on the last two axes: (S|1, m, k) . (S|1, k, n) -> (S, m, n), the batched GEMM with its reverse mode"""
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != y.shape[1]:
        raise ValueError('dot: per-sample matrices (m, k) and (k, n) are expected, got %s and %s' % (tuple(x.shape[1:]), tuple(y.shape[1:])))
    return matmul(_unexpand(x), _unexpand(y))


@OperatorDecorator(name='diag', args=['data', 'k', 'axis1', 'axis2'], inputs=['data'])
def diag(F, data, k=0, axis1=None, axis2=None):
    """a per-sample vector -> the diagonal matrix; a per-sample square matrix -> its diagonal.  Only k = 0."""
    if axis1 is not None or axis2 is not None:
        raise NotImplementedError('diag: axis1 and axis2 are not implemented yet.')
    if k != 0:
        raise NotImplementedError('diag: only the main diagonal (k = 0) is implemented, got k = %r' % (k,))
    if data.dim() == 2:
        return make_diagonal(F, data)
    if data.dim() == 3 and data.shape[1] == data.shape[2]:
        return _DiagOfFn.apply(data)
    raise ValueError('diag: a per-sample vector or square matrix is expected, got %s' % (tuple(data.shape[1:]),))


@OperatorDecorator(name='reshape', args=['data', 'shape', 'reverse'], inputs=['data'])
def reshape(F, data, shape, reverse=False):
    """to the per-sample `shape` (one -1 allowed); a view where the layout allows"""
    if reverse or any(s in (0, -2, -3, -4) for s in shape):
        raise NotImplementedError("reshape: MXNet's special shape codes 0, -2, -3, -4 and reverse=True are not implemented; give the plain "
                                  'per-sample shape (one -1 is allowed)')
    return data.reshape((data.shape[0],) + tuple(shape))


@OperatorDecorator(name='transpose', args=['data', 'axes'], inputs=['data'])
def transpose(F, data, axes=None):
    """permutes the per-sample axes; axes=None (or empty) reverses them.  A view."""
    nd = data.dim() - 1
    axes = tuple(range(nd - 1, -1, -1)) if axes is None or len(axes) == 0 else tuple(int(a) for a in axes)
    return data.permute((0,) + tuple(a + 1 if a >= 0 else a + nd + 1 for a in axes))


class BroadcastToOperator(Operator):
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
