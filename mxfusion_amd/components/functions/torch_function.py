"""A neural network inside a model (mxfusion/components/functions/mxfusion_gluon_function.py, gluon_func_eval.py and the `broadcastable`
switch of function_evaluation.py:47-99): MXFusionTorchFunction wraps a torch.nn.Module, exposes each of its parameters as a model
Variable -- a free parameter, or a random variable once it is given a prior: a Bayesian neural network -- and its call puts a
TorchFunctionEvaluation into the graph.

Evaluation with S samples of the weights.  The reference evaluates the block once per sample in a Python loop and concatenates.  Here a
module that is a torch.nn.Sequential of Linear / Tanh / ReLU / Sigmoid / Identity / Flatten layers of widths 1 .. 128 takes all samples
through the fused HIP dense layer (ops.dense: one launch per Linear, bias and activation fused, reverse mode ops.dense_bwd_); every other
module is evaluated per sample through torch.func.functional_call -- the parameters are passed in, never written into the module."""
import copy

import torch

from ... import _lib, ops
from ..distributions._fused import carved_grads
from ..factor import Factor
from ..variables.variable import Variable, VariableType
from .function_evaluation import FunctionEvaluation

# The fused dense layer against the per-sample loop it replaces: DESIGN.md section 12 holds the measurement behind this default.
FUSED_DENSE = True

_ACTIVATIONS = {torch.nn.Tanh: _lib.ACT_TANH, torch.nn.ReLU: _lib.ACT_RELU, torch.nn.Sigmoid: _lib.ACT_SIGMOID}


def dense_plan(module):
    """[(name of a Linear child, has bias, activation code)] when `module` qualifies for the fused dense path, else None.  The rule: a
    torch.nn.Sequential that holds only Linear, Tanh, ReLU, Sigmoid, Identity and Flatten (with its default axes: the identity on the
    (N, I) rows a Linear takes) layers, at least one Linear, every activation directly behind a Linear (Identity and Flatten aside), and
    every width within the kernel's 1 .. 128."""
    if type(module) is not torch.nn.Sequential:
        return None
    plan = []
    fused = True          # no Linear is waiting for an activation
    for name, layer in module.named_children():
        kind = type(layer)
        if kind is torch.nn.Linear:
            if not (1 <= layer.in_features <= _lib.DENSE_MAX_WIDTH and 1 <= layer.out_features <= _lib.DENSE_MAX_WIDTH):
                return None
            plan.append([name, layer.bias is not None, _lib.ACT_IDENTITY])
            fused = False
        elif kind in _ACTIVATIONS:
            if fused:
                return None
            plan[-1][2] = _ACTIVATIONS[kind]
            fused = True
        elif kind is torch.nn.Identity or (kind is torch.nn.Flatten and layer.start_dim == 1 and layer.end_dim == -1):
            continue
        else:
            return None
    return [tuple(p) for p in plan] or None


class _DenseFn(torch.autograd.Function):
    """One Linear and the activation behind it for all samples: ops.dense forward, ops.dense_bwd_ reverse."""

    @staticmethod
    def forward(ctx, X, W, b, act):
        Y = ops.dense(X, W, b, act)
        ctx.save_for_backward(X, W, Y)
        ctx.act, ctx.b_shape = act, None if b is None else tuple(b.shape)
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, W, Y = ctx.saved_tensors
        need = [w and s is not None for w, s in zip(ctx.needs_input_grad, (X.shape, W.shape, ctx.b_shape))]
        grads = carved_grads((X.shape, W.shape, ctx.b_shape or ()), need, Y)
        if any(g is not None for g in grads):
            ops.dense_bwd_(X, W, Y, dY.contiguous(), ctx.act, *grads)
        return grads[0], grads[1], grads[2], None


def _unexpand(t):
    """an operand whose sample axis is expanded (stride 0) as its one shared block"""
    return ops._shared_axes(t, (0,), None)[0]


class TorchFunctionEvaluation(FunctionEvaluation):
    """The evaluation of a MXFusionTorchFunction on given input variables; its inputs are those variables followed by the function's
    parameter variables under their names (gluon_func_eval.py, function_evaluation.py:117-169)."""

    def __init__(self, func, input_variables, output_variables, broadcastable=False):
        given = {k for k, _ in input_variables}
        inputs = list(input_variables) + [(k, func.parameters[k]) for k in func.parameter_names if k not in given]
        Factor.__init__(self, inputs, output_variables, [k for k, _ in inputs], [k for k, _ in output_variables])
        self._func = func
        self.broadcastable = broadcastable

    @property
    def function(self):
        return self._func

    @property
    def parameters(self):
        """{parameter name: the Variable this evaluation takes it from}: the function's own, or the caller's override."""
        names = set(self._func.parameter_names)
        return {k: v for k, v in self.inputs if k in names}

    def _split(self, variables):
        names = set(self._func.parameter_names)
        args = [variables[v.uuid] for k, v in self.inputs if k not in names]
        params = {self._func.torch_name(k): variables[v.uuid] for k, v in self.inputs if k in names}
        return args, params

    def eval(self, F, variables, always_return_tuple=False):
        args, params = self._split(variables)
        module = self._func.module
        S = max(t.shape[0] for t in args + list(params.values()))
        if self.broadcastable:
            S = max([t.shape[0] for t in args] + [1])
            out = torch.func.functional_call(module, {k: v[0] for k, v in params.items()}, tuple(a.expand((S,) + tuple(a.shape[1:])) for a in args))
        elif self._fused(args, params):
            out = self._eval_fused(args[0], params)
        else:
            pick = lambda t, s: t[s] if t.shape[0] > 1 else t[0]
            per = [torch.func.functional_call(module, {k: pick(v, s) for k, v in params.items()}, tuple(pick(a, s) for a in args))
                   for s in range(S)]
            if isinstance(per[0], (tuple, list)):
                out = tuple(torch.stack([p[i] for p in per], 0) for i in range(len(per[0])))
            else:
                out = torch.stack(per, 0)
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        return out if always_return_tuple or len(out) > 1 else out[0]

    def _fused(self, args, params):
        return (FUSED_DENSE and self._func.plan is not None and len(args) == 1 and args[0].dim() == 3 and args[0].is_cuda
                and args[0].dtype in (torch.float32, torch.float64) and all(p.dtype == args[0].dtype for p in params.values()))

    def _eval_fused(self, x, params):
        x = _unexpand(x)
        for name, has_bias, act in self._func.plan:
            W = _unexpand(params[name + '.weight'])
            b = _unexpand(params[name + '.bias']) if has_bias else None
            x = _DenseFn.apply(x, W, b, act)
        return x


class MXFusionTorchFunction(object):
    """m.f = MXFusionTorchFunction(net, num_outputs=1); m.r = m.f(m.x); then, for a Bayesian neural network,
    `for v in m.r.factor.parameters.values(): v.set_prior(Normal(...))`.  One inherited parameter Variable per entry of
    module.named_parameters(), named `<name>_<parameter name with '.' -> '_'>`, shaped and initialised like the parameter.
    `broadcastable`: the module maps inputs with a leading sample axis by itself (one call, the parameters at their first sample)."""

    def __init__(self, module, num_outputs, name=None, dtype=None, broadcastable=False):
        from ...common.exceptions import ModelSpecificationError
        if not isinstance(module, torch.nn.Module):
            raise ModelSpecificationError('The module argument must be a torch.nn.Module.')
        self._module = module
        self.name = name if name is not None else type(module).__name__.lower()
        self.num_outputs = num_outputs
        self.dtype = dtype
        self.broadcastable = broadcastable
        self._torch_names = {self.name + '_' + n.replace('.', '_'): n for n, _ in module.named_parameters()}
        self._parameters = {}
        for pname, n in self._torch_names.items():
            p = module.get_parameter(n)
            v = Variable(shape=tuple(p.shape), isInherited=True, initial_value=p.detach().clone())
            v.inherited_name = pname
            self._parameters[pname] = v
        self._parameter_names = sorted(self._parameters)
        self._input_variable_names = None
        self._input_names = None
        self._output_names = ['%s_output_%d' % (self.name, i) for i in range(num_outputs)]
        self.plan = dense_plan(module)

    @property
    def module(self):
        return self._module

    @property
    def parameters(self):
        return self._parameters

    @property
    def parameter_names(self):
        return self._parameter_names

    @property
    def input_names(self):
        """the inputs of the last call followed by the parameters; None before the first call"""
        return self._input_names

    @property
    def output_names(self):
        return self._output_names

    def torch_name(self, parameter_name):
        return self._torch_names[parameter_name]

    def __call__(self, *args, **kwargs):
        from ...common.exceptions import ModelSpecificationError
        unknown = [k for k in kwargs if k not in self._parameters]
        if unknown:
            raise ModelSpecificationError('%s has no parameter named %s' % (self.name, ', '.join(unknown)))
        self._input_variable_names = ['%s_input_%d' % (self.name, i) for i in range(len(args))]
        self._input_names = self._input_variable_names + self._parameter_names
        # a parameter that is a random or a function variable differs from sample to sample: one call cannot take it
        broadcastable = self.broadcastable and all(v.type == VariableType.PARAMETER for v in kwargs.values())
        given = dict(zip(self._input_variable_names, args))
        given.update(kwargs)
        inputs = [(k, given[k]) for k in self._input_names if k in given]
        outputs = [(k, Variable(shape=None)) for k in self._output_names]
        fe = TorchFunctionEvaluation(self, inputs, outputs, broadcastable=broadcastable)
        outs = [v for _, v in fe.outputs]
        return outs[0] if len(outs) == 1 else tuple(outs)

    def replicate_self(self, attribute_map=None):
        """a copy that shares the module and holds replicas (same UUIDs) of the parameter variables"""
        new = copy.copy(self)
        new._parameters = {}
        for k, v in self._parameters.items():
            r = v.replicate_self()
            r.inherited_name = k
            new._parameters[k] = r
        new._parameter_names = list(self._parameter_names)
        new._torch_names = dict(self._torch_names)
        new._input_names = copy.copy(self._input_names)
        new._input_variable_names = copy.copy(self._input_variable_names)
        new._output_names = list(self._output_names)
        return new

    def __deepcopy__(self, memo):
        """(FactorGraph.clone) the module is shared, as its arrays are; the variables are copied with the graph"""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        memo[id(self._module)] = self._module
        for k, v in self.__dict__.items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new


MXFusionGluonFunction = MXFusionTorchFunction      # source-compatible aliases
GluonFunctionEvaluation = TorchFunctionEvaluation
