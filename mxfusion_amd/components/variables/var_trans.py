"""Variable transformations (mxfusion/components/variables/var_trans.py:53-147).  Softplus runs as a HIP
kernel (mxf_softplus_fwd / _bwd) wrapped in an autograd Function; Logistic, and a batch of Logistic and offset Softplus
transformations, run on the segmented kernel (mxf_transform_fwd / _bwd)."""
import math

import torch

from ... import ops


class _SoftplusFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.softplus(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ops.softplus_bwd_(x, dy, torch.zeros_like(x))


class _SoftplusManyFn(torch.autograd.Function):
    """softplus of several tensors as ONE kernel each way (concatenate -> mxf_softplus_fwd -> views): a model has five to ten positive
    parameters, and every one of them cost a launch forward and two backward in the step's launch-paced head and tail."""

    @staticmethod
    def forward(ctx, *xs):
        sizes = [x.numel() for x in xs]
        flat = torch.cat([x.reshape(-1) for x in xs]) if len(xs) > 1 else xs[0].reshape(-1)
        ctx.save_for_backward(flat)
        ctx.meta = (sizes, [x.shape for x in xs])
        y = ops.softplus(flat)
        return tuple(p.view(sh) for p, sh in zip(torch.split_with_sizes(y, sizes), ctx.meta[1]))

    @staticmethod
    def backward(ctx, *dys):
        (flat,) = ctx.saved_tensors
        sizes, shapes = ctx.meta
        parts = [(d.reshape(-1) if d is not None else flat.new_zeros(n)) for d, n in zip(dys, sizes)]
        dy = torch.cat(parts) if len(parts) > 1 else parts[0]
        dx = ops.softplus_bwd_(flat, dy, torch.zeros_like(flat))
        return tuple(p.view(sh) for p, sh in zip(torch.split_with_sizes(dx, sizes), shapes))


class _TransformManyFn(torch.autograd.Function):
    """Several tensors, each under a transformation of its own, as ONE kernel each way (concatenate -> mxf_transform_fwd -> views); `maps`
    holds (kind, p0, p1) per tensor as ops.transform takes them."""

    @staticmethod
    def forward(ctx, maps, *xs):
        sizes = [x.numel() for x in xs]
        flat = torch.cat([x.reshape(-1) for x in xs]) if len(xs) > 1 else xs[0].contiguous().view(-1)
        ctx.save_for_backward(flat)
        ctx.meta = ([(k, n, p0, p1) for (k, p0, p1), n in zip(maps, sizes)], sizes, [x.shape for x in xs])
        y = ops.transform(ctx.meta[0], flat)
        return tuple(p.view(sh) for p, sh in zip(torch.split_with_sizes(y, sizes), ctx.meta[2]))

    @staticmethod
    def backward(ctx, *dys):
        (flat,) = ctx.saved_tensors
        segments, sizes, shapes = ctx.meta
        parts = [(d.reshape(-1) if d is not None else flat.new_zeros(n)) for d, n in zip(dys, sizes)]
        dy = torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()
        dx = ops.transform_bwd_(segments, flat, dy, torch.zeros_like(flat))
        return (None,) + tuple(p.view(sh) for p, sh in zip(torch.split_with_sizes(dx, sizes), shapes))


def _segment_map(t):
    """(kind, p0, p1) of a transformation the segmented kernel runs: a Logistic, or a softplus with an offset; None for any other"""
    if type(t) is Logistic:
        return ('logistic', t._lower, t._difference)
    if type(t) in (Softplus, PositiveTransformation) and t._offset:
        return ('softplus', t._offset, 0.)
    return None


def transform_many(transformations, tensors):
    """[t.transform(x) for t, x in zip(...)] with every plain softplus (offset 0, device tensor) of the list batched into one kernel call,
    and every Logistic and offset softplus of one dtype and device into one call of the segmented kernel."""
    out = list(tensors)
    groups = {}
    for i, (t, x) in enumerate(zip(transformations, tensors)):
        if isinstance(x, torch.Tensor) and x.is_cuda and _segment_map(t) is not None:
            groups.setdefault((x.dtype, x.device), []).append(i)
    segmented = set()
    for members in groups.values():
        if len(members) > 1:
            ys = _TransformManyFn.apply(tuple(_segment_map(transformations[i]) for i in members), *[tensors[i] for i in members])
            for i, y in zip(members, ys):
                out[i] = y
            segmented.update(members)
    idx = [i for i, (t, x) in enumerate(zip(transformations, tensors))
           if type(t) in (Softplus, PositiveTransformation) and not t._offset and isinstance(x, torch.Tensor) and x.is_cuda]
    if len(idx) > 1 and len({(tensors[i].dtype, tensors[i].device) for i in idx}) == 1:
        for i, y in zip(idx, _SoftplusManyFn.apply(*[tensors[i] for i in idx])):
            out[i] = y
        rest = [i for i in range(len(out)) if i not in set(idx)]
    else:
        rest = range(len(out))
    for i in rest:
        if i not in segmented:
            out[i] = transformations[i].transform(tensors[i])
    return out


class VariableTransformation(object):
    def transform(self, var, F=None, dtype=None):
        raise NotImplementedError

    def inverseTransform(self, out_var, F=None, dtype=None):
        raise NotImplementedError


class Softplus(VariableTransformation):
    """f = log(1+exp(x)) + c ; f^-1 = log(exp(x-c)-1)   (var_trans.py:53-91)."""

    def __init__(self, offset):
        self._offset = offset

    def transform(self, var, F=None, dtype=None):
        y = _SoftplusFn.apply(var)
        return y + self._offset if self._offset else y

    def inverseTransform(self, out_var, F=None, dtype=None):
        # host-side, once per parameter assignment (var_trans.py:91: log(expm1(y)))
        return torch.log(torch.expm1(out_var - self._offset))


class PositiveTransformation(Softplus):
    def __init__(self):
        super(PositiveTransformation, self).__init__(offset=0.)


class Logistic(VariableTransformation):
    """f = lower + (upper - lower) sigmoid(x), a parameter kept inside [lower, upper]; f^-1 = log((y - lower) / (upper - y))
    (var_trans.py:105-147)."""

    def __init__(self, lower, upper):
        if lower >= upper:
            raise ValueError('The lower bound is above the upper bound')
        self._lower, self._upper = lower, upper
        lo, hi = float(lower), float(upper)
        d = hi - lo
        while lo + d > hi:             # the kernel forms the upper bound as lower + difference, which rounding may carry past `upper`
            d = math.nextafter(d, 0.)
        self._difference = d

    def transform(self, var, F=None, dtype=None):
        return _TransformManyFn.apply((_segment_map(self),), var)[0]

    def inverseTransform(self, out_var, F=None, dtype=None):
        # host-side, once per parameter assignment, in float64: the reference's clip to [lower + 1e-10, upper - 1e-10] (var_trans.py:146)
        # moves nothing in float32 for bounds like (1, 200000), and log(0) or log(inf) would follow at a bound
        y = out_var.to(torch.float64).clamp(self._lower + 1e-10, self._upper - 1e-10)
        return torch.log((y - self._lower) / (self._upper - y)).to(out_var.dtype)
