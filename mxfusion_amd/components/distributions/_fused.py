"""What the classes over the fused log-pdf kernels share (mvn.py, wishart.py, dirichlet.py, categorical.py, univariate.py, and the dense
layer of components/functions/torch_function.py): operands flattened onto one batch axis, the gradient buffers of a reverse mode, and the
bare replica of a factor without constructor state of its own."""
import torch

from ... import ops
from .distribution import Distribution


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _flatten(t, lead, tail, full=False):
    """t (S|1, ..., *tail-broadcastable) -> (S|1, B|1, *tail): leading dimensions aligned with `lead` from the right and flattened into one
    batch axis, which stays at extent 1 where t has nothing but ones there (unless `full`).  A leading axis that is an expanded view goes
    back to extent 1 first: the kernels broadcast it, and autograd sums its gradient."""
    k = len(tail)
    if t.dim() < 1 + k:
        raise ValueError('an operand of shape %s has no sample axis in front of %d trailing dimension(s)'
                         % (tuple(t.shape), k))
    want = 1 + len(lead) + k
    if t.dim() < want:
        t = t.reshape((t.shape[0],) + (1,) * (want - t.dim()) + tuple(t.shape[1:]))
    t = ops._shared_axes(t, range(t.dim() - k), None)[0]
    mid = tuple(t.shape[1:t.dim() - k])
    if tuple(t.shape[t.dim() - k:]) != tuple(tail):
        t = t.expand(tuple(t.shape[:t.dim() - k]) + tuple(tail))
    if all(m == 1 for m in mid) and not (full and _numel(lead) > 1):
        return t.reshape((t.shape[0], 1) + tuple(tail))
    if mid != tuple(lead):
        t = t.expand((t.shape[0],) + tuple(lead) + tuple(tail))
    return t.reshape((t.shape[0], _numel(lead)) + tuple(tail))


def _carve(sizes, like):
    """ONE zero-filled buffer carved into len(sizes) accumulators with 16-byte aligned starts (size 0: None), as _NormalLogPdfSumFn does:
    the kernels accumulate into their outputs, and a fill per output would be a launch per output."""
    starts, off = [], 0
    for s in sizes:
        starts.append(off)
        off += (s + 3) // 4 * 4
    buf = torch.zeros(max(off, 1), dtype=like.dtype, device=like.device)
    return [buf[o:o + s] if s else None for o, s in zip(starts, sizes)]


def carved_grads(shapes, need, like):
    """_carve's accumulators for the operands of `shapes` whose gradient is wanted (`need`), each viewed in its shape; None for the others"""
    grads = _carve([_numel(s) if w else 0 for s, w in zip(shapes, need)], like)
    return [None if t is None else t.view(tuple(s)) for t, s in zip(grads, shapes)]


# Which route Distribution.log_pdf_per_sample takes for Normal and the univariate family: the per-sample HIP reductions
# (mxf_normal_logpdf_ps*, mxf_univariate_logpdf_ps*) where S * n >= PER_SAMPLE_KERNEL_MIN_ELEMS, below it the un-reduced log_pdf summed over
# every axis but the first.  Measured on the MI355X in both size classes ("Score-function inference"); 0 sends every
# size to the kernels, None none.
PER_SAMPLE_KERNEL_MIN_ELEMS = 0


def per_sample_kernels(S, n):
    return PER_SAMPLE_KERNEL_MIN_ELEMS is not None and S * n >= PER_SAMPLE_KERNEL_MIN_ELEMS


class _LogPdfPerSampleFn(torch.autograd.Function):
    """scale * sum_i log p(x[s,i] | a, b), (S,).  x (S, n...); a, b: 1 or n elements, or (S, n...) with a sample axis of their own.  The
    reverse mode hands the incoming (S,) cotangent to the kernel as its per-sample weights."""

    @staticmethod
    def forward(ctx, kind, scale, x, a, b):
        ctx.kind, ctx.scale = kind, float(scale)
        ctx.save_for_backward(x, a, b)
        return ops.logpdf_per_sample_(kind, x, a, b, scale, torch.zeros(x.shape[0], dtype=x.dtype, device=x.device))

    @staticmethod
    def backward(ctx, g):
        x, a, b = ctx.saved_tensors
        grads = carved_grads((x.shape, a.shape, b.shape), ctx.needs_input_grad[2:5], x)
        if any(t is not None for t in grads):
            ops.logpdf_per_sample_bwd_(ctx.kind, x, a, b, g.contiguous(), ctx.scale, *grads)
        return (None, None) + tuple(grads)


def spread_operands(x, a, b):
    """x (S|1, ...) and the parameters a, b (S|1, ...), each broadcastable against it, in the layouts of the elementwise kernels: x
    (S, ...) contiguous; a parameter flat with one element, per element (no sample axis), or (S, ...) with one"""
    S = max(int(x.shape[0]), int(a.shape[0]), int(b.shape[0]))
    rest = tuple(x.shape[1:])

    def spread(p):
        if p.numel() == 1:
            return p.reshape(1)
        return p[0].expand(rest).contiguous() if p.shape[0] == 1 else p.expand((S,) + rest).contiguous()
    return x.expand((S,) + rest).contiguous(), spread(a), spread(b)


def log_pdf_per_sample(kind, scale, x, a, b):
    """(S,) sums of scale * log p over every axis but the first, on the per-sample kernels; operands as spread_operands takes them"""
    return _LogPdfPerSampleFn.apply(kind, scale, *spread_operands(x, a, b))


def replicate(dist):
    """(factor.py:121-143) a factor of dist's class with the same names and UUID and no inputs or outputs yet, for a replicated graph to
    wire up.  For a class without constructor state of its own: nothing but what Distribution holds is carried over."""
    rep = dist.__class__.__new__(dist.__class__)
    Distribution.__init__(rep, None, None, list(dist.input_names), list(dist.output_names), rand_gen=dist._rand_gen, dtype=dist.dtype,
                          ctx=dist.ctx)
    rep.uuid = dist.uuid
    rep.log_pdf_scaling = dist.log_pdf_scaling
    return rep
