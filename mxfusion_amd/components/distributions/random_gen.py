"""Noise source for reparameterised sampling: the injection seam of
mxfusion/components/distributions/random_gen.py:21-98 (tests use a mock that replays a caller-supplied
buffer, util/testutils.py:58-93).  Drawing the noise itself (N(0,1), uniform, Laplace, Gamma) is plumbing (torch's generators on
the device); everything downstream of it is HIP."""
import torch


class RandomGenerator(object):
    @staticmethod
    def sample_normal(loc=0, scale=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        raise NotImplementedError

    @staticmethod
    def sample_gamma(alpha=1, beta=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        raise NotImplementedError

    @staticmethod
    def sample_uniform(low=0., high=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        raise NotImplementedError

    @staticmethod
    def sample_laplace(location=0., scale=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        raise NotImplementedError

    @staticmethod
    def sample_multinomial(data, shape=None, get_prob=False, dtype=None, F=None):
        raise NotImplementedError

    @staticmethod
    def sample_bernoulli(prob_true=0.5, dtype=None, shape=None, F=None):
        raise NotImplementedError


def _numel(shape):
    n = 1
    for s in shape or ():
        n *= int(s)
    return n


class TorchRandomGenerator(RandomGenerator):
    @staticmethod
    def sample_normal(loc=0, scale=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        from ...common import config
        eps = torch.randn(tuple(shape), dtype=config.torch_dtype(dtype), device=ctx or config.get_default_device())
        if scale != 1:
            eps = eps * scale
        if loc != 0:
            eps = eps + loc
        return eps

    @staticmethod
    def sample_gamma(alpha=1, beta=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        """random_gen.py:141-160: alpha the shape, beta the RATE; array parameters of shape (x, y) give (x, y) + shape draws."""
        from ...common import config
        shape = tuple(shape or ())
        if not isinstance(alpha, torch.Tensor):
            alpha = torch.full((), float(alpha), dtype=config.torch_dtype(dtype), device=ctx or config.get_default_device())
        beta = torch.as_tensor(beta, dtype=alpha.dtype, device=alpha.device)
        alpha, beta = torch.broadcast_tensors(alpha, beta)
        full = tuple(alpha.shape) + shape
        tail = (Ellipsis,) + (None,) * len(shape)
        return torch.distributions.Gamma(alpha[tail].expand(full), beta[tail].expand(full), validate_args=False).sample()

    @staticmethod
    def sample_uniform(low=0., high=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        """random_gen.py:163-183: uniform on [low, high)."""
        from ...common import config
        u = torch.rand(tuple(shape or ()), dtype=config.torch_dtype(dtype), device=ctx or config.get_default_device())
        return u * (high - low) + low

    @staticmethod
    def sample_laplace(location=0., scale=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        """random_gen.py:186-219: U uniform on [-1/2, 1/2), location - scale sign(U) log(1 - 2 |U|); the one U = -1/2 the generator can
        return would be log 0, an infinite draw: the argument of the logarithm is kept at the smallest normal number."""
        U = TorchRandomGenerator.sample_uniform(low=-0.5, high=0.5, shape=shape, dtype=dtype, ctx=ctx)
        return location - scale * torch.sign(U) * torch.log((1 - 2 * torch.abs(U)).clamp_min(torch.finfo(U.dtype).tiny))

    @staticmethod
    def sample_multinomial(data, shape=None, get_prob=False, dtype=None, F=None):
        """random_gen.py:101-124: data (..., K) holds PROBABILITIES along its last axis (each row is normalised by the sampler); one class
        index per row, data.shape[:-1], or with `shape` that many per row, data.shape[:-1] + shape.  dtype None: int64.  get_prob: also the
        log-probability of each draw."""
        from ...common import config
        K = int(data.shape[-1])
        extra = tuple(shape) if shape is not None and not isinstance(shape, int) else (() if shape is None else (int(shape),))
        idx = torch.multinomial(data.reshape(-1, K), max(_numel(extra), 1), replacement=True).reshape(tuple(data.shape[:-1]) + extra)
        out = idx if dtype is None else idx.to(dtype if isinstance(dtype, torch.dtype) else config.torch_dtype(dtype))
        if not get_prob:
            return out
        rows = data.reshape(tuple(data.shape[:-1]) + (1,) * len(extra) + (K,)).expand(tuple(idx.shape) + (K,))
        logp = torch.log(torch.gather(rows, -1, idx.unsqueeze(-1)).squeeze(-1) / data.sum(-1).reshape(tuple(data.shape[:-1]) + (1,) * len(extra)))
        return out, logp

    @staticmethod
    def sample_bernoulli(prob_true=0.5, dtype=None, shape=None, F=None):
        """random_gen.py:127-138 as it is meant: uniform < prob_true, true with probability prob_true (the reference's `>` is true with
        probability 1 - prob_true).  1 / 0 in `dtype`."""
        from ...common import config
        dt = dtype if isinstance(dtype, torch.dtype) else config.torch_dtype(dtype)
        device = prob_true.device if isinstance(prob_true, torch.Tensor) else config.get_default_device()
        u = torch.rand(tuple(shape or ()), dtype=dt if dt.is_floating_point else torch.float32, device=device)
        return (u < prob_true).to(dt)


MXNetRandomGenerator = TorchRandomGenerator   # source-compatible alias


class MockRandomGenerator(RandomGenerator):
    """Replays `samples` (flattened, cycled) -- util/testutils.py:58-93 MockMXNetRandomGenerator."""

    def __init__(self, samples):
        self._samples = samples.reshape(-1)
        self._pos = 0

    def _replay(self, shape):
        shape = tuple(shape)
        n = _numel(shape)
        idx = (torch.arange(n, device=self._samples.device) + self._pos) % self._samples.numel()
        self._pos = (self._pos + n) % self._samples.numel()
        return self._samples[idx].reshape(shape).clone()

    def sample_normal(self, loc=0, scale=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._replay(shape)

    def sample_gamma(self, alpha=1, beta=1, shape=None, dtype=None, out=None, ctx=None, F=None):
        """testutils.py:83-87: the buffer in the shape of the draw, alpha's shape followed by `shape`."""
        return self._replay((tuple(alpha.shape) if isinstance(alpha, torch.Tensor) else ()) + tuple(shape or ()))

    def sample_uniform(self, low=0., high=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._replay(shape)

    def sample_laplace(self, location=0., scale=1., shape=None, dtype=None, out=None, ctx=None, F=None):
        return self._replay(shape)

    def sample_multinomial(self, data, shape=None, get_prob=False, dtype=None, F=None):
        """testutils.py:77-78: the buffer in the shape of one draw per row, data.shape[:-1]."""
        return self._replay(tuple(data.shape[:-1]))

    def sample_bernoulli(self, prob_true=0.5, dtype=None, shape=None, F=None):
        """testutils.py:80-81."""
        return self._replay(shape)


MockMXNetRandomGenerator = MockRandomGenerator
