"""CPU tests of the two helpers under every reverse-mode wrapper of ops.py: _shared_axes (an expanded axis is a shared axis and is never
materialised) and _check_buffers (a gradient buffer is contiguous and shaped like its operand with the shared axes at extent 1)."""
import pytest
import torch

S, B, K = 3, 5, 4


@pytest.mark.parametrize('shape, shared', [((1, B, K), (0,)), ((S, 1, K), (1,)), ((1, 1, K), (0, 1))])
def test_an_expanded_operand_is_passed_as_it_is(shape, shared):
    from mxfusion_amd import ops
    t = torch.arange(float(shape[0] * shape[1] * K)).reshape(shape)
    got, axes = ops._shared_axes(t.expand(S, B, K), (0, 1))
    assert got.data_ptr() == t.data_ptr() and tuple(got.shape) == shape and torch.equal(got, t)
    for d in (0, 1):
        assert (axes[d] == (1, 0)) == (d in shared)
        assert (axes[d][1] == 0) == (d in shared)
        if d not in shared:
            assert axes[d] == ((S, B)[d], t.stride(d))


def test_only_the_named_axes_are_narrowed():
    from mxfusion_amd import ops
    t = torch.zeros(1, 1, K)
    got, axes = ops._shared_axes(t.expand(S, B, K), (0,), None)
    assert tuple(got.shape) == (1, B, K) and axes == [(1, 0)] and got.data_ptr() == t.data_ptr()


def test_a_padded_operand_comes_back_contiguous_and_extent_one_is_shared():
    from mxfusion_amd import ops
    buf = torch.arange(float(S * 1 * (K + 2))).reshape(S, 1, K + 2)
    padded = buf[..., :K]
    got, axes = ops._shared_axes(padded, (0, 1))
    assert got.is_contiguous() and torch.equal(got, padded) and axes == [(S, K), (1, 0)]
    kept, axes = ops._shared_axes(padded, (0, 1), lambda t: t.stride(-1) == 1)           # the layout fits: no copy
    assert kept.data_ptr() == padded.data_ptr() and axes == [(S, K + 2), (1, 0)]
    both = torch.zeros(1, 1, K + 2)[..., :K].expand(S, B, K)                               # a copy never materialises a shared axis
    got, axes = ops._shared_axes(both, (0, 1))
    assert tuple(got.shape) == (1, 1, K) and got.is_contiguous() and axes == [(1, 0), (1, 0)]


def test_the_buffer_check():
    from mxfusion_amd import ops
    p, _ = ops._shared_axes(torch.zeros(1, 1, K).expand(S, B, K), (0, 1))
    cot = torch.zeros(S, B)
    ops._check_buffers('test', (cot, (S, B)), (torch.zeros(1, 1, K), p.shape), (None, (S, B, K)))
    with pytest.raises(ValueError):
        ops._check_buffers('test', (cot, (S, B)), (torch.zeros(S, B, K), p.shape))           # the full shape of a shared operand
    with pytest.raises(ValueError):
        ops._check_buffers('test', (cot, (S, B)), (torch.zeros(1, 1, 2 * K)[..., ::2], p.shape))
    with pytest.raises(ValueError):
        ops._check_buffers('test', (torch.zeros(B, S).t(), (S, B)))
