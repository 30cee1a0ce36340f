"""CPU self-test of tests/_strided.py: the carved views hold what they were given, and the padding checker sees a store one element past a
row end, into the gap between samples, in front of the view and behind the last sample -- and nothing when a kernel stays inside."""
import numpy as np
import pytest
import torch

import _strided as st


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('shape', [(5, 7), (3, 5, 7), (1, 4, 4)])
@pytest.mark.parametrize('ld_pad,lead,gap', [(0, 0, 0), (8, 0, 0), (3, 0, 0), (0, 1, 0), (0, 0, 5), (3, 1, 5)])
def test_carve_round_trips(dtype, shape, ld_pad, lead, gap):
    rng = np.random.RandomState(sum(shape) + ld_pad + lead + gap)
    a = rng.randn(*shape)
    v = st.carve(a, ld_pad=ld_pad, lead=lead, gap=gap, fill=st.SENTINEL, dtype=dtype)
    R, C = shape[-2:]
    assert v.dtype == dtype and tuple(v.shape) == shape
    assert torch.equal(v, torch.as_tensor(a).to(dtype))
    assert st.ld(v) == C + ld_pad and v.storage_offset() == lead
    if len(shape) == 3:
        assert v.stride(0) == R * (C + ld_pad) + gap
        assert st.sstride(v) == (0 if shape[0] == 1 else v.stride(0))
    base = v._base
    S = shape[0] if len(shape) == 3 else 1
    assert base.dim() == 1 and base.numel() == lead + S * (R * (C + ld_pad) + gap) + st.TAIL
    # the byte address of the view is `lead` elements into the allocation, and everything outside the view is the fill
    assert v.data_ptr() == base.data_ptr() + lead * base.element_size()
    outside = st._outside(v)
    assert int(outside.sum()) == base.numel() - a.size
    assert bool((base[outside] == st.SENTINEL).all())
    # NaN padding for inputs
    vn = st.carve(a, ld_pad=ld_pad, lead=lead, gap=gap, dtype=dtype)
    assert bool(torch.isnan(vn._base[st._outside(vn)]).all()) and not bool(torch.isnan(vn).any())
    st.assert_padding_untouched(v, st.snapshot(v))


def _numpy_kernel(v, bug):
    """C[s] = 2 C[s] on the raw allocation with explicit ld / stride indexing, as a HIP kernel would; `bug` adds one stray store"""
    base = v._base.numpy()           # shares memory with the tensor
    off, (S, R, C) = v.storage_offset(), v.shape
    sS, ld = v.stride(0), v.stride(1)
    for s in range(S):
        for r in range(R):
            for c in range(C):
                base[off + s * sS + r * ld + c] *= 2.0
    if bug == 'row_end':             # one element past the end of a row (a vector store that ignores the row width)
        base[off + 1 * sS + 2 * ld + C] = 1.0
    elif bug == 'gap':               # into the gap between two samples (a kernel that takes the sample stride for R * ld)
        base[off + 1 * R * ld] = 1.0
    elif bug == 'front':             # in front of a misaligned base (a store rounded down to 16 bytes)
        base[off - 1] = 1.0
    elif bug == 'tail':              # behind the last row of the last sample
        base[off + (S - 1) * sS + (R - 1) * ld + C] = 1.0


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('bug', [None, 'row_end', 'gap', 'front', 'tail'])
def test_checker_fires_on_stray_stores_only(dtype, bug):
    a = np.arange(2 * 4 * 6, dtype=np.float64).reshape(2, 4, 6)
    v = st.carve(a, ld_pad=3, lead=1, gap=5, fill=st.SENTINEL, dtype=dtype)
    snap = st.snapshot(v)
    _numpy_kernel(v, bug)
    assert torch.equal(v, torch.as_tensor(2.0 * a).to(dtype))        # the "kernel" did its work inside the view
    if bug is None:
        st.assert_padding_untouched(v, snap)
        assert st.padding_diff(v, snap).numel() == 0
        return
    with pytest.raises(AssertionError, match='outside the view'):
        st.assert_padding_untouched(v, snap, bug)
    assert st.padding_diff(v, snap).numel() == 1


def test_checker_compares_bits_not_values():
    """NaN padding compares equal to itself through the integer view, and a changed NaN payload or a sign flip of zero is seen."""
    v = st.carve(np.zeros((2, 3, 3)), ld_pad=2, gap=1, fill=st.NAN, dtype=torch.float32)
    snap = st.snapshot(v)
    st.assert_padding_untouched(v, snap)                 # NaN != NaN as floats; equal as bits
    st.assert_unchanged(v, snap)
    v._base.view(torch.int32)[3] ^= 1                    # row 0's first padding element: another NaN payload
    assert bool(torch.isnan(v._base[3]))
    with pytest.raises(AssertionError):
        st.assert_padding_untouched(v, snap)
    z = st.carve(np.ones((2, 2)), ld_pad=1, fill=0.0, dtype=torch.float64)
    zs = st.snapshot(z)
    z._base[2] = -0.0
    with pytest.raises(AssertionError):
        st.assert_padding_untouched(z, zs)
    w = st.carve(np.ones((2, 2)), ld_pad=1, dtype=torch.float64)
    ws = st.snapshot(w)
    w[0, 0] = 5.0                                        # inside the view: fine for an output, an error for an input
    st.assert_padding_untouched(w, ws)
    with pytest.raises(AssertionError, match='read-only'):
        st.assert_unchanged(w, ws)


def test_variants_cover_the_layouts_of_the_issue():
    assert st.VARIANTS['ld+8'][1] % 4 == 0 and st.VARIANTS['ld+3'][1] % 2 == 1          # (a) keeps 16-byte rows, (b) breaks them for both dtypes
    assert st.VARIANTS['lead1'][1:] == (0, 1, 0)                                          # (c) the base only
    assert st.VARIANTS['gap5'][3] % 4 != 0 and st.VARIANTS['gap5'][3] % 2 != 0           # (d) breaks stride % VEC for both dtypes
    v = st.carve_as(np.ones((2, 3, 4)), 'gap5+ld8', device='cpu')
    assert v.stride() == (3 * 12 + 5, 12, 1)
