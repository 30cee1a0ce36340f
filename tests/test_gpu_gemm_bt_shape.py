"""The K-major f16x2 product (gemm_bt.hip, mxf_gemm_f16x2_planes_kmajor) at the smallest shapes where its k-block pairing, its request stream
across work items, its U-row rotation and its lane-to-(m, n) output map can go wrong and that test_gpu_gemm.py does not pin.  Bounds as there:
6e-7 normwise against sum |a| |b| (float64 reference), for C and for the fused row U = w^T Bt."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _unblock(out, M, N, blocked):
    return out.view(N // 16, M, 16).permute(1, 0, 2).reshape(M, N) if blocked else out.view(M, N)


@pytest.mark.parametrize('M,N,K,blocked', [
    (256, 256, 80, True),          # five k blocks: an odd count above the minimum, the single last block behind two full pairs
    (512, 512, 96, True),          # two row tiles share a column strip: the owner of the U row rotates (strip 0 -> tile 0, strip 1 -> tile 1); even count
    (256, 256 * 300, 48, False),   # 300 items on at most 256 workgroups (the ABI has no grid argument): some take two items of three k blocks
                                   # each, so an item's single last block sits directly in front of the next item's first pair in the stream
])
def test_kmajor_product_block_pairs_items_and_u_row(M, N, K, blocked):
    from mxfusion_amd import ops
    g = torch.Generator(device='cuda').manual_seed(M + N + K)
    A = torch.randn(M, K, device='cuda', generator=g) * torch.exp(torch.randn(M, 1, device='cuda', generator=g))
    Bt = torch.rand(K, N, device='cuda', generator=g) - 0.3
    w = torch.randn(K, device='cuda', generator=g) * 3.0
    out = torch.full((M * N,), float('nan'), device='cuda')
    _, U = ops.gemm_f16x2_planes_kmajor(ops.f16x2_split(A), ops.f16x2_split(Bt), M, N, K, alpha=0.75, out=out.view(M, N), blocked=blocked, w=w)
    C = _unblock(out, M, N, blocked)
    assert not torch.isnan(C).any()
    ref = 0.75 * (A.double() @ Bt.double())
    scale = A.double().abs() @ Bt.double().abs()
    assert float(((C.double() - ref).abs() / scale).max()) < 6e-7
    uref = w.double() @ Bt.double()
    uscale = w.double().abs() @ Bt.double().abs()
    assert float(((U.double() - uref).abs() / uscale).max()) < 6e-7


@pytest.mark.parametrize('K', [48, 64])
@pytest.mark.parametrize('row,col', [(137, 203), (6, 49), (255, 0), (112, 255)])
def test_kmajor_product_places_a_single_entry_exactly(row, col, K):
    """A has one non-zero row, Bt one non-zero column, both of small integers: every f16 term, every product and the f32 sum are exact, so C
    is the one entry (row, col) = sum_k A[row, k] Bt[k, col], bit for bit, and zero everywhere else -- in the row-major and in the blocked
    layout.  A wrong lane-to-(m, n) map of the epilogue displaces the entry; a wrong k pairing changes its value."""
    from mxfusion_amd import ops
    M = N = 256
    g = torch.Generator(device='cuda').manual_seed(row * 1000 + col + K)
    A = torch.zeros(M, K, device='cuda')
    Bt = torch.zeros(K, N, device='cuda')
    A[row] = torch.randint(-40, 41, (K,), device='cuda', generator=g).float()
    Bt[:, col] = torch.randint(1, 60, (K,), device='cuda', generator=g).float()      # distinct per k: a swapped or repeated k block shows
    want = torch.zeros(M, N, device='cuda')
    want[row, col] = (A[row].double() * Bt[:, col].double()).sum().float()
    w = torch.arange(1, K + 1, device='cuda', dtype=torch.float32)
    uwant = torch.zeros(N, device='cuda')
    uwant[col] = (w.double() * Bt[:, col].double()).sum().float()
    pa, pbt = ops.f16x2_split(A), ops.f16x2_split(Bt)
    for blocked in (False, True):
        out = torch.full((M * N,), float('nan'), device='cuda')
        _, U = ops.gemm_f16x2_planes_kmajor(pa, pbt, M, N, K, out=out.view(M, N), blocked=blocked, w=w)
        assert torch.equal(_unblock(out, M, N, blocked), want)
        assert torch.equal(U, uwant)
