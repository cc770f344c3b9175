"""The dX GEMM of a BPTT step, dX = dG [W_ih | W_hh], reads its weights IN PLACE as column segments of B (capmi_gemm_desc.n_bcol,
loader / consumer kernel of gemm_lc.hip) instead of from a copy packed side by side.  Every output element is the same sum over
the same K slices in the same order, so the K-slice slabs of the two routes must be equal bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def wide(shape, g, scale=1.0):
    x = torch.randn(shape, generator=g)
    return (x * torch.exp(1.5 * torch.randn(shape, generator=g)) * scale).float()


# R = 1000: the last column block of every segment is ragged (1000 = 7 * 128 + 104); R = 512: whole blocks
@pytest.mark.parametrize('nsegs', [2, 3])
@pytest.mark.parametrize('R', [1000, 512])
@pytest.mark.parametrize('M', [50, 64])
def test_column_segmented_dx_gemm_equals_packed_route_bit_for_bit(dev, M, R, nsegs):
    from imagecaptioning.pytorch_amd import ops
    g = torch.Generator().manual_seed(1000 * nsegs + R + M)
    K = 4 * R
    dG = wide((M, K), g, 0.3).to(dev)
    planes = ops.planes_from_f32(dG)
    # segment 0 is the leading R columns of a WIDER matrix (att W_ih(:, 0:R) of the attention LSTM: row stride 2R + E), the others are
    # whole matrices of their own; two segments of R columns or three (R | R | R)
    E = 1000
    w0 = (torch.randn((K, 2 * R + E), generator=g) * 0.05).to(dev)
    rest = [(torch.randn((K, R), generator=g) * 0.05).to(dev) for _ in range(nsegs - 1)]
    cols = [(w0, 2 * R + E, R)] + [(w, R, R) for w in rest]
    N = nsegs * R
    packed = torch.cat([w0[:, :R]] + rest, dim=1).contiguous()
    assert packed.shape == (K, N)

    def run(b_cols):
        ws = ops.Workspace(dev, 8 << 20)
        ws.buf[ops.Workspace.COUNTER_FLOATS:].fill_(float('nan'))          # every slab word must be written
        out = torch.zeros(M, N, device=dev)
        segs = [(dG, K, None if b_cols else packed, N, K, 1)]
        splits = ops.gemm(segs, M, N, out, b_layout=1, ws=ws, defer_reduce=True, a_planes=[planes], b_cols=b_cols)
        torch.cuda.synchronize()
        return ws.slabs[:splits * M * N].view(splits, M, N).clone(), splits

    s_col, n_col = run(cols)
    s_pack, n_pack = run(None)
    assert n_col == n_pack and n_col > 1
    assert not bool(torch.isnan(s_col).any()) and not bool(torch.isnan(s_pack).any())
    assert torch.equal(s_col, s_pack)
    # ... and they are the product (fp32-grade: exact bf16x3 terms, fp32 accumulation)
    ref = dG.double() @ packed.double()
    mag = dG.double().abs() @ packed.double().abs() + 1e-30
    assert float(((s_col.double().sum(0) - ref).abs() / mag).max()) < 1e-6


def test_column_segments_are_refused_where_no_kernel_reads_them(dev):
    """[N][K] weights, or activations without planes: CAPMI_EINVAL, never another kernel on the wrong operand."""
    from imagecaptioning.pytorch_amd import ops
    M, R = 50, 512
    dG = torch.randn(M, 4 * R, device=dev)
    w = [torch.randn(4 * R, R, device=dev) for _ in range(2)]
    cols = [(w[0], R, R), (w[1], R, R)]
    out = torch.zeros(M, 2 * R, device=dev)
    segs = [(dG, 4 * R, None, 2 * R, 4 * R, 1)]
    with pytest.raises(Exception):
        ops.gemm(segs, M, 2 * R, out, b_layout=1, defer_reduce=True, b_cols=cols)                       # no planes
    with pytest.raises(Exception):
        ops.gemm(segs, M, 2 * R, out, b_layout=0, defer_reduce=True, a_planes=[ops.planes_from_f32(dG)], b_cols=cols)
