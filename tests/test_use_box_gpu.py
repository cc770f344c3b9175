"""use_box on the device: capmi_region_rows_build (csrc/region_rows.hip) against the reference's own rows (tests/golden/box_ref.npz),
the HBM-resident store built by it against the loader's host path, att_embed at the odd width D + 5, and tools/train.py."""
import os
import sys

import numpy as np
import pytest
import torch

import box_ds as BD
import gemm_ref64 as G
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
SENT = -123.25                                     # what the destination holds before the launch


def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


def _loader(argv):
    sys.path.insert(0, PKG)
    from captioning.data.feature_loader import FeatureLoader
    return FeatureLoader(_opts(argv), workers=2, processes=False)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _run(dev, atts, boxes, hw, na, ub, nb, offset=0, extra_ld=0, lead=2, trail=3):
    """the kernel on the images (atts[i] [K_i, D], boxes[i] [K_i, 4], hw[i] = (height, width)) -> (rows per image, the whole
    destination buffer as numpy, the boolean map of the elements the launch may write).  The destination starts `offset` floats into
    its allocation (+ `lead` untouched rows), its leading dimension is the row + extra_ld."""
    from imagecaptioning.pytorch_amd import ops
    D = atts[0].shape[1]
    W = D + 5 * ub
    ldd = W + extra_ld
    ks = [a.shape[0] for a in atts]
    R = sum(ks)
    table = np.zeros((len(atts), 4), dtype=np.int32)
    table[:, 0] = np.concatenate([[0], np.cumsum(ks)[:-1]])
    table[:, 1] = ks
    table[:, 2:] = hw
    src = torch.from_numpy(np.concatenate(atts, 0)).to(dev)
    bx = torch.from_numpy(np.concatenate(boxes, 0)).to(dev) if ub else None
    buf = torch.full((offset + (lead + R + trail) * ldd + 4,), SENT, dtype=torch.float32, device=dev)
    start = offset + lead * ldd
    dst = buf[start:start + R * ldd].view(R, ldd)[:, :W]
    assert dst.data_ptr() % 16 == (4 * start) % 16
    ops.region_rows_build(src, bx, table, torch.from_numpy(table).to(dev), dst, na, ub, nb)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    may = np.zeros(out.shape, dtype=bool)
    for r in range(R):
        may[start + r * ldd:start + r * ldd + W] = True
    rows, r = [], 0
    for k in ks:
        rows.append(np.stack([out[start + (r + j) * ldd:start + (r + j) * ldd + W] for j in range(k)]))
        r += k
    return rows, out, may


@pytest.mark.parametrize('layout', ['aligned', 'one_float_in', 'wide_ld', 'wide_ld_one_float_in'])
@pytest.mark.parametrize('na,nb', BD.FLAGS)
def test_kernel_reproduces_the_reference_rows(dev, na, nb, layout):
    """all 6 images in one launch; every row of every image is checked (order exact, unnormalised columns bit-equal, normalised ones
    within 1e-6 relative), and every element between the rows, in front of and behind the block keeps the sentinel"""
    z = BD.ref()
    atts, boxes = [z['att%d' % i] for i in range(6)], [z['box%d' % i] for i in range(6)]
    hw = np.stack([z['height'], z['width']], 1)
    rows, out, may = _run(dev, atts, boxes, hw, na, 1, nb, offset=1 if 'one_float_in' in layout else 0,
                          extra_ld=7 if 'wide_ld' in layout else 0)
    for i in range(6):
        BD.check_rows(rows[i], na, nb, i, layout)
    assert np.all(out[~may] == np.float32(SENT)), 'wrote outside the rows'
    assert np.all(out[may] != np.float32(SENT))


@pytest.mark.parametrize('D', [4, 5, 1, 8, 67])
@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_kernel_small_widths_and_single_regions(dev, D, offset):
    """K = 1 and K = 3 images at the smallest widths with (D = 4: row of 9) and without (D = 5, D = 1) a 16-byte body in the source,
    at every destination phase, against the loader's numpy path (pinned to the reference by test_use_box_host.py)"""
    sys.path.insert(0, PKG)
    from captioning.data.feature_loader import append_boxes
    rng = np.random.default_rng(100 + D)
    z = BD.ref()
    ks, hw = [1, 3, 1, 2], [(300, 400), (211, 127), (64, 48), (500, 333)]
    atts = [(rng.random((k, D)) + 0.1).astype(np.float32) for k in ks]
    boxes = [z['box5'][:1], z['box5'][1:4] * np.float32(0.2), z['box0'] * np.float32(0.1), z['box1']]
    for na, nb in BD.FLAGS:
        rows, out, may = _run(dev, atts, boxes, np.array(hw), na, 1, nb, offset=offset, extra_ld=2)
        for i, k in enumerate(ks):
            a = atts[i] / np.linalg.norm(atts[i], 2, 1, keepdims=True) if na else atts[i]
            w = append_boxes(a, boxes[i], hw[i][0], hw[i][1], nb)
            got = rows[i]
            for cols, normed in ((slice(0, D), na), (slice(D, D + 5), nb)):
                if normed:
                    assert np.all(np.abs(got[:, cols].astype(np.float64) - w[:, cols]) <= BD.REL * np.abs(w[:, cols])), (D, offset, na, nb, i)
                else:
                    assert np.array_equal(got[:, cols].view(np.int32), w[:, cols].view(np.int32)), (D, offset, na, nb, i)
        assert np.all(out[~may] == np.float32(SENT))


@pytest.mark.parametrize('offset', [0, 1])
def test_kernel_norm_att_alone(dev, offset):
    """use_box 0, norm_att 1: rows of D floats, each over its L2 norm, file order kept; norm_att 0 as well: a plain copy"""
    z = BD.ref()
    atts = [z['att%d' % i] for i in range(6)]
    hw = np.zeros((6, 2), dtype=np.int32)
    rows, out, may = _run(dev, atts, None, hw, 1, 0, 0, offset=offset, extra_ld=3)
    for i in range(6):
        w = atts[i] / np.linalg.norm(atts[i], 2, 1, keepdims=True)
        assert np.all(np.abs(rows[i].astype(np.float64) - w) <= BD.REL * np.abs(w)), i
    assert np.all(out[~may] == np.float32(SENT))
    rows, out, may = _run(dev, atts, None, hw, 0, 0, 0, offset=offset)
    for i in range(6):
        assert np.array_equal(rows[i].view(np.int32), atts[i].view(np.int32))


def test_kernel_nan_keys_go_last_in_file_order(dev):
    """the documented order for keys Python's sorted cannot order: non-NaN keys first, descending; NaN keys behind them, in file order
    (a degenerate box of zeros under norm_box is 0 / 0)"""
    z = BD.ref()
    boxes = z['box5'][:5].copy()
    boxes[1] = 0
    boxes[3] = 0
    att = np.arange(5 * 4, dtype=np.float32).reshape(5, 4) + 1
    rows, _, _ = _run(dev, [att], [boxes], np.array([[512, 768]]), 0, 1, 1)
    got = rows[0]
    assert np.isnan(got[3:, 4:]).all() and not np.isnan(got[:3]).any()
    assert got[3:, 0].tolist() == [att[1, 0], att[3, 0]]
    assert np.all(np.diff(got[:3, -1]) < 0)


def test_wrapper_refuses_rows_outside_its_tensors(dev):
    from imagecaptioning.pytorch_amd import ops, _lib
    src = torch.zeros(4, 8, device=dev)
    bx = torch.zeros(4, 4, device=dev)
    dst = torch.zeros(4, 13, device=dev)
    for t in ([[0, 5, 9, 9]], [[2, 3, 9, 9]], [[0, 3, 9, 9], [2, 2, 9, 9]]):
        th = np.array(t, dtype=np.int32)
        with pytest.raises(_lib.CapmiError):
            ops.region_rows_build(src, bx, th, torch.from_numpy(th).to(dev), dst, 0, 1, 0)
    torch.cuda.synchronize()
    assert not dst.any()


@pytest.mark.parametrize('na,nb', [(0, 0), (1, 1)])
def test_resident_store_equals_the_host_path(dev, tmp_path, na, nb):
    """two passes over the split through ResidentFeatures on the device against FeatureLoader alone (resident_features 0), image by
    image; the budget leaves no room for the last images drawn, which are streamed through the host path; the second pass launches
    the kernel zero times"""
    sys.path.insert(0, PKG)
    from captioning.data.resident import ResidentFeatures
    from imagecaptioning.pytorch_amd import ops
    args = BD.write_dataset(tmp_path) + BD.flag_args(na, nb) + ['--batch_size', '3', '--seq_per_img', '2']
    host = _loader(args)
    res = ResidentFeatures(_loader(args), dev, budget_bytes=(1 + 23) * 29 * 4, first_rows=4)       # room for 23 of the 31 rows
    assert res.device_build
    calls0 = ops.region_rows_build_calls
    calls_after_first = None
    for p in range(2):
        for _ in range(2):
            a, b = host.get_batch('train'), res.get_batch('train')
            assert [i['ix'] for i in a['infos']] == [i['ix'] for i in b['infos']]
            assert b['att_feats'].device.type == 'cuda' and b['att_feats'].shape == a['att_feats'].shape
            assert (a['att_masks'] is None) == (b['att_masks'] is None)
            if a['att_masks'] is not None:
                assert torch.equal(a['att_masks'], b['att_masks'].cpu())
            got, want = b['att_feats'].cpu().numpy(), a['att_feats'].numpy()
            for row, info in enumerate(b['infos']):
                k = BD.KS[info['ix']]
                BD.check_rows(got[row, :k], na, nb, info['ix'], 'resident pass %d' % p)
                assert not got[row, k:].any() and not want[row, k:].any()
            assert np.allclose(b['fc_feats'].cpu().numpy(), a['fc_feats'].numpy(), rtol=1e-5, atol=0)
        if p == 0:
            calls_after_first = ops.region_rows_build_calls
    assert res.streamed >= 1 and len(res.slot) < 6 and len(res.slot) >= 1
    assert calls_after_first > calls0
    assert ops.region_rows_build_calls == calls_after_first, 'the second pass built rows again'
    assert res.rows.shape[1] == 29


def test_att_embed_at_width_29(dev):
    """The prefill at att_feat_size 29 (K = 29 of the forward GEMM is odd, rows are off 16-byte boundaries), 7 regions, B = 3,
    rnn_size 32: att_embed's forward, its weight gradient (grouped launch and one launch each) and the input-gradient product
    dY W, against float64 linear + relu.  The bound is the one test_gemm_routes_gpu.test_gemm_route_vs_float64 holds every route to:
    max |out - ref64| / mag <= 1.5 x the same measure of torch's fp32 evaluation + 1e-7, mag the formula on absolute values."""
    from imagecaptioning.pytorch_amd import engine_common as E, ops
    g = torch.Generator().manual_seed(29)
    B, K, F, R, A = 3, 7, 29, 32, 16
    P = {'att_embed.0.weight': torch.randn(R, F, generator=g) * 0.3, 'att_embed.0.bias': torch.randn(R, generator=g) * 0.1,
         'ctx2att.weight': torch.randn(A, R, generator=g) * 0.3, 'ctx2att.bias': torch.randn(A, generator=g) * 0.1}
    P = {k: v.to(dev).contiguous() for k, v in P.items()}
    x = torch.randn(B, K, F, generator=g).to(dev)
    W, b = P['att_embed.0.weight'], P['att_embed.0.bias']
    x2 = x.view(B * K, F)

    def held(out, ref, mag, f32, what):
        e_ours, e_f32 = G.measure(out, ref, mag), G.measure(f32, ref, mag)
        print('att_embed_29 %s e_ours=%.3e e_fp32=%.3e' % (what, e_ours, e_f32))
        assert e_ours <= 1.5 * e_f32 + 1e-7, (what, e_ours, e_f32)

    pr = E.prepare(P, None, x, None)
    torch.cuda.synchronize()
    ref = torch.relu(x2.double() @ W.double().t() + b.double())
    mag = x2.double().abs() @ W.double().abs().t() + b.double().abs()
    held(pr.att.view(B * K, R), ref, mag, torch.relu(torch.nn.functional.linear(x2, W, b)), 'forward')
    for group in (True, False):
        grads = {k: torch.full_like(v, 7.0) for k, v in P.items()}
        d_att = torch.randn(B, K, R, generator=g).to(dev)
        d_p = torch.randn(B, K, A, generator=g).to(dev)
        d_pre, _, _ = E.prepare_backward(P, pr, None, d_att, d_p, grads, group=group)
        torch.cuda.synchronize()
        assert bool((d_pre != 0).any())
        held(grads['att_embed.0.weight'], d_pre.double().t() @ x2.double(), d_pre.double().abs().t() @ x2.double().abs(),
             d_pre.t() @ x2, 'dW group=%d' % group)
    dx = torch.full((B * K, F), 7.0, device=dev)
    ops.gemm([(d_pre, R, W, F, R, 1)], B * K, F, dx, a_layout=0, b_layout=1)
    torch.cuda.synchronize()
    held(dx, d_pre.double() @ W.double(), d_pre.double().abs() @ W.double().abs(), d_pre @ W, 'dX')


def test_train_with_boxes_runs_and_checkpoints(tmp_path):
    """2 iterations of UpDown XE with --use_box 1 --norm_box_feat 1 --att_feat_size 29 on the tiny dataset write a checkpoint; the same
    command with --att_feat_size 24 stops at start-up and names both widths"""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import rewards
    rewards.reset_scorer()
    args = BD.write_dataset(tmp_path)[:-4] + ['--caption_model', 'updown', '--rnn_size', '32', '--input_encoding_size', '32',
                                               '--att_hid_size', '16', '--fc_feat_size', '29', '--batch_size', '3', '--seq_per_img', '2',
                                               '--losses_log_every', '1000', '--max_iters', '2', '--save_checkpoint_every', '2',
                                               '--use_box', '1', '--norm_box_feat', '1', '--checkpoint_path', str(tmp_path / 'ck')]
    loss = T.train(_opts(args + ['--att_feat_size', '29']))
    torch.cuda.synchronize()
    assert loss == loss
    assert os.path.exists(tmp_path / 'ck' / 'model.pth')
    sd = torch.load(tmp_path / 'ck' / 'model.pth', map_location='cpu')
    assert sd['att_embed.0.weight'].shape == (32, 29)
    with pytest.raises(ValueError, match=r'width 29 .*att_feat_size is 24'):
        T.train(_opts(args + ['--att_feat_size', '24']))
    rewards.reset_scorer()
