"""The compact resident feature store on the device (csrc/resident.hip): capmi_rows_narrow against torch's own conversion bit for bit,
capmi_rows_l2norm against numpy's row norm bit for bit, capmi_resident_gather against index_select + the numpy mask bit for bit, the
store end to end per dtype, and tools/train.py with --resident_dtype bf16."""
import os
import sys

import numpy as np
import pytest
import torch

import box_ds as BD
from conftest import ROOT
from test_feature_loader import make_dataset

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
SENT16 = 0x5a5a                                     # what a 16-bit destination holds before the launch


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


def _loader(argv):
    sys.path.insert(0, PKG)
    from captioning.data.feature_loader import FeatureLoader
    return FeatureLoader(_opts(argv), workers=2, processes=False)


def _store(argv, device, dtype='fp32', **kw):
    sys.path.insert(0, PKG)
    from captioning.data.resident import ResidentFeatures
    return ResidentFeatures(_loader(argv), device, dtype=dtype, **kw)


# ---- narrow ------------------------------------------------------------------------------------------------------------------------
def _specials():
    f = np.float32
    up = lambda x: np.nextafter(f(x), f(np.inf))                 # noqa: E731
    down = lambda x: np.nextafter(f(x), f(-np.inf))              # noqa: E731
    pos = [0.0, np.inf, 65504.0, up(65504.0), down(65520.0), 65520.0, up(65520.0), 3.4028235e38, 3.3895314e38, up(3.3895314e38),
           # halfway cases of bf16 (8 significant bits) in both directions, and their neighbours
           1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, up(1 + 2.0 ** -8), down(1 + 2.0 ** -8), up(1 + 3 * 2.0 ** -8), down(1 + 3 * 2.0 ** -8),
           # ... of fp16 (11 significant bits)
           1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, up(1 + 2.0 ** -11), down(1 + 2.0 ** -11), up(1 + 3 * 2.0 ** -11), down(1 + 3 * 2.0 ** -11),
           # fp16 subnormals (multiples of 2^-24), their halfway cases, the smallest normal, and values below the smallest subnormal
           2.0 ** -14, down(2.0 ** -14), 2.0 ** -15, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, up(2.0 ** -25), down(2.0 ** -25), 3 * 2.0 ** -25,
           5 * 2.0 ** -25, up(3 * 2.0 ** -25), 1023.5 * 2.0 ** -24, 2.0 ** -26, 1e-8, 1e-30, 1e-40, 1.1754944e-38]
    v = np.array(pos, dtype=np.float32)
    v = np.concatenate([v, -v])
    nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fbfffff, 0x7f80ffff], dtype=np.uint32).view(np.float32)
    return np.concatenate([v, nan])


def _same_bits_nan_as_a_class(got, want):
    g, w = got.view(torch.int16).cpu().numpy(), want.view(torch.int16).cpu().numpy()
    gn, wn = torch.isnan(got).cpu().numpy(), torch.isnan(want).cpu().numpy()
    return np.array_equal(gn, wn) and np.array_equal(g[~wn], w[~wn])


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_narrow_is_torchs_conversion_bit_for_bit(dev, dtype):
    """counts 1, 3, 4, 7, 4099 at destination offsets of 0..3 elements (and a source 0 / 1 float off its 16 bytes): every element equals
    src.to(dtype) on the same device as int16, NaN as a class; nothing outside the destination is written"""
    from imagecaptioning.pytorch_amd import ops
    sp = _specials()
    rng = np.random.default_rng(7)
    for count in (1, 3, 4, 7, 4099):
        if count < len(sp):                                        # a draw of the special values (each of them alone: the test below)
            vals = sp[rng.permutation(len(sp))[:count]]
        else:                                                      # all of them, then values of every magnitude fp16 tells apart
            more = count - len(sp)
            vals = np.concatenate([sp, (rng.standard_normal(more) * 10.0 ** rng.integers(-9, 6, more)).astype(np.float32)])
        for off in (0, 1, 2, 3):
            for soff in (0, 1):
                sbuf = torch.zeros(count + 4, dtype=torch.float32, device=dev)
                src = sbuf[soff:soff + count]
                src.copy_(torch.from_numpy(vals))
                buf = torch.full((count + 24,), SENT16, dtype=torch.int16, device=dev).view(TORCH[dtype])
                dst = buf[off:off + count]
                assert dst.data_ptr() % 16 == 2 * off and src.data_ptr() % 16 == 4 * soff
                ops.rows_narrow(src, dst)
                torch.cuda.synchronize()
                assert _same_bits_nan_as_a_class(dst, src.to(TORCH[dtype])), (dtype, count, off, soff)
                raw = buf.view(torch.int16)
                assert bool((raw[:off] == SENT16).all()) and bool((raw[off + count:] == SENT16).all()), (dtype, count, off, soff)


def test_narrow_every_special_value_alone(dev):
    """each special value converted on its own at every destination phase (a head, a body or a tail element depending on the phase)"""
    from imagecaptioning.pytorch_amd import ops
    sp = torch.from_numpy(_specials()).to(dev)
    for dtype in ('bf16', 'fp16'):
        for off in range(8):
            buf = torch.zeros(len(sp) + 16, dtype=TORCH[dtype], device=dev)
            ops.rows_narrow(sp, buf[off:off + len(sp)])
            assert _same_bits_nan_as_a_class(buf[off:off + len(sp)], sp.to(TORCH[dtype])), (dtype, off)


# ---- norm_att_feat on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 5, 7, 8, 9, 24, 29, 67, 128, 129, 131, 300, 2048, 2053, 8192])
def test_l2norm_is_numpys_bit_for_bit(dev, D):
    """rows over their L2 norm against att / np.linalg.norm(att, 2, 1, keepdims=True) (feature_loader.finish_image), as int32: below 8
    elements, one run with and without a tail, the first split (129), splits whose halves have tails, the COCO widths and the widest
    row the kernel takes; the block starts 0 and 1 floats off a 16-byte boundary; post-ReLU rows (half zeros) and a zero row (NaN)"""
    from imagecaptioning.pytorch_amd import ops
    rng = np.random.default_rng(D)
    n = 7
    x = np.clip(rng.standard_normal((n, D)), 0, None).astype(np.float32) * np.float32(3) + np.float32(1e-3)
    x[3] = rng.standard_normal(D).astype(np.float32) * np.float32(1e3)
    x[5] = 0
    with np.errstate(invalid='ignore', divide='ignore'):
        want = x / np.linalg.norm(x, 2, 1, keepdims=True)
    assert np.isnan(want[5]).all()
    for off in (0, 1):
        buf = torch.full((off + n * D + 5,), -7.0, device=dev)
        rows = buf[off:off + n * D].view(n, D)
        rows.copy_(torch.from_numpy(x))
        ops.rows_l2norm(rows)
        got = buf.cpu().numpy()
        g = got[off:off + n * D].reshape(n, D)
        assert np.isnan(g[5]).all(), (D, off)
        keep = np.arange(n) != 5
        assert np.array_equal(g[keep].view(np.int32), want[keep].view(np.int32)), (D, off, float(np.abs(g[keep] - want[keep]).max()))
        assert (got[:off] == -7).all() and (got[off + n * D:] == -7).all()


# ---- gather ------------------------------------------------------------------------------------------------------------------------
def _ksets(B, kmax):
    """all equal to kmax; ragged; one image with K = 0"""
    ragged = [max(1, kmax - 2 * b - 1) for b in range(B)]
    ragged[-1] = kmax
    zero = list(ragged)
    zero[0] = 0
    return [[kmax] * B, ragged, zero]


def _make_store(dev, dtype, n, F, off, seed):
    """a store of n rows whose first element stands `off` elements into its allocation; row 0 is the zero row"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(n, F, generator=g) * 3
    vals[torch.rand(n, F, generator=g) < 0.1] = -0.0
    vals[torch.rand(n, F, generator=g) < 0.05] = float('inf')
    if dtype == 'fp16':
        vals[torch.rand(n, F, generator=g) < 0.1] = 3 * 2.0 ** -24          # an fp16 subnormal
    vals[0] = 0
    buf = torch.zeros(off + n * F + 8, dtype=TORCH[dtype], device=dev)
    rows = buf[off:off + n * F].view(n, F)
    rows.copy_(vals.to(TORCH[dtype]))
    return rows


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('F', [5, 8, 13, 16])
def test_gather_equals_index_select_and_the_numpy_mask(dev, dtype, F):
    """B in {1, 3} x kmax in {1, 7} x the three K sets, the store 0, 1 and 3 elements off a 16-byte boundary and every image at an odd
    first row: att is bit-equal to index_select through the zero row (of rows.float() at 16 bits), the padding is exactly +0.0 although
    the store row behind every image is NaN, the mask is the numpy mask"""
    from imagecaptioning.pytorch_amd import ops
    for off in (0, 1, 3):
        for B in (1, 3):
            for kmax in (1, 7):
                for ks in _ksets(B, kmax):
                    n = 2 + B * (kmax + 3)
                    rows = _make_store(dev, dtype, n, F, off, seed=F * 100 + B * 10 + kmax)
                    assert rows.data_ptr() % 16 == (off * rows.element_size()) % 16
                    table = np.zeros((B, 2), dtype=np.int32)
                    gather = np.zeros((B, kmax), dtype=np.int64)
                    mask = np.zeros((B, kmax), dtype=np.float32)
                    r = 1
                    for b, k in enumerate(ks):
                        r += 1 - (r % 2) if k else 0                       # an odd first row
                        table[b] = (r, k) if k else (0, 0)
                        gather[b, :k] = np.arange(r, r + k)
                        mask[b, :k] = 1
                        if k:
                            rows[r + k] = float('nan')                     # the row behind the image
                            r += k + 1
                    want = rows.float().index_select(0, torch.from_numpy(gather.reshape(-1)).to(dev)).view(B, kmax, F)
                    att, m = ops.resident_gather(rows, table, torch.from_numpy(table).to(dev), kmax)
                    torch.cuda.synchronize()
                    tag = (dtype, F, off, B, kmax, ks)
                    assert att.dtype == torch.float32 and att.shape == (B, kmax, F) and m.shape == (B, kmax)
                    assert torch.equal(att.view(torch.int32), want.view(torch.int32)), tag
                    assert np.array_equal(m.cpu().numpy(), mask), tag
                    pad = att.view(torch.int32)[torch.from_numpy(mask == 0).to(dev)]
                    assert bool((pad == 0).all()), tag                      # +0.0, bit for bit


def test_gather_invalid_arguments_are_einval_and_write_nothing(dev):
    from imagecaptioning.pytorch_amd import ops, _lib
    rows = torch.ones(12, 8, dtype=torch.bfloat16, device=dev)
    att = torch.full((2, 3, 8), 7.0, device=dev)
    mask = torch.full((2, 3), 7.0, device=dev)
    good = np.array([[1, 3], [5, 2]], dtype=np.int32)
    tab = torch.from_numpy(good).to(dev)
    fn = _lib.lib.capmi_resident_gather

    def call(rows_p=rows.data_ptr(), dtype=_lib.ROWS_BF16, F=8, th=good, t=tab.data_ptr(), B=2, kmax=3, a=att.data_ptr(), m=mask.data_ptr()):
        return fn(rows_p, dtype, F, None if th is None else th.ctypes.data, t, B, kmax, a, m, _lib.stream_ptr())

    for kw in (dict(rows_p=None), dict(th=None), dict(t=None), dict(a=None), dict(m=None), dict(B=0), dict(B=-2), dict(kmax=0), dict(kmax=-1),
               dict(F=0), dict(F=-8), dict(dtype=3), dict(dtype=-1), dict(kmax=2), dict(th=np.array([[1, 4], [5, 2]], dtype=np.int32)),
               dict(th=np.array([[1, -1], [5, 2]], dtype=np.int32)), dict(th=np.array([[-1, 3], [5, 2]], dtype=np.int32))):
        assert call(**kw) == _lib.EINVAL, kw
    for bad in ([[1, 4], [5, 2]], [[10, 3], [5, 2]], [[1, 3], [-1, 2]]):       # the wrapper also knows the store's size
        th = np.array(bad, dtype=np.int32)
        with pytest.raises(_lib.CapmiError):
            ops.resident_gather(rows, th, torch.from_numpy(th).to(dev), 3)
    f = _lib.lib.capmi_rows_narrow
    src = torch.ones(8, device=dev)
    dst = torch.zeros(8, dtype=torch.bfloat16, device=dev)
    for a in ((None, dst.data_ptr(), 8, _lib.ROWS_BF16), (src.data_ptr(), None, 8, _lib.ROWS_BF16), (src.data_ptr(), dst.data_ptr(), 0, _lib.ROWS_BF16),
              (src.data_ptr(), dst.data_ptr(), 8, _lib.ROWS_F32), (src.data_ptr(), dst.data_ptr(), 8, 7)):
        assert f(*a, _lib.stream_ptr()) == _lib.EINVAL, a
    torch.cuda.synchronize()
    assert bool((att == 7).all()) and bool((mask == 7).all()) and not dst.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((att[0] == 1).all()) and bool((att[1, :2] == 1).all()) and not att[1, 2].any()


# ---- the store, end to end -----------------------------------------------------------------------------------------------------------
ARGS = ['--batch_size', '4', '--seq_per_img', '3']


def _same_batch(x, y, what, convert=None):
    want = (x['att_feats'] if convert is None else x['att_feats'].to(convert).float()).cpu()
    assert y['att_feats'].is_cuda and y['att_feats'].dtype == torch.float32
    assert torch.equal(want.view(torch.int32), y['att_feats'].cpu().view(torch.int32)), (what, 'att_feats')
    assert torch.equal(x['fc_feats'].cpu(), y['fc_feats'].cpu()), (what, 'fc_feats')
    assert (x['att_masks'] is None) == (y['att_masks'] is None), what
    if x['att_masks'] is not None:
        assert torch.equal(x['att_masks'].cpu(), y['att_masks'].cpu()), (what, 'att_masks')
        assert x['att_masks']._capmi_kmax == y['att_masks']._capmi_kmax
    assert torch.equal(x['labels'], y['labels']) and x['infos'] == y['infos'] and x['bounds'] == y['bounds']


@pytest.fixture(scope='module')
def plain(tmp_path_factory):
    """the ragged set (odd images have no fc file) and the unchanged CPU-device torch path's fp32 batches over two epochs, computed once"""
    tmp = tmp_path_factory.mktemp('compact_gpu')
    args = make_dataset(tmp, n_img=13) + ARGS
    cpu = _store(args, 'cpu', first_rows=8)
    n_train = len(cpu.split_ix['train'])
    per_epoch = (n_train + 3) // 4
    return args, [cpu.get_batch('train') for _ in range(2 * per_epoch + 1)], n_train, per_epoch


@pytest.mark.parametrize('fixed', [None, 6])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
def test_device_store_equals_the_cpu_torch_path(dev, plain, tmp_path, dtype, fixed):
    """fp32: bit-equal to the CPU-device store; 16 bits: to those batches rounded once.  One launch per batch, and the second epoch
    decodes nothing."""
    from imagecaptioning.pytorch_amd import ops
    if fixed is None:
        args, want, n_train, per_epoch = plain
    else:                                                          # every image has 6 regions: no att_masks
        args = make_dataset(tmp_path, fixed_regions=fixed) + ARGS
        cpu = _store(args, 'cpu', first_rows=8)
        n_train = len(cpu.split_ix['train'])
        per_epoch = (n_train + 3) // 4
        want = [cpu.get_batch('train') for _ in range(2 * per_epoch + 1)]
        assert all(w['att_masks'] is None for w in want)
    res = _store(args, dev, dtype, first_rows=8)
    calls0 = ops.resident_gather_calls
    for it, x in enumerate(want):
        if it == per_epoch + 1:
            misses = res.misses
        _same_batch(x, res.get_batch('train'), (dtype, it), None if dtype == 'fp32' else TORCH[dtype])
    assert ops.resident_gather_calls == calls0 + len(want)
    assert res.misses == misses == n_train and res.streamed == 0, 'the second epoch decoded an image again'
    assert res.rows.dtype == TORCH[dtype] and res.fc.dtype == torch.float32


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_device_store_with_streamed_images(dev, plain, dtype):
    """a budget of 20 rows at this dtype: the images that do not fit are copied into the gathered block by the host, and their mask
    rows come from the host-known K"""
    args, want, n_train, per_epoch = plain
    res = _store(args, dev, dtype, first_rows=8, budget_bytes=20 * 24 * (4 if dtype == 'fp32' else 2))
    for it, x in enumerate(want):
        y = res.get_batch('train')
        if dtype == 'fp32':
            _same_batch(x, y, (dtype, it))
        else:                                                      # resident rows are rounded, streamed rows arrive as the files hold them
            a, r = y['att_feats'].cpu(), x['att_feats']
            for b, info in enumerate(x['infos']):
                w = r[b].to(torch.bfloat16).float() if info['ix'] in res.slot else r[b]
                assert torch.equal(a[b].view(torch.int32), w.view(torch.int32)), (it, b)
            assert torch.equal(x['att_masks'].cpu(), y['att_masks'].cpu()) if x['att_masks'] is not None else y['att_masks'] is None
    assert res.streamed > 0 and 0 < len(res.slot) < n_train and res.used <= 20


BUILT = [(0, 1, 0), (1, 0, 0), (1, 1, 1)]                 # (norm_att_feat, use_box, norm_box_feat): the rows are built by the device


def _built_args(tmp_path, na, ub, nb):
    args = BD.write_dataset(tmp_path) + ['--use_box', str(ub), '--norm_att_feat', str(na), '--norm_box_feat', str(nb),
                                          '--batch_size', '3', '--seq_per_img', '2']
    if not ub:
        args[args.index('--att_feat_size') + 1] = args[args.index('--fc_feat_size') + 1] = str(BD.D)
    return args


@pytest.mark.parametrize('na,ub,nb', BUILT)
def test_device_built_store_per_dtype(dev, tmp_path, na, ub, nb):
    """norm_att_feat / use_box, two passes over the 6 images: the fp32 batch is bit-equal to index_select over the device-built store
    (the gather adds nothing to what capmi_region_rows_build wrote), and stands within the bound test_use_box_gpu.py holds the build
    to (box_ds.REL) of the loader's host path; bf16 / fp16 batches equal the fp32 batches rounded once -- the build goes through the
    fp32 staging block --, and fc (the mean of the fp32 rows: the set has no fc files) is bit-equal to the fp32 store's."""
    args = _built_args(tmp_path, na, ub, nb)
    host = _loader(args)
    stores = {d: _store(args, dev, d, first_rows=4) for d in ('fp32', 'bf16', 'fp16')}
    assert all(s.device_build for s in stores.values())
    for it in range(4):
        a = host.get_batch('train')
        got = {d: s.get_batch('train') for d, s in stores.items()}
        for d in ('bf16', 'fp16'):
            _same_batch(got['fp32'], got[d], (d, it), TORCH[d])
        res, y = stores['fp32'], got['fp32']['att_feats']
        gather = np.zeros(y.shape[:2], dtype=np.int64)
        for b, info in enumerate(a['infos']):
            r0, k = res.slot[info['ix']]
            gather[b, :k] = np.arange(r0, r0 + k)
        want = res.rows.index_select(0, torch.from_numpy(gather.reshape(-1)).to(dev)).view(y.shape)
        assert torch.equal(want.view(torch.int32), y.view(torch.int32)), it
        x = a['att_feats'].double()
        assert bool(((y.cpu().double() - x).abs() <= BD.REL * x.abs()).all()), it
        assert (a['att_masks'] is None) == (got['fp32']['att_masks'] is None)
        if a['att_masks'] is not None:
            assert torch.equal(a['att_masks'], got['fp32']['att_masks'].cpu())
    assert all(s.misses == BD.N_IMG and s.streamed == 0 for s in stores.values())
    assert all(s.rows.shape[1] == BD.D + 5 * ub for s in stores.values())


@pytest.mark.parametrize('na,ub,nb', BUILT)
def test_device_built_fp32_batches_equal_finish_image_on_the_host(dev, tmp_path, na, ub, nb):
    """norm_att_feat / use_box: fp32 batches of the device store against ld.finish_image applied on the host (the loader alone), bit
    for bit.  The geometry columns and the row order are capmi_region_rows_build's; norm_att_feat is applied to the staged rows by
    capmi_rows_l2norm, which sums the squares in numpy's order (the build kernel's own norm, a wave-order sum, stands one unit in the
    last place off the host path for some rows: measured 5.96e-08 on features near 0.5)."""
    args = _built_args(tmp_path, na, ub, nb)
    host, res = _loader(args), _store(args, dev, 'fp32', first_rows=4)
    pairs = [(host.get_batch('train'), res.get_batch('train')) for _ in range(4)]
    worst = max(float((a['att_feats'].double() - b['att_feats'].cpu().double()).abs().max()) for a, b in pairs)
    print('device build vs finish_image norm_att_feat=%d use_box=%d norm_box_feat=%d: max |diff| = %.3e' % (na, ub, nb, worst))
    for it, (a, b) in enumerate(pairs):
        assert torch.equal(a['att_feats'].view(torch.int32), b['att_feats'].cpu().view(torch.int32)), (it, worst)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
def test_train_with_a_bf16_store_runs_and_resumes(tmp_path):
    """tools/train.py --resident_dtype bf16: two iterations of UpDown XE on the tiny ragged set, a checkpoint, two more from --start_from"""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import rewards
    rewards.reset_scorer()
    data = tmp_path / 'data'
    data.mkdir()
    args = make_dataset(data, n_img=12) + ['--caption_model', 'updown', '--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16',
                                           '--batch_size', '4', '--seq_per_img', '3', '--losses_log_every', '1000', '--learning_rate', '0.01',
                                           '--checkpoint_path', str(tmp_path / 'ck'), '--resident_dtype', 'bf16', '--save_checkpoint_every', '2']
    l0 = T.train(_opts(args + ['--max_iters', '2']))
    assert np.isfinite(l0) and os.path.exists(tmp_path / 'ck' / 'model.pth')
    l1 = T.train(_opts(args + ['--max_iters', '4', '--start_from', str(tmp_path / 'ck')]))
    torch.cuda.synchronize()
    assert np.isfinite(l1)
    rewards.reset_scorer()
