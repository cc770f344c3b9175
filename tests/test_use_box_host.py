"""use_box / norm_box_feat / input_box_dir, host side: FeatureLoader's numpy path against the reference's own rows
(tests/golden/box_ref.npz, written by make_box_golden.py from captioning/data/dataloader.py:262-299), the loader's refusals, the
batch contract at width D + 5, the start-up check of the tools, and the C ABI of capmi_region_rows_build."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import box_ds as BD
from conftest import ROOT

PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
HEADER = os.path.join(ROOT, 'include', 'capmi.h')


def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


def _loader(argv):
    sys.path.insert(0, PKG)
    from captioning.data.feature_loader import FeatureLoader
    return FeatureLoader(_opts(argv), workers=2, processes=False)


def test_fixture_is_what_the_issue_asks_for():
    """6 images, K = 1, 2, 5, 7, 7, 9, D = 24, distinct height != width; an exact tie, a descending and an ascending image"""
    z = BD.ref()
    assert tuple(z['att%d' % i].shape[0] for i in range(6)) == BD.KS == (1, 2, 5, 7, 7, 9)
    assert all(z['att%d' % i].shape == (BD.KS[i], 24) and z['box%d' % i].shape == (BD.KS[i], 4) for i in range(6))
    assert all(z['height'] != z['width']) and len(set(zip(z['height'], z['width']))) == 6
    assert np.array_equal(z['box2'][1], z['box2'][3]) and not np.array_equal(z['att2'][1], z['att2'][3])
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])                            # noqa: E731
    assert np.all(np.diff(area(z['box3'])) < 0) and np.all(np.diff(area(z['box4'])) > 0)
    # the tie is decided by file order: row 1 stands directly in front of row 3
    w = BD.want(0, 0, 2)
    pos = {j: int(np.where((w[:, :24] == z['att2'][j]).all(1))[0][0]) for j in (1, 3)}
    assert pos[3] == pos[1] + 1


@pytest.mark.parametrize('na,nb', BD.FLAGS)
def test_feature_loader_reproduces_the_reference_rows(tmp_path, na, nb):
    ld = _loader(BD.write_dataset(tmp_path) + BD.flag_args(na, nb) + ['--batch_size', '6', '--seq_per_img', '2'])
    assert ld.att_feat_width() == 29
    for i in range(BD.N_IMG):
        fc, att = ld._image(i)
        BD.check_rows(att, na, nb, i, 'host')
        ref_fc = BD.ref()['fc.a%d.b%d.%d' % (na, nb, i)]                                  # no fc file: the mean of the built rows
        assert fc.shape == (29,) and np.allclose(fc, ref_fc, rtol=1e-5, atol=0)
    # the batch contract is the old one, 5 columns wider: zero padding rows, the mask
    b = ld.get_batch('train')
    att, m = b['att_feats'].numpy(), b['att_masks'].numpy()
    assert att.shape == (6, 9, 29) and m.shape == (6, 9) and b['fc_feats'].shape == (6, 29)
    for row, info in enumerate(b['infos']):
        i = info['ix']
        BD.check_rows(att[row, :BD.KS[i]], na, nb, i, 'batch')
        assert not att[row, BD.KS[i]:].any() and m[row].tolist() == [1.0] * BD.KS[i] + [0.0] * (9 - BD.KS[i])


def test_boxes_in_npz_files_and_a_cpu_store_give_the_same_rows(tmp_path):
    """input_box_dir takes the store kinds input_att_dir takes (<id>.npz with `feat`, or <id>.npy); a ResidentFeatures store on the
    CPU has no device to build rows on and keeps the numpy path"""
    sys.path.insert(0, PKG)
    from captioning.data.resident import ResidentFeatures
    args = BD.write_dataset(tmp_path, box_ext='.npz') + BD.flag_args(1, 1) + ['--batch_size', '6', '--seq_per_img', '2']
    res = ResidentFeatures(_loader(args), 'cpu', first_rows=8)
    assert not res.device_build
    for _ in range(2):
        b = res.get_batch('train')
        for row, info in enumerate(b['infos']):
            BD.check_rows(b['att_feats'][row, :BD.KS[info['ix']]].numpy(), 1, 1, info['ix'], 'cpu store')
    assert res.rows.shape[1] == 29


def test_use_box_0_reads_no_box_and_keeps_the_rows(tmp_path):
    args = BD.write_dataset(tmp_path, hw=False)
    ld = _loader(args + ['--batch_size', '6', '--seq_per_img', '2', '--input_box_dir', str(tmp_path / 'nowhere')])
    for i in range(BD.N_IMG):
        assert np.array_equal(ld._image(i)[1], BD.ref()['att%d' % i])
    ld.check_att_feat_size(2048)                                  # only a use_box run is checked: nothing changes without it


def test_loader_refuses_what_it_cannot_build(tmp_path):
    base = ['--batch_size', '6', '--seq_per_img', '2'] + BD.flag_args(0, 0)
    args = BD.write_dataset(tmp_path / 'a')
    with pytest.raises(ValueError, match='input_box_dir'):
        _loader(args + base + ['--input_box_dir', str(tmp_path / 'a' / 'no_such_dir')])
    with pytest.raises(ValueError, match='input_box_dir'):
        _loader(args + base + ['--input_box_dir', ''])
    with pytest.raises(ValueError, match="'height'.*image 500"):
        _loader(BD.write_dataset(tmp_path / 'b', hw=False) + base)
    ld = _loader(BD.write_dataset(tmp_path / 'c', drop_box_row_of=4) + base)
    ld._image(3)
    with pytest.raises(ValueError, match=r'image 504.*\(6, 4\).*7 regions'):
        ld._image(4)
    info = json.load(open(tmp_path / 'a' / 'd.json'))
    info['images'][2]['width'] = 0
    json.dump(info, open(tmp_path / 'a' / 'd.json', 'w'))
    with pytest.raises(ValueError, match="'width'.*image 502"):
        _loader(args + base)


def test_att_feat_size_is_checked_at_start_up(tmp_path):
    """tools/train.py and tools/eval.py call check_att_feat_size right after they build the loader; both numbers are named"""
    ld = _loader(BD.write_dataset(tmp_path) + BD.flag_args(0, 1) + ['--batch_size', '6', '--seq_per_img', '2'])
    ld.check_att_feat_size(29)
    with pytest.raises(ValueError, match=r'width 29 .*att_feat_size is 24'):
        ld.check_att_feat_size(24)
    for tool in ('train.py', 'eval.py'):
        assert 'loader.check_att_feat_size(' in open(os.path.join(PKG, 'tools', tool)).read(), tool


def test_box_columns_restate_the_five_lines(tmp_path):
    """box_columns (the host path, and the documentation of what the kernel computes) in float32, operation by operation"""
    sys.path.insert(0, PKG)
    from captioning.data.feature_loader import box_columns
    z = BD.ref()
    for i in range(BD.N_IMG):
        h, w = int(z['height'][i]), int(z['width'][i])
        x1, y1, x2, y2 = np.hsplit(z['box%d' % i], 4)
        ref = np.hstack((x1 / w, y1 / h, x2 / w, y2 / h, (x2 - x1) * (y2 - y1) / (w * h)))     # dataloader.py:277, verbatim
        assert ref.dtype == np.float32
        assert np.array_equal(box_columns(z['box%d' % i], h, w).view(np.int32), ref.view(np.int32))


def test_region_rows_prototype_matches_the_binding():
    from imagecaptioning.pytorch_amd import _lib, ops
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    d = {m.group(1): len(m.group(2).split(',')) for m in re.finditer(r'\bint\s*(capmi_region_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S)}
    assert d == {'capmi_region_rows_build': 12}
    assert len(_lib.SIGNATURES['capmi_region_rows_build']) == 12
    assert int(re.search(r'#define CAPMI_REGION_KMAX (\d+)', src).group(1)) == ops.REGION_KMAX
    assert 'region_rows.hip' in [os.path.basename(s) for s in __import__('imagecaptioning.pytorch_amd.build', fromlist=['x']).sources()]


def test_region_rows_invalid_arguments_are_einval():
    """NULL pointers, K <= 0, D <= 0, height / width <= 0 with use_box, a leading dimension below the row: CAPMI_EINVAL before anything
    is launched (no device is touched: the checks come first, the pointers are host memory)"""
    from imagecaptioning.pytorch_amd import _lib
    fn = _lib.lib.capmi_region_rows_build
    buf = (C.c_float * 64)()
    a = C.addressof(buf)

    def table(first=0, K=2, h=10, w=20):
        return (C.c_int32 * 4)(first, K, h, w)

    def call(t, **kw):
        p = dict(src=a, boxes=a, th=C.addressof(t), td=a, n=1, D=4, dst=a, ldd=9, na=1, ub=1, nb=1)
        p.update(kw)
        return fn(p['src'], p['boxes'], p['th'], p['td'], p['n'], p['D'], p['dst'], p['ldd'], p['na'], p['ub'], p['nb'], None)

    t = table()
    for kw in (dict(src=None), dict(boxes=None), dict(th=None), dict(td=None), dict(dst=None), dict(n=0), dict(n=-1), dict(D=0),
               dict(D=-4), dict(ldd=8), dict(ldd=3, ub=0), dict(dst=a + 2)):
        assert call(t, **kw) == _lib.EINVAL, kw
    for bad in (table(K=0), table(K=-3), table(h=0), table(w=0), table(h=-5), table(first=-1), table(K=1025)):
        assert call(bad) == _lib.EINVAL, list(bad)
