#!/usr/bin/env python3
"""Golden region rows of the REFERENCE's own ``Dataset.__getitem__`` (captioning/data/dataloader.py:262-299) with ``use_box 1``:
what pins the host path of captioning/data/feature_loader.py and the device path (csrc/region_rows.hip) to the reference's box
geometry, normalisation and row order.

Run only where the reference is at hand (the tests need only the .npz this writes):

    CAPMI_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_box_golden.py

Writes tests/golden/box_ref.npz: the inputs (``att<i>`` [K, 24] and ``box<i>`` [K, 4] float32, ``height`` / ``width`` [6]) and, for
norm_att_feat a and norm_box_feat b in {0, 1}, the reference's ``att_feat`` of every image as ``want.a<a>.b<b>.<i>`` [K, 29] plus
its ``fc_feat`` (no fc file: the mean of those rows) as ``fc.a<a>.b<b>.<i>``.

The 6 images have K = 1, 2, 5, 7, 7, 9 regions and distinct height != width.  Image 2 holds two IDENTICAL boxes with different
features (an exact tie: only the stable order decides), image 3's boxes stand in descending order of area, image 4's in ascending
order.  Every other pair of keys of an image differs by more than 1e-3 relative, in the plain and in the normalised area (asserted
below in float64), so float32 rounding of a norm cannot legitimately reorder rows: the reference's row order is the only right one.

``h5py`` and ``lmdbdict`` are imported by the reference module and not installed here; they are stubbed as in
make_loader_golden.py (no label file and no lmdb store is read: input_label_h5 'none', directories of .npy / .npz files)."""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get('CAPMI_REFERENCE', '')             # a checkout of the reference (ImageCaptioning.pytorch)
HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 2, 5, 7, 7, 9)
D = 24
SIZES = ((480, 640), (375, 500), (427, 641), (333, 512), (600, 399), (512, 768))      # (height, width)
TIE, DESC, ASC = 2, 3, 4


def keys64(boxes, h, w):
    """plain and normalised area of every box, in float64"""
    b = boxes.astype(np.float64)
    col = np.stack([b[:, 0] / w, b[:, 1] / h, b[:, 2] / w, b[:, 3] / h, (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) / (w * h)], 1)
    return col[:, 4], col[:, 4] / np.linalg.norm(col, 2, 1)


def separated(k):
    k = np.sort(k)
    return bool(np.all(np.diff(k) > 1e-3 * np.abs(k[1:])))


def draw_boxes(rng, K, h, w, same_order):
    """K boxes inside a w x h image whose plain and normalised areas are separated (and, same_order, ranked alike)"""
    while True:
        x1, y1 = rng.uniform(0, 0.6 * w, K), rng.uniform(0, 0.6 * h, K)
        x2, y2 = x1 + rng.uniform(0.05 * w, 0.4 * w, K), y1 + rng.uniform(0.05 * h, 0.4 * h, K)
        b = np.stack([x1, y1, x2, y2], 1).astype(np.float32)
        plain, normed = keys64(b, h, w)
        if separated(plain) and separated(normed) and (not same_order or np.array_equal(np.argsort(plain), np.argsort(normed))):
            return b


def build_inputs():
    rng = np.random.default_rng(20261019)
    att, box = [], []
    for i, K in enumerate(KS):
        h, w = SIZES[i]
        a = np.clip(rng.standard_normal((K, D)), 0, None).astype(np.float32) + np.float32(0.01)
        b = draw_boxes(rng, K - 1 if i == TIE else K, h, w, same_order=i in (DESC, ASC))
        if i == TIE:                                        # rows 1 and 3 are the same box (different features)
            b = np.insert(b, 3, b[1], axis=0)
        if i in (DESC, ASC):
            order = np.argsort(keys64(b, h, w)[0])
            b = b[order[::-1] if i == DESC else order]
        att.append(a)
        box.append(np.ascontiguousarray(b))
    return att, box


def check_inputs(att, box):
    for i, (a, b) in enumerate(zip(att, box)):
        h, w = SIZES[i]
        assert a.shape == (KS[i], D) and b.shape == (KS[i], 4) and h != w
        plain, normed = keys64(b, h, w)
        if i == TIE:
            assert np.array_equal(b[1], b[3]) and not np.array_equal(a[1], a[3])
            plain, normed = np.delete(plain, 3), np.delete(normed, 3)
        assert separated(plain) and separated(normed), i
        if i == DESC:
            assert np.all(np.diff(plain) < 0) and np.all(np.diff(normed) < 0)
        if i == ASC:
            assert np.all(np.diff(plain) > 0) and np.all(np.diff(normed) > 0)
    assert len(set(SIZES)) == len(SIZES)


def install_stubs():
    h5 = types.ModuleType('h5py')
    h5.File = lambda *a, **k: (_ for _ in ()).throw(RuntimeError('no label file is part of this fixture'))
    sys.modules['h5py'] = h5
    ld = types.ModuleType('lmdbdict')
    ld.lmdbdict = lambda *a, **k: (_ for _ in ()).throw(RuntimeError('lmdb stores are not part of this fixture'))
    lm = types.ModuleType('lmdbdict.methods')
    lm.DUMPS_FUNC, lm.LOADS_FUNC = {'ascii': None}, {'identity': None}
    sys.modules['lmdbdict'], sys.modules['lmdbdict.methods'] = ld, lm


def main():
    att, box = build_inputs()
    check_inputs(att, box)
    out = {'height': np.array([s[0] for s in SIZES], dtype=np.int32), 'width': np.array([s[1] for s in SIZES], dtype=np.int32)}
    for i in range(len(KS)):
        out['att%d' % i], out['box%d' % i] = att[i], box[i]
    install_stubs()
    assert os.path.isdir(os.path.join(REF, 'captioning')), 'set CAPMI_REFERENCE to a checkout of the reference'
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    from captioning.data.dataloader import Dataset            # noqa: E402  (the reference)
    with tempfile.TemporaryDirectory() as tmp:
        for d in ('att', 'box', 'fc'):
            os.makedirs(os.path.join(tmp, d))
        images = []
        for i in range(len(KS)):
            images.append({'id': 500 + i, 'split': 'train', 'height': SIZES[i][0], 'width': SIZES[i][1]})
            np.savez(os.path.join(tmp, 'att', '%d.npz' % (500 + i)), feat=att[i])
            np.save(os.path.join(tmp, 'box', '%d.npy' % (500 + i)), box[i])
        json.dump({'images': images, 'ix_to_word': {'1': 'a'}}, open(os.path.join(tmp, 'dataset.json'), 'w'))
        for na in (0, 1):
            for nb in (0, 1):
                opt = argparse.Namespace(seq_per_img=1, use_fc=True, use_att=True, use_box=1, norm_att_feat=na, norm_box_feat=nb,
                                         input_json=os.path.join(tmp, 'dataset.json'), input_label_h5='none',
                                         input_fc_dir=os.path.join(tmp, 'fc'), input_att_dir=os.path.join(tmp, 'att'),
                                         input_box_dir=os.path.join(tmp, 'box'), train_only=0, data_in_memory=False)
                ds = Dataset(opt)
                for i in range(len(KS)):
                    fc, a = ds[(i, 0, False)][:2]
                    assert a.dtype == np.float32 and a.shape == (KS[i], D + 5)
                    out['want.a%d.b%d.%d' % (na, nb, i)] = a
                    out['fc.a%d.b%d.%d' % (na, nb, i)] = np.asarray(fc, dtype=np.float32)
    np.savez_compressed(os.path.join(HERE, 'box_ref.npz'), **out)
    print('written box_ref.npz with', len(out), 'arrays')


if __name__ == '__main__':
    main()
