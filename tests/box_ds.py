"""The tiny use_box dataset of tests/golden/box_ref.npz (make_box_golden.py: 6 images, K = 1, 2, 5, 7, 7, 9, D = 24, the reference's
own rows for the four norm_att_feat / norm_box_feat settings) written out as the files FeatureLoader reads, and the comparisons the
host and the GPU tests share."""
import json
import os

import numpy as np

from conftest import GOLDEN

N_IMG, D = 6, 24
KS = (1, 2, 5, 7, 7, 9)
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]                # (norm_att_feat, norm_box_feat)
REL = 1e-6                                               # test_optim_gpu.TOL: the project's bound for element-wise kernels
_Z = None


def ref():
    global _Z
    if _Z is None:
        z = np.load(os.path.join(GOLDEN, 'box_ref.npz'))
        _Z = {k: z[k] for k in z.files}
    return _Z


def want(na, nb, i):
    return ref()['want.a%d.b%d.%d' % (na, nb, i)]


def write_dataset(tmp, hw=True, drop_box_row_of=None, box_ext='.npy'):
    """-> argv of the loader options.  hw False: the info json carries no height / width; drop_box_row_of: that image's box file
    holds one box too few"""
    z = ref()
    rng = np.random.default_rng(5)
    for d in ('att', 'box'):
        os.makedirs(os.path.join(str(tmp), d), exist_ok=True)
    images, labels, start, end = [], [], [], []
    for i in range(N_IMG):
        img = {'id': 500 + i, 'split': 'train', 'file_path': 'img/%d.jpg' % (500 + i)}
        if hw:
            img['height'], img['width'] = int(z['height'][i]), int(z['width'][i])
        images.append(img)
        np.savez(os.path.join(str(tmp), 'att', '%d.npz' % (500 + i)), feat=z['att%d' % i])
        b = z['box%d' % i]
        if drop_box_row_of == i:
            b = b[:-1]
        if box_ext == '.npy':
            np.save(os.path.join(str(tmp), 'box', '%d.npy' % (500 + i)), b)
        else:
            np.savez(os.path.join(str(tmp), 'box', '%d.npz' % (500 + i)), feat=b)
        start.append(len(labels) + 1)
        for _ in range(3):
            ln = int(rng.integers(2, 6))
            row = np.zeros(5, dtype=np.uint32)
            row[:ln] = rng.integers(1, 13, size=ln)
            labels.append(row)
        end.append(len(labels))
    json.dump({'images': images, 'ix_to_word': {str(i): 'w%d' % i for i in range(1, 13)}}, open(os.path.join(str(tmp), 'd.json'), 'w'))
    np.savez(os.path.join(str(tmp), 'l.npz'), labels=np.stack(labels), label_start_ix=np.array(start, dtype=np.uint32),
             label_end_ix=np.array(end, dtype=np.uint32))
    return ['--input_json', os.path.join(str(tmp), 'd.json'), '--input_label_h5', os.path.join(str(tmp), 'l.npz'),
            '--input_att_dir', os.path.join(str(tmp), 'att'), '--input_box_dir', os.path.join(str(tmp), 'box'),
            '--fc_feat_size', str(D + 5), '--att_feat_size', str(D + 5)]


def flag_args(na, nb):
    return ['--use_box', '1', '--norm_att_feat', str(na), '--norm_box_feat', str(nb)]


def check_rows(got, na, nb, i, what=''):
    """every row of image i against the reference's: the row order exact, unnormalised columns bit-equal, normalised ones within REL"""
    w = want(na, nb, i)
    got = np.asarray(got)
    tag = '%s image %d norm_att %d norm_box %d' % (what, i, na, nb)
    assert got.shape == w.shape and got.dtype == np.float32, tag
    # the order: every reference row is nearest to the row that stands at its own position
    dist = np.abs(got[None, :, :].astype(np.float64) - w[:, None, :]).max(2)              # [want row, got row]
    assert np.array_equal(dist.argmin(1), np.arange(w.shape[0])), (tag, dist.argmin(1))
    for cols, normed in ((slice(0, D), na), (slice(D, D + 5), nb)):
        g, x = got[:, cols], w[:, cols]
        if normed:
            err = np.abs(g.astype(np.float64) - x)
            assert np.all(err <= REL * np.abs(x)), (tag, cols, float((err / np.maximum(np.abs(x), 1e-300)).max()))
        else:
            assert np.array_equal(g.view(np.int32), x.view(np.int32)), (tag, cols)
