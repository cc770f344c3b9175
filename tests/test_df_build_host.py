"""Host side of the device document-frequency build: the checker (tests/df_ref.py) pinned on what the project already trusts, the
host half of tools/prepro_ngrams.py, and the argument checks of the two entry points that need no GPU.

PARITY UNPINNED: the reference's scripts/prepro_ngrams.py cannot be run, because the scorer package it imports (pyciderevalcap,
the `cider` submodule) is empty in the reference checkout.  The checker restates its published behaviour and is held equal to
oracle/ciderd.py::build_document_frequency, the restatement of compute_doc_freq the CIDEr-D tests already rest on.
"""
import ctypes as C
import json

import numpy as np
import pytest

import df_ref

SMALL = [[[5, 0], [3, 4, 0]],                      # lengths 1 + eos ... the shapes of the GPU test
         [[3, 4, 3, 4, 0], [3, 4, 7, 0]],
         [],
         [[7, 7, 7, 7, 7, 0]]]


def test_checker_agrees_with_the_oracle_restatement_of_compute_doc_freq():
    from oracle import ciderd as O
    rng = np.random.default_rng(0)
    for images in (SMALL, df_ref.random_images(rng, 30, 4, 9, 6), [[]] + df_ref.random_images(rng, 5, 2, 70, 3) + [[]]):
        df, ref_len = df_ref.doc_freq(images)
        odf, oref = O.build_document_frequency(images)
        assert dict(odf) == df and oref == ref_len == len(images)
    df, _ = df_ref.doc_freq(SMALL)
    assert df[(3, 4)] == 2.0 and df[(4, 0)] == 2.0 and df[(7,)] == 2.0 and df[(7, 7, 7, 7)] == 1.0 and df[(5, 0)] == 1.0
    assert (4, 3, 4, 0) in df and (0,) in df and df[(0,)] == 3.0


def test_checker_table_round_trips_through_the_image_file(tmp_path):
    from imagecaptioning.pytorch_amd import ciderd as D
    df, ref_len = df_ref.doc_freq(df_ref.random_images(np.random.default_rng(1), 40, 3, 8, 12))
    keys, vals = D.build_table(df)
    want = {(D.pack_ngram(g), c) for g, c in df.items()}
    assert df_ref.pairs(keys, vals) == want
    path = D.save_df_image(df, ref_len, str(tmp_path / 'x.capmi.npz'))
    k2, v2, r2 = D.load_df_image(path)
    assert df_ref.pairs(k2, v2) == want and r2 == ref_len and k2.shape[0] == D.table_cap(len(df))
    # the writer of an already hashed table (what tools/prepro_ngrams.py uses) stores the same file
    path = D.save_table_image(keys, vals, ref_len, str(tmp_path / 'y.capmi.npz'))
    k3, v3, r3 = D.load_df_image(path)
    assert (k3 == keys).all() and (v3 == vals).all() and r3 == ref_len and int(np.load(path)['n']) == len(df)


@pytest.mark.parametrize('n', [0, 1, 8, 9, 1024, 1025, 4096, 4097])
def test_table_cap_is_the_size_build_table_chooses(n):
    from imagecaptioning.pytorch_amd import ciderd as D
    keys, _ = D.build_table({(i % 60000, i // 60000): 1.0 for i in range(n)})
    assert keys.shape[0] == D.table_cap(n) and 2 * n <= D.table_cap(n) and (n <= 8 or D.table_cap(n) < 4 * n)


def _dataset():
    sent = lambda *w: {'tokens': list(w)}                                                    # noqa: E731
    images = [{'cocoid': 1, 'split': 'train', 'sentences': [sent('a', 'cat'), sent('a', 'zebra', 'sat')]},
              {'cocoid': 2, 'split': 'restval', 'sentences': [sent('a', 'cat', 'sat')]},
              {'cocoid': 3, 'split': 'val', 'sentences': [sent('cat')]},
              {'cocoid': 4, 'split': 'test', 'sentences': []},
              {'cocoid': 5, 'split': 'train', 'sentences': []}]
    vocab = {'1': 'a', '2': 'cat', '3': 'sat', '4': 'UNK'}
    return {'images': images}, {'ix_to_word': vocab}


def _images_of(tok, cap_off, img_off):
    return [[tok[cap_off[c]:cap_off[c + 1]].tolist() for c in range(img_off[i], img_off[i + 1])] for i in range(len(img_off) - 1)]


def test_host_half_of_the_tool_reads_captions_as_the_reference_does():
    from imagecaptioning.pytorch_amd.tools import prepro_ngrams as P
    data, d = _dataset()
    train = _images_of(*P.corpus_from_json(data['images'], d['ix_to_word'], 'train'))
    assert train == [[[1, 2, 0], [1, 4, 3, 0]], [[1, 2, 3, 0]], []]          # restval joins, zebra -> UNK, <eos> = 0, image 5 stays
    assert _images_of(*P.corpus_from_json(data['images'], d['ix_to_word'], 'val')) == [[[2, 0]]]
    assert _images_of(*P.corpus_from_json(data['images'], d['ix_to_word'], 'test')) == [[]]
    assert len(_images_of(*P.corpus_from_json(data['images'], d['ix_to_word'], 'all'))) == 5
    tok, cap_off, img_off = P.corpus_from_json(data['images'], d['ix_to_word'], 'train')
    assert cap_off.dtype == np.int64 and img_off.dtype == np.int64 and cap_off[-1] == len(tok) and img_off[-1] == len(cap_off) - 1
    no_unk = {k: v for k, v in d['ix_to_word'].items() if v != 'UNK'}
    with pytest.raises(SystemExit, match='UNK'):
        P.corpus_from_json(data['images'], no_unk, 'train')


def test_label_rows_become_captions_with_an_eos_where_the_row_has_room():
    from imagecaptioning.pytorch_amd.tools import prepro_ngrams as P
    from imagecaptioning.pytorch_amd import synthetic
    labels = np.array([[1, 2, 0, 0], [1, 2, 3, 4], [5, 0, 0, 0], [2, 2, 2, 0]], dtype=np.uint32)
    lab = {'labels': labels, 'label_start_ix': np.array([1, 3, 4], dtype=np.uint32), 'label_end_ix': np.array([2, 3, 4], dtype=np.uint32)}
    info = {'images': [{'id': 0, 'split': 'train'}, {'id': 1, 'split': 'val'}, {'id': 2, 'split': 'restval'}]}
    images = _images_of(*P.corpus_from_labels(info, lab, 'train'))
    assert images == [[[1, 2, 0], [1, 2, 3, 4]], [[2, 2, 2, 0]]]               # the full row is a cut caption: no <eos>
    # the table tools/train.py builds on the host when no file is named
    want = synthetic.document_frequency([labels[0:2], labels[3:4]])
    assert df_ref.doc_freq(images) == want


def test_bpe_vocabulary_is_refused_by_name(tmp_path):
    from imagecaptioning.pytorch_amd.tools import prepro_ngrams as P
    data, d = _dataset()
    d['bpe'] = '#version: 0.2\na t</w>\n'
    (tmp_path / 'd.json').write_text(json.dumps(data))
    (tmp_path / 'v.json').write_text(json.dumps(d))
    with pytest.raises(SystemExit, match='bpe'):
        P.main(['--input_json', str(tmp_path / 'd.json'), '--dict_json', str(tmp_path / 'v.json'), '--output_pkl', str(tmp_path / 'x')])
    assert not list(tmp_path.glob('x*'))


def test_help_says_what_is_not_produced(capsys):
    from imagecaptioning.pytorch_amd.tools import prepro_ngrams as P
    with pytest.raises(SystemExit):
        P.main(['--help'])
    out = capsys.readouterr().out
    assert '-words' in out and 'bpe' in out and '--from_labels' in out and 'label file cuts' in out


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """CAPMI_EINVAL is decided on the host: the pointers below are host buffers that are never dereferenced on the device."""
    from imagecaptioning.pytorch_amd import _lib
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    good_cap, good_img = np.array([0, 2, 5], dtype=np.int64), np.array([0, 1, 2], dtype=np.int64)

    def count(tok=p, elem=8, total=5, cap_off=p, cap_host=good_cap, n_caps=2, img_off=p, img_host=good_img, n_img=2, keys=p,
              counts=p, cap=16, nd=p, err=p):
        return _lib.lib.capmi_df_count(tok, elem, total, cap_off, cap_host.ctypes.data if cap_host is not None else None, n_caps,
                                       img_off, img_host.ctypes.data if img_host is not None else None, n_img, keys, counts, cap,
                                       nd, err, None)

    assert count(n_img=0, img_host=np.array([0], dtype=np.int64), n_caps=0, cap_host=np.array([0], dtype=np.int64), total=0) == 0
    for bad in (dict(tok=None), dict(cap_off=None), dict(img_off=None), dict(keys=None), dict(counts=None), dict(nd=None),
                dict(err=None), dict(elem=2), dict(total=-1), dict(cap=0), dict(cap=24),
                dict(cap_host=np.array([0, 3, 2], dtype=np.int64)),             # decreasing
                dict(cap_host=np.array([0, 2, 4], dtype=np.int64)),             # does not end at total_tokens
                dict(cap_host=np.array([1, 2, 5], dtype=np.int64)),             # does not start at 0
                dict(img_host=np.array([0, 2, 1], dtype=np.int64)),
                dict(img_host=np.array([0, 1, 3], dtype=np.int64))):
        assert count(**bad) == _lib.EINVAL, bad
    fin = _lib.lib.capmi_df_finalize
    assert fin(None, p, 16, p, p, 16, p, None) == _lib.EINVAL and fin(p, p, 16, p, None, 16, p, None) == _lib.EINVAL
    assert fin(p, p, 12, p, p, 16, p, None) == _lib.EINVAL and fin(p, p, 16, p, p, 0, p, None) == _lib.EINVAL
    assert fin(p, p, 16, p, p, 16, None, None) == _lib.EINVAL
