"""Device document-frequency build (capmi_df_count / capmi_df_finalize, tools/prepro_ngrams.py) against the dict checker
tests/df_ref.py.  Everything is an integer or an exact conversion: every comparison is equality, there is no tolerance.

PARITY UNPINNED: the reference's scripts/prepro_ngrams.py cannot be run (its scorer package is absent from the reference
checkout); tests/test_df_build_host.py holds the checker equal to the project's restatement of compute_doc_freq.
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import df_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')

# caption lengths 1, 2, 4, 3 and 5 before the <eos>: n-grams that contain the trailing 0; (3, 4) twice inside one caption, again in
# the image's other caption (counts once) and in another image (counts twice); an image without captions
SMALL = [[[5, 0], [3, 4, 0]],
         [[3, 4, 3, 4, 0], [3, 4, 7, 0]],
         [],
         [[7, 7, 7, 7, 7, 0]]]


def _want(images):
    """what build_table makes of the checker's dict: the (key, val) set, cap, ref_len"""
    from imagecaptioning.pytorch_amd import ciderd as D
    df, ref_len = df_ref.doc_freq(images)
    return df_ref.pairs(*D.build_table(df)), D.table_cap(len(df)), float(ref_len)


def _check(images, tok_dtype=np.int64, on_device=False, count_cap=None, want=None):
    """build on the device and compare with _want: the (key, val) set, cap, ref_len"""
    from imagecaptioning.pytorch_amd import ciderd as D
    corpus = df_ref.ragged(images, tok_dtype)
    if on_device:
        corpus = tuple(torch.from_numpy(a).to(DEV) for a in corpus)
    keys, vals, ref_len = D.build_df_image(*corpus, device=DEV, count_cap=count_cap)
    assert keys.dtype == np.uint64 and vals.dtype == np.float64
    assert (df_ref.pairs(keys, vals), keys.shape[0], ref_len) == (want or _want(images))


def _surviving(tok, cap_off, img_off):
    """the images whose own offsets are well formed (capmi.h CAPMI_DF_E_OFFSETS: the others are skipped)"""
    out, n_caps, n_img = [], len(cap_off) - 1, len(img_off) - 1
    for i in range(n_img):
        c0, c1 = int(img_off[i]), int(img_off[i + 1])
        ok = 0 <= c0 <= c1 <= n_caps and (i > 0 or c0 == 0) and (i < n_img - 1 or c1 == n_caps)
        if ok and all(0 <= cap_off[c] <= cap_off[c + 1] <= len(tok) for c in range(c0, c1)):
            out.append([tok[cap_off[c]:cap_off[c + 1]].tolist() for c in range(c0, c1)])
    return out


@pytest.mark.parametrize('tok_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('on_device', [False, True])
def test_small_corpus_with_empty_images_anywhere(tok_dtype, on_device):
    _check(SMALL, tok_dtype, on_device)
    _check([[]] + SMALL, tok_dtype, on_device)               # the first image is empty
    _check(SMALL + [[]], tok_dtype, on_device)               # the last one
    _check([[], [[9, 0]], []], tok_dtype, on_device)
    _check([[[4]]], tok_dtype, on_device)                    # a caption is its tokens: nothing is appended


def test_captions_beyond_the_row_width_and_an_image_beyond_one_tile():
    rng = np.random.default_rng(5)
    long_cap = rng.integers(1, 6, size=70).tolist() + [0]                    # 71 tokens > CAPMI_LANGEVAL_LMAX
    big = [rng.integers(1, 30, size=60).tolist() for _ in range(40)]         # 2400 tokens: ten tiles of positions
    _check([[long_cap], big, [[1, 2, 0]], [long_cap[:65]]])


@pytest.mark.parametrize('vocab', [50, 60000])
def test_many_images_contended_keys_and_long_probe_chains_are_reproducible(vocab):
    """vocab 50: 10 000 captions hammer a few thousand slots; vocab 60 000: some 700 000 keys.  Two runs: the same pairs.  The
    scorer built from the corpus scores a fixed batch bit for bit like the one built from the checker's dict."""
    from imagecaptioning.pytorch_amd import ciderd as D
    rng = np.random.default_rng(vocab)
    images = df_ref.random_images(rng, 2000, 5, 19, vocab, min_len=3)
    want = _want(images)
    _check(images, np.int32, want=want)
    _check(images, np.int32, on_device=True, want=want)      # the second run: the same set
    df, ref_len = df_ref.doc_freq(images)
    a = D.DeviceCiderD(df, ref_len, DEV)
    b = D.DeviceCiderD.from_corpus(*df_ref.ragged(images), device=DEV)
    assert b.cap == a.cap and b.log_ref_len == a.log_ref_len and b.keys.dtype == a.keys.dtype and b.vals.dtype == a.vals.dtype
    B, n, L = 6, 3, 20
    gts = [np.array([c[:L] + [0] * (L - len(c[:L])) for c in images[i]], dtype=np.int64) for i in range(B)]
    hyp = np.zeros((B * n, L), dtype=np.int64)
    for i in range(B * n):
        row = gts[i // n][i % 5].copy()
        flip = rng.random(L) < 0.25
        row[flip] = rng.integers(0, vocab + 1, size=int(flip.sum()))
        hyp[i] = row
    hyp_d = torch.from_numpy(hyp).to(DEV)
    img = (torch.arange(B * n, device=DEV) // n).to(torch.int32)
    scores = []
    for s in (a, b):
        packed = s.pack_refs(gts)
        scores.append(s.score(hyp_d, img, packed[0], packed[1], packed.cooked).cpu().numpy())
        scores.append(s.score(hyp_d, img, packed[0], packed[1]).cpu().numpy())
        scores.append(s.bleu4(hyp_d, img, packed, 0.0, 1.0).cpu().numpy())
        scores.append(s.self_cider(hyp_d, n).cpu().numpy())
    for x, y in zip(scores[:4], scores[4:]):
        assert x.tobytes() == y.tobytes()
    assert scores[0].max() > 0


@pytest.mark.parametrize('n', [8, 9, 1024, 1025])
def test_finalize_at_the_load_factor_boundaries(n):
    """n single-token captions: exactly n distinct n-grams.  At a power of two the image is exactly half full, one more doubles it."""
    from imagecaptioning.pytorch_amd import ciderd as D
    images = [[[t] for t in range(n)], [[t] for t in range(0, n, 3)]]
    _check(images)
    assert len(df_ref.doc_freq(images)[0]) == n
    keys, _, _ = D.build_df_image(*df_ref.ragged(images), device=DEV)
    assert keys.shape[0] == D.table_cap(n) == (2 * n if n & (n - 1) == 0 else 4 * (n - 1))


def test_token_range_table_full_and_malformed_offsets():
    from imagecaptioning.pytorch_amd import _lib, ops
    from imagecaptioning.pytorch_amd import ciderd as D
    _check([[[65534, 1, 65534, 0]], [[65534]]])                               # the largest id a key field holds
    for bad in (65535, -1, 1 << 40):
        with pytest.raises(_lib.CapmiError, match='token id'):
            D.build_df_image(*df_ref.ragged([[[1, 2, 0]], [[3, bad, 0]]]), device=DEV)
    images = df_ref.random_images(np.random.default_rng(2), 20, 3, 10, 40)
    n = len(df_ref.doc_freq(images)[0])
    assert n > 64
    with pytest.raises(_lib.CapmiError, match='table full'):
        D.build_df_image(*df_ref.ragged(images), device=DEV, count_cap=64)
    _check(images, count_cap=D.table_cap(n) // 2)                             # a counting table that is nearly full still serves

    tok, cap_off, img_off = df_ref.ragged(SMALL)
    bad_cap, bad_img = cap_off.copy(), img_off.copy()
    bad_cap[3] = 4                                                            # image 1's first caption runs backwards
    bad_img[2] = 1
    # offsets on the host are checked before anything is launched: CAPMI_EINVAL
    for c, i in ((bad_cap, img_off), (cap_off, bad_img)):
        with pytest.raises(_lib.CapmiError, match='capmi_df_count failed: invalid argument'):
            D.build_df_image(tok, c, i, device=DEV)
    # offsets that exist on the device only set the error bit; the image is skipped, the others are counted, nothing else is touched
    dev = lambda a: torch.from_numpy(a).to(DEV)                                              # noqa: E731
    for c, i in ((bad_cap, img_off), (cap_off, bad_img), (np.array([0, 2, 5, 10, 14, 1 << 40]), img_off),      # beyond the corpus
                 (cap_off, np.array([0, 2, 4, 4, 1 << 33])), (cap_off, np.array([-3, 2, 4, 4, 5])), (cap_off, np.array([0, 2, 4, 4, 4]))):
        with pytest.raises(_lib.CapmiError, match='offsets'):
            D.build_df_image(dev(tok), dev(np.asarray(c, dtype=np.int64)), dev(np.asarray(i, dtype=np.int64)), device=DEV)
        ckeys = torch.zeros(256, dtype=torch.int64, device=DEV)
        guard = torch.zeros(3, 256, dtype=torch.int32, device=DEV)            # the counts sit between two rows that must stay 0
        meta = torch.zeros(2, dtype=torch.int32, device=DEV)
        ops.df_count(dev(tok), dev(np.asarray(c, dtype=np.int64)), dev(np.asarray(i, dtype=np.int64)), ckeys, guard[1], meta)
        assert meta[0].item() == _lib.DF_E_OFFSETS
        left = _surviving(tok, c, i)
        assert len(left) < len(SMALL)
        want, _ = df_ref.doc_freq(left)
        got = df_ref.pairs(ckeys.cpu().numpy().view(np.uint64), guard[1].cpu().numpy())
        assert got == {(D.pack_ngram(g), int(v)) for g, v in want.items()} and meta[1].item() == len(want)
        assert not guard[0].any() and not guard[2].any()


def _write_dataset(tmp_path, n_img=12, width=8):
    """a dataset json with tokenised captions, the dict json and the training files (label rows, features) of the same captions"""
    rng = np.random.default_rng(0)
    (tmp_path / 'att').mkdir()
    (tmp_path / 'data').mkdir()
    itow = {str(i): 'w%d' % i for i in range(1, 29)}
    itow['29'] = 'UNK'
    labels, start, end, images, talk = [], [], [], [], []
    for i in range(n_img):
        np.savez_compressed(tmp_path / 'att' / ('%d.npz' % i), feat=np.clip(rng.standard_normal((6, 24)), 0, None).astype(np.float32))
        split = ('train', 'train', 'restval', 'val', 'test', 'train')[i % 6]
        start.append(len(labels) + 1)
        sents = []
        for _ in range(5):
            ids = rng.integers(1, 29, size=int(rng.integers(3, width + 3))).tolist()      # some captions are longer than the label width
            words = ['w%d' % t for t in ids]
            if rng.random() < 0.3:
                words[1], ids[1] = 'zebra%d' % i, 29                                        # not in the vocabulary
            sents.append({'tokens': words, 'ids': ids})
            row = np.zeros(width, dtype=np.uint32)
            row[:min(width, len(ids))] = ids[:width]
            labels.append(row)
        end.append(len(labels))
        images.append({'cocoid': i, 'split': split, 'sentences': [{'tokens': s['tokens']} for s in sents]})
        talk.append({'id': i, 'split': split})
        images[-1]['_ids'] = [s['ids'] for s in sents]
    (tmp_path / 'dataset.json').write_text(json.dumps({'images': [{k: v for k, v in im.items() if k != '_ids'} for im in images]}))
    (tmp_path / 'talk.json').write_text(json.dumps({'images': talk, 'ix_to_word': itow}))
    np.savez(tmp_path / 'label.npz', labels=np.stack(labels), label_start_ix=np.array(start, dtype=np.uint32),
             label_end_ix=np.array(end, dtype=np.uint32))
    return images, np.stack(labels), start, end


def test_tool_writes_the_image_the_scorer_and_the_trainer_load(tmp_path, monkeypatch):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd import ciderd as D
    from imagecaptioning.pytorch_amd.tools import prepro_ngrams as P, train as T
    from captioning.utils import opts, rewards
    images, labels, start, end = _write_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    base = ['--input_json', 'dataset.json', '--dict_json', 'talk.json']
    for split, stem in (('train', 'data/x'), ('all', 'data/all'), ('val', 'data/v')):
        out = P.main(base + ['--output_pkl', stem, '--split', split])
        assert out == stem + '-idxs.capmi.npz' and not os.path.exists(stem + '-words.p')
        mine = [[c + [0] for c in im['_ids']] for im in images
                if split == 'all' or im['split'] == split or (split == 'train' and im['split'] == 'restval')]
        keys, vals, ref_len = D.load_df_image(out)
        pairs, cap, want_len = _want(mine)
        assert df_ref.pairs(keys, vals) == pairs and keys.shape[0] == cap and ref_len == want_len
    assert len([im for im in images if im['split'] == 'restval']) == 2 and _want(mine)[2] == 2.0

    # the label-file mode: the checker on the label rows of the training images
    out = P.main(['--from_labels', '--input_json', 'talk.json', '--input_label_h5', 'label.npz', '--output_pkl', 'data/lab'])
    rows = [[P.caption_of_label_row(r) for r in labels[start[i] - 1:end[i]]] for i, im in enumerate(images) if im['split'] in ('train', 'restval')]
    assert any(0 not in c for im in rows for c in im) and any(0 in c for im in rows for c in im)
    keys, vals, ref_len = D.load_df_image(out)
    pairs, cap, want_len = _want(rows)
    assert df_ref.pairs(keys, vals) == pairs and keys.shape[0] == cap and ref_len == want_len == 8.0

    # rewards.init_scorer finds the file by the reference's name, and one self-critical iteration trains on it
    rewards.reset_scorer()
    scorer = rewards.init_scorer('x-idxs', device=torch.device(DEV))
    assert scorer.cap == np.load('data/x-idxs.capmi.npz')['keys'].shape[0] and scorer.log_ref_len == math.log(8.0)
    rewards.reset_scorer()
    loaded = []
    orig = D.DeviceCiderD.from_image
    monkeypatch.setattr(D.DeviceCiderD, 'from_image', classmethod(lambda cls, path, device: loaded.append(path) or orig(path, device)))
    loss = T.train(opts.parse_opt(
        ['--caption_model', 'updown', '--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--att_feat_size', '24',
         '--fc_feat_size', '24', '--input_json', 'talk.json', '--input_label_h5', 'label.npz', '--input_att_dir', 'att',
         '--batch_size', '4', '--seq_per_img', '3', '--losses_log_every', '1000', '--cached_tokens', 'x-idxs',
         '--self_critical_after', '0', '--train_sample_n', '3', '--max_iters', '1', '--checkpoint_path', str(tmp_path / 'ck')]))
    torch.cuda.synchronize()
    assert loss == loss and loaded == [os.path.join('data', 'x-idxs.capmi.npz')]
    rewards.reset_scorer()
