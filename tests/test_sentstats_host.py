"""The host side of the sentence statistics (imagecaptioning/pytorch_amd/sentstats.py): ids <=> strings -- the two restatements of
tests/sentstats_ref.py agree, so counting over ids (what the device does) is counting over the reference's strings --, the
loaders' training_captions(), and the switch's default.  No GPU."""
import json
import os
import sys

import numpy as np

from conftest import ROOT

import sentstats_ref as S
from test_feature_loader import make_dataset, _opts

PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')

# a vocabulary with bad endings and an UNK: id 7 is 'UNK', ids 1, 2, 3 are bad endings
WORDS = {'1': 'a', '2': 'the', '3': 'with', '4': 'dog', '5': 'cat', '6': 'sits', '7': 'UNK', '8': 'grass', '9': 'on'}
UNK, BAD = 7, [1, 2, 3, 9]


def _pad(rows, w):
    out = np.zeros((len(rows), w), dtype=np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _both(words, train, rows_n, first):
    unk = next((int(k) for k, v in words.items() if v == 'UNK'), 0)
    bad = [int(k) for k, v in words.items() if v in S.BAD_ENDINGS]
    a, b = S.on_strings(words, train, rows_n, first), S.on_ids(train, rows_n, first, unk, bad)
    assert a == b, (a, b)
    return a


def test_hand_made_cases_agree_and_mean_what_they_should():
    assert sorted(BAD) == sorted(int(k) for k, v in WORDS.items() if v in S.BAD_ENDINGS)
    train = _pad([[4, 6], [4, 6], [5, 6, 9, 8], [4, 7], [], [5]], 5)
    train[0, 3] = 8                                            # behind the first 0: ignored
    rows_n = _pad([[4, 6],                                     # seen
                   [4, 6, 9],                                  # the seen one is its strict prefix: novel
                   [4],                                        # a strict prefix of a seen one: novel
                   [4, 7],                                     # equals a training row token for token, but holds UNK: novel
                   [],                                         # the empty caption is a training sentence here: seen
                   [5, 6, 9, 8], [5, 6, 9, 8],                 # twice: distinct once, seen
                   [8, 8, 8, 8, 8]], 5)                        # full width, no terminator: novel
    rows_n[2, 2] = 6                                           # behind the first 0: still the sentence (4,)
    first = _pad([[4, 6, 9], [4, 6], [], [1, 1, 1, 1, 2], [7]], 5)
    got = _both(WORDS, train, rows_n, first)
    assert got == {'rows': 8, 'distinct': 7, 'novel': 4, 'vocab_size': 6, 'first': 5, 'bad': 2, 'novel_sentences': 0.5,
                   'bad_count_rate': 0.4}
    # without an empty training row the empty caption is novel; without any sample_n row the two keys are absent (eval_utils.py:54)
    assert _both(WORDS, train[:4], rows_n, first)['novel'] == 5
    none = _both(WORDS, train, rows_n[:0], first)
    assert 'novel_sentences' not in none and 'vocab_size' not in none and none['bad_count_rate'] == 0.4


def test_a_vocabulary_without_unk_skips_nothing():
    words = {k: ('zebra' if v == 'UNK' else v) for k, v in WORDS.items()}
    train = _pad([[4, 7], [4, 6]], 4)
    got = _both(words, train, _pad([[4, 7], [4, 6], [5]], 4), _pad([[4]], 4))
    assert got['novel'] == 1 and got['distinct'] == 3


def test_random_cases_agree():
    rng = np.random.default_rng(20240913)
    for case in range(40):
        w, vocab = int(rng.integers(1, 9)), int(rng.integers(3, 12))
        words = {str(i): 'w%d' % i for i in range(1, vocab + 1)}
        if case % 2:
            words[str(int(rng.integers(1, vocab + 1)))] = 'UNK'
        for i in rng.choice(vocab, size=2, replace=False) + 1:                 # two bad endings (never the UNK)
            if words[str(i)] != 'UNK':
                words[str(i)] = S.BAD_ENDINGS[int(i) % len(S.BAD_ENDINGS)]
        assert len(set(words.values())) == len(words)

        def rows(n):
            r = rng.integers(0, vocab + 1, size=(n, w))                        # zeros anywhere: short, empty and full rows
            return r.astype(np.int64)
        got = _both(words, rows(30), rows(int(rng.integers(0, 25))), rows(int(rng.integers(1, 10))))
        assert got['novel'] <= got['distinct'] <= got['rows']


def test_training_captions_of_the_feature_loader(tmp_path):
    sys.path.insert(0, PKG)
    from captioning.data.feature_loader import FeatureLoader
    from captioning.data.resident import ResidentFeatures
    from captioning.data.prefetch import DevicePrefetcher
    args = make_dataset(tmp_path)                              # 9 images: 0-5 train, 6-7 val, 8 restval
    info = json.load(open(tmp_path / 'data.json'))
    info['images'][5]['split'] = 'test'
    (tmp_path / 'data.json').write_text(json.dumps(info))
    lab = np.load(tmp_path / 'labels.npz')

    def rows_of(images):
        return np.concatenate([lab['labels'][lab['label_start_ix'][i] - 1: lab['label_end_ix'][i]] for i in images])
    want = rows_of([0, 1, 2, 3, 4, 8])                         # restval is training; val and test are not
    for train_only in ('0', '1'):                              # train_only drops restval from the train SPLIT, not from this set
        ld = FeatureLoader(_opts(args + ['--batch_size', '4', '--train_only', train_only]))
        assert (8 in ld.split_ix['train']) == (train_only == '0')
        got = ld.training_captions()
        assert got.dtype == np.uint32 and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(ResidentFeatures(ld, 'cpu').training_captions(), want)
        pre = DevicePrefetcher.__new__(DevicePrefetcher)       # its constructor opens a device stream; the forwarding is what counts
        pre.loader = ld
        np.testing.assert_array_equal(pre.training_captions(), want)


def test_training_captions_of_the_synthetic_loader():
    sys.path.insert(0, PKG)
    from captioning.data.synthetic_loader import SyntheticLoader
    ld = SyntheticLoader(_opts(['--vocab_size', '40', '--seq_length', '6', '--synthetic_images', '12']))
    got = ld.training_captions()
    assert got.shape == (60, 6)
    np.testing.assert_array_equal(got, np.concatenate(ld.refs))
    np.testing.assert_array_equal(got.astype(np.int64), ld.language_eval_refs('val')[0])
    assert ld.get_vocab()['40'] == 'UNK'


def test_the_switch_is_off_by_default_and_reaches_no_sampler():
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import eval as E
    from imagecaptioning.pytorch_amd.tools import eval_ensemble
    assert opts.DEFAULTS['sentence_stats'] == 0
    off, on = _opts([]), _opts(['--sentence_stats', '1'])
    assert off.sentence_stats == 0 and on.sentence_stats == 1
    rest = {k: v for k, v in vars(on).items() if k != 'sentence_stats'}
    assert rest == {k: v for k, v in vars(off).items() if k != 'sentence_stats'}
    assert E.eval_kwargs_of(off) == E.eval_kwargs_of(on) and 'sentence_stats' not in E.eval_kwargs_of(on)
    assert set(E.eval_kwargs_of(off)) == set(E.SAMPLE_KEYS)
    assert 'sentence_stats' in eval_ensemble.EVAL_KEYS
