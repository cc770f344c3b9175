"""Device language_eval (csrc/langeval.hip, langeval.py) against the float64 restatement tests/langeval_ref64.py: corpus CIDEr,
BLEU-1..4 and ROUGE-L over token ids.  Integer statistics (BLEU counts, lengths, LCS lengths, document frequencies) must match
exactly; the float scores within REL_TOL.  Then tools/eval.py and tools/train.py end to end with language_eval 1."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import langeval_ref64 as R

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
DEV = 'cuda:0'

# Largest relative deviation of a float score (corpus and per image) from langeval_ref64.py over the cases of this file, measured
# on an MI355X: MEASURED_REL.  The kernels sum in double and in a fixed order, so the deviation comes from the order of the
# n-gram sums (a dict's order in the restatement) and the device's log / sqrt / pow / exp; the bound is 4 x the measured value.
MEASURED_REL = 2.531e-15       # general / minimum capacity / two chunks / replacement: 2.531e-15; degenerate: 0
REL_TOL = 4 * MEASURED_REL


def _row(rng, length, L, vocab):
    row = np.zeros(L, dtype=np.int64)
    row[:length] = rng.integers(1, vocab, size=length)
    return row


def _general():
    """7 images, 1..5 references each, vocabulary 12, L = 8: n-grams repeat within and across captions"""
    rng = np.random.default_rng(20240611)
    L, vocab = 8, 12
    n_refs = [1, 2, 3, 4, 5, 3, 5]
    refs = [[_row(rng, int(rng.integers(2, L + 1)), L, vocab) for _ in range(n)] for n in n_refs]
    hyps = [_row(rng, int(rng.integers(1, L + 1)), L, vocab) for _ in n_refs]
    # a hypothesis that copies most of a reference, so that higher-order matches and clipping occur
    hyps[4] = refs[4][2].copy()
    hyps[4][1] = hyps[4][0]
    return refs, hyps


def _degenerate():
    L = 8
    refs = [[np.array([1, 2, 3, 4, 5, 6, 7, 8]), np.array([1, 2, 0, 0, 0, 0, 0, 0])],      # a full-length row without a 0
            [np.array([3, 3, 3, 0, 0, 0, 0, 0])],
            [np.array([4, 5, 0, 0, 0, 0, 0, 0]), np.array([5, 0, 0, 0, 0, 0, 0, 0])],
            [np.array([1, 2, 3, 0, 0, 0, 0, 0]), np.array([2, 3, 4, 5, 0, 0, 0, 0])],
            [np.array([6, 7, 6, 7, 0, 0, 0, 0])]]
    hyps = [np.array([1, 2, 3, 4, 5, 6, 7, 8]),       # full length, no terminating 0
            np.zeros(L, dtype=np.int64),              # empty
            np.array([5, 0, 0, 0, 0, 0, 0, 0]),       # length 1: no 2-grams
            np.array([1, 2, 3, 4, 5, 1, 2, 3]),       # longer than every reference
            np.array([0, 6, 7, 6, 7, 0, 0, 0])]       # empty: everything after the first 0 is padding
    return [[r.astype(np.int64) for r in image] for image in refs], [h.astype(np.int64) for h in hyps]


def _device_eval(refs, hyps, chunks=None, table_cap=None):
    """chunks: list of lists of image positions, one `add` each (default: one call, split order)"""
    from imagecaptioning.pytorch_amd.langeval import LanguageEval
    le = LanguageEval.from_gts([np.stack(image) for image in refs], DEV, table_cap=table_cap)
    for chunk in (chunks if chunks is not None else [list(range(len(refs)))]):
        rows = torch.from_numpy(np.stack([hyps[i] if isinstance(i, int) else i[1] for i in chunk])).to(DEV)
        le.add([i if isinstance(i, int) else i[0] for i in chunk], rows)
    stats, per_image = le.compute()
    return le, stats, per_image


def _table(le):
    keys = le.table_keys.cpu().numpy().view(np.uint64)
    counts = le.table_counts.cpu().numpy()
    return {int(k): int(c) for k, c in zip(keys, counts) if k != 0}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.where(b == 0, np.where(a == 0, 0.0, np.inf), np.abs(a - b) / np.abs(b))
    return float(np.max(d)) if d.size else 0.0


def _check(le, stats, per_image, refs, hyps, label):
    """integers exact, floats within REL_TOL; returns the largest relative deviation (printed: run with -s to measure)"""
    from imagecaptioning.pytorch_amd.ciderd import pack_ngram
    want = R.evaluate(refs, hyps)
    assert _table(le) == {pack_ngram(g): c for g, c in want['df'].items()}
    np.testing.assert_array_equal(le._totals.cpu().numpy(), want['totals'])
    bs, lens, lcs, off = le.bleu_stats.cpu().numpy(), le.lens.cpu().numpy(), le.lcs.cpu().numpy(), le.ref_off.cpu().numpy()
    seen = le.seen.cpu().numpy()
    for i, hyp in enumerate(hyps):
        assert bool(seen[i]) == (hyp is not None)
        if hyp is None:
            continue
        g, c, tl, rl = want['stats'][i]
        assert bs[i, :, 0].tolist() == g and bs[i, :, 1].tolist() == c and lens[i].tolist() == [tl, rl], (label, i)
        assert lcs[off[i]:off[i + 1]].tolist() == want['lcs'][i], (label, i)
    assert le.n_added == sum(h is not None for h in hyps)
    has = np.array([h is not None for h in hyps])
    dev = max(_rel([stats[k] for k in R_KEYS], [want[k] for k in R_KEYS]),
              _rel(per_image[has], want['cider_img'][has]), _rel(le.rouge.cpu().numpy()[has], want['rouge_img'][has]))
    print('langeval %s: max relative deviation %.3e' % (label, dev))
    assert np.isnan(per_image[~has]).all()
    assert dev <= REL_TOL, (label, dev)
    return dev


R_KEYS = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDEr')


def test_general_case_matches_the_restatement():
    refs, hyps = _general()
    le, stats, per_image = _device_eval(refs, hyps)
    assert set(stats) == set(R_KEYS) and all(isinstance(v, float) for v in stats.values())
    _check(le, stats, per_image, refs, hyps, 'general')
    assert stats['CIDEr'] > 0 and stats['Bleu_4'] > 1e-4          # the case exercises the higher orders


def test_degenerate_captions():
    refs, hyps = _degenerate()
    le, stats, per_image = _device_eval(refs, hyps)
    _check(le, stats, per_image, refs, hyps, 'degenerate')
    assert per_image[1] == 0.0 and per_image[4] == 0.0 and float(le.rouge[1]) == 0.0       # empty hypotheses score 0


def test_table_at_minimum_capacity_wraps_round():
    from imagecaptioning.pytorch_amd.langeval import min_table_cap
    from imagecaptioning.pytorch_amd._lib import CapmiError
    refs, hyps = _general()
    n_keys = len(R.document_frequency(refs))
    cap = min_table_cap(n_keys)
    assert cap // 2 < n_keys <= cap
    le, stats, per_image = _device_eval(refs, hyps, table_cap=cap)
    assert le.table_cap == cap
    _check(le, stats, per_image, refs, hyps, 'minimum capacity')
    with pytest.raises(CapmiError):                               # one size down the n-grams do not fit: reported, not dropped
        _device_eval(refs, hyps, table_cap=cap // 2)


def test_chunks_in_another_order_give_the_same_result():
    refs, hyps = _general()
    le, stats, per_image = _device_eval(refs, hyps)
    le2, stats2, per_image2 = _device_eval(refs, hyps, chunks=[[5, 2, 6, 0], [3, 1, 4]])
    _check(le2, stats2, per_image2, refs, hyps, 'two chunks')
    assert stats2 == stats                                        # to the last bit: integer sums, fixed-order float sums
    np.testing.assert_array_equal(per_image2, per_image)


def test_a_later_hypothesis_replaces_the_earlier_one():
    refs, hyps = _general()
    other = hyps[5].copy()
    # image 2 first gets another image's caption, then (in the same call: the later row counts) its own; image 0 is replaced by a
    # later call; image 6 never gets a hypothesis
    le, stats, per_image = _device_eval(refs, hyps, chunks=[[(2, other), 0, 1, 2, 3], [4, 5, (0, other)]])
    final = list(hyps)
    final[0], final[6] = other, None
    _check(le, stats, per_image, refs, final, 'replacement')


def test_rows_beyond_the_compiled_bound_are_refused():
    from imagecaptioning.pytorch_amd.langeval import LanguageEval
    refs, hyps = _general()
    le = LanguageEval.from_gts([np.stack(image) for image in refs], DEV)
    with pytest.raises(ValueError):
        le.add([0], torch.zeros(1, 65, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError):
        LanguageEval(np.zeros((2, 65), dtype=np.int64), [0, 1, 2], DEV)


SMALL = ['--caption_model', 'updown', '--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--fc_feat_size', '24',
         '--att_feat_size', '24', '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6', '--max_length', '6',
         '--batch_size', '4', '--seq_per_img', '2', '--synthetic_images', '12']


def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


def test_eval_entrypoint_reports_lang_stats(tmp_path):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    loss, preds, lang_stats = E.main(_opts(SMALL + ['--num_images', '10', '--language_eval', '1', '--split', 'val',
                                                    '--eval_results_dir', str(tmp_path)]))
    assert set(lang_stats) == set(R_KEYS) and all(np.isfinite(v) for v in lang_stats.values())
    assert len(preds) == 10
    res = json.load(open(tmp_path / 'capmi_val.json'))
    assert res['overall'] == lang_stats
    assert len(res['imgToEval']) == 10                            # 10 of the 12 images: num_images cuts the last batch
    assert all(np.isfinite(v['CIDEr']) and isinstance(v['caption'], str) for v in res['imgToEval'].values())
    assert np.mean([v['CIDEr'] for v in res['imgToEval'].values()]) == pytest.approx(lang_stats['CIDEr'], rel=1e-12)


def test_trainer_keeps_the_best_checkpoint_by_cider(tmp_path):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    T.train(_opts(SMALL + ['--max_iters', '6', '--val_every', '2', '--val_images', '8', '--save_checkpoint_every', '2',
                           '--language_eval', '1', '--learning_rate', '0.01', '--checkpoint_path', str(tmp_path)]))
    infos = pickle.load(open(tmp_path / 'infos_capmi.pkl', 'rb'))
    hist = infos['histories']['val_result_history']
    assert sorted(hist) == [2, 4, 6]
    ciders = [h['lang_stats']['CIDEr'] for h in hist.values()]
    assert all(set(h['lang_stats']) == set(R_KEYS) for h in hist.values())
    assert infos['best_val_score'] == max(ciders)                 # CIDEr, not -val_loss (which is negative)
    assert infos['best_val_score'] >= 0 and all(h['loss'] > 0 for h in hist.values())
    assert (tmp_path / 'model-best.pth').exists() and (tmp_path / 'infos_capmi-best.pkl').exists()
    best = pickle.load(open(tmp_path / 'infos_capmi-best.pkl', 'rb'))
    assert best['best_val_score'] == max(ciders) and best['iter'] == sorted(hist)[int(np.argmax(ciders))]
