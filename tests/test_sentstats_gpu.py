"""Device sentence statistics (csrc/sentset.hip, sentstats.py) through the C ABI against tests/sentstats_ref.py: novel_sentences,
vocab_size, bad_count_rate, mean perplexity / entropy.  Every count is an integer and every rate a ratio of two of them, so the
comparison is exact equality; only the two means carry a tolerance (MEASURED_* below).  Then tools/eval.py and tools/train.py end to
end with --sentence_stats 1.

Hash-equal sentences with different tokens: the 64-bit hash yields no such pair to a CPU search of a second, so the tests narrow
it with the descriptor's hash_mask (0xF: sixteen hash values, one tag), which makes every probe compare tokens."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import sentstats_ref as S

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
DEV = 'cuda:0'
COUNTS = ('rows', 'distinct', 'novel', 'first', 'bad')        # record [0..4]; record [5] is the bitmap's popcount


def _pad(rows, w, dtype=np.int64):
    out = np.zeros((len(rows), w), dtype=dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _run(train, chunks, first=None, vocab=40, unk=0, bad=(), **kw):
    """build, one `add` per chunk, one add_first -> (SentenceStats, compute())"""
    from imagecaptioning.pytorch_amd.sentstats import SentenceStats
    cap = kw.pop('capacity_rows', sum(len(c) for c in chunks))
    st = SentenceStats(train, DEV, vocab, unk, bad, cap, **kw)
    for c in chunks:
        st.add(torch.from_numpy(np.asarray(c, dtype=np.int64)).to(DEV))
    if first is not None:
        z = torch.zeros(len(first), dtype=torch.float32, device=DEV)
        st.add_first(torch.from_numpy(np.asarray(first, dtype=np.int64)).to(DEV), z, z)
    return st, st.compute()


def _check(st, got, train, chunks, first=None, unk=0, bad=()):
    rows_n = np.concatenate([np.asarray(c, dtype=np.int64) for c in chunks]) if chunks else np.zeros((0, 1), dtype=np.int64)
    want = S.on_ids(train if train is not None else [], rows_n, first if first is not None else [], unk, bad)
    rec = st.record
    assert {k: int(rec[i]) for i, k in enumerate(COUNTS)} == {k: want[k] for k in COUNTS}
    assert rec[8] == 0
    for k in ('novel_sentences', 'vocab_size', 'bad_count_rate'):
        assert got.get(k) == want.get(k), k                    # exact: integers and ratios of two integers
    assert isinstance(got.get('vocab_size', 0), int)
    return want


def _occupied(table):
    return int((table != 0).sum().item())


def _case(rng, w, vocab):
    """rows of every length that matters at width w (0, 1, w - 1, w: no terminator) among random ones; the generated rows repeat
    training rows, repeat each other, and carry tokens behind their first 0"""
    def row(ln):
        r = np.zeros(w, dtype=np.int64)
        r[:ln] = rng.integers(1, vocab + 1, size=ln)
        return r
    lens = sorted({0, 1, max(0, w - 1), w})
    train = [row(ln) for ln in lens] + [row(int(rng.integers(0, w + 1))) for _ in range(12)]
    train += [train[i].copy() for i in (1, 2, 5, 5)]
    gen = [row(ln) for ln in lens] + [row(int(rng.integers(0, w + 1))) for _ in range(10)] + [train[i].copy() for i in (0, 1, 3, 6, 7, 7)]
    gen += [gen[4].copy(), gen[5].copy()]
    for r in gen + train:
        ln = len(S.sentence(r))
        if ln + 1 < w and rng.integers(0, 2):
            r[ln + 1:] = rng.integers(0, vocab + 1, size=w - ln - 1)           # behind the first 0: ignored
    order = rng.permutation(len(gen))
    return np.stack(train), np.stack([gen[i] for i in order])


@pytest.mark.parametrize('w', [1, 5, 16, 20, 64])
def test_every_width_and_row_length(w):
    rng = np.random.default_rng(1000 + w)
    vocab = 3 if w == 1 else 9                                 # small: chance repeats and chance hits of the training set
    train, gen = _case(rng, w, vocab)
    if w in (5, 20):
        train = train.astype(np.uint32)                        # the label file's dtype
    first = gen[:7]
    st, got = _run(train, [gen[:9], gen[9:]], first, vocab=vocab, unk=2, bad=[1, 3])
    want = _check(st, got, train, [gen], first, unk=2, bad=[1, 3])
    assert 0 < want['novel'] < want['distinct'] < want['rows']
    assert _occupied(st.train_table) == len({s for s in map(S.sentence, train) if 2 not in s})


def test_prefixes_are_distinct_and_the_tail_behind_a_zero_is_not_read():
    train = _pad([[1, 2, 3], [4, 5]], 6)
    train[1, 3:] = [9, 9, 9]                                   # the sentence is still (4, 5)
    gen = _pad([[1, 2], [1, 2, 3], [1, 2, 3, 4], [4, 5], [4, 5], [6, 7]], 6)
    gen[3, 3:], gen[4, 3:] = [7, 0, 1], [0, 8, 8]              # equal up to the first 0, different behind it: one sentence, seen
    gen[5, 4] = 6
    st, got = _run(train, [gen])
    want = _check(st, got, train, [gen])
    assert (want['distinct'], want['novel'], want['vocab_size']) == (5, 3, 7)


def test_the_empty_sentence_counts_once_and_adds_no_word():
    gen = _pad([[], [], [3], []], 4)
    gen[1, 1:] = [5, 6, 7]                                     # still empty
    st, got = _run(None, [gen])
    want = _check(st, got, None, [gen])
    assert (want['distinct'], want['novel'], want['vocab_size']) == (2, 2, 1)
    st, got = _run(_pad([[]], 4), [gen])                       # an empty training caption: the empty sentence is seen
    assert _check(st, got, _pad([[]], 4), [gen])['novel'] == 1


def _race():
    others = [[7, 8], [5, 4, 3, 2, 1], [5]]
    a = _pad([[5, 4, 3]] * 64 + others, 8)
    a = a[np.random.default_rng(7).permutation(len(a))]
    b = _pad([[5, 4, 3], [7, 8]], 8)
    from imagecaptioning.pytorch_amd.sentstats import SentenceStats
    st = SentenceStats(_pad([[7, 8]], 8), DEV, 40, 0, [], 80)
    st.add(torch.from_numpy(a).to(DEV))
    st.compute()
    r1 = st.record.copy()
    st.add(torch.from_numpy(b).to(DEV))
    st.compute()
    return r1, st.record.copy(), _occupied(st.gen_table)


def test_equal_sentences_in_one_launch_count_once():
    r1, r2, occupied = _race()
    assert r1[:3].tolist() == [67, 4, 3] and r2[:3].tolist() == [69, 4, 3] and occupied == 4
    assert r1[5] == r2[5] == 7
    again = _race()                                            # whichever twin wins: the record is the same to the bit
    assert again[0].tobytes() == r1.tobytes() and again[1].tobytes() == r2.tobytes()


def _distinct_rows(rng, n, w, vocab, taken=()):
    seen, out = set(taken), []
    while len(out) < n:
        r = np.zeros(w, dtype=np.int64)
        ln = int(rng.integers(1, w + 1))
        r[:ln] = rng.integers(1, vocab + 1, size=ln)
        if S.sentence(r) not in seen:
            seen.add(S.sentence(r))
            out.append(r)
    return out


def test_a_crowded_training_table_and_its_duplicates():
    """16 slots, 12 distinct sentences in 40 rows: long probe chains that wrap round; duplicates take no slot"""
    rng = np.random.default_rng(11)
    base = _distinct_rows(rng, 12, 5, 6)
    train = np.stack(base + [base[int(i)] for i in rng.integers(0, 12, size=28)])
    gen = np.stack(base + _distinct_rows(rng, 8, 5, 6, taken=map(S.sentence, base)))
    st, got = _run(train, [gen], table_cap=16)
    want = _check(st, got, train, [gen])
    assert (want['distinct'], want['novel']) == (20, 8) and _occupied(st.train_table) == 12


def test_equal_hashes_are_told_apart_by_their_tokens():
    """hash_mask 0xF: 16 hash values for 20 (24) distinct sentences -- some are hash-equal and token-different, in both tables"""
    rng = np.random.default_rng(12)
    base = _distinct_rows(rng, 20, 6, 7)
    train = np.stack(base + base[:5])
    gen = np.stack(base[:10] + _distinct_rows(rng, 14, 6, 7, taken=map(S.sentence, base)) + base[:3])
    st, got = _run(train, [gen[:13], gen[13:]], table_cap=64, gen_table_cap=64, hash_mask=0xF)
    want = _check(st, got, train, [gen])
    assert (want['distinct'], want['novel']) == (24, 14)
    assert _occupied(st.train_table) == 20 and _occupied(st.gen_table) == 24
    words = st.train_table.cpu().numpy().view(np.uint64)
    assert (words[words != 0] >> np.uint64(32) == 0).all() and (words[16 + 20:] == 0).all()   # one tag; chains start in slots 0..15


def test_a_table_one_entry_too_small_is_reported():
    from imagecaptioning.pytorch_amd._lib import CapmiError
    rng = np.random.default_rng(13)
    rows = np.stack(_distinct_rows(rng, 17, 5, 6))
    missing = np.stack(_distinct_rows(rng, 4, 5, 6, taken=map(S.sentence, rows)))
    # 16 in 16: full, and looking a missing sentence up in a full table ends
    st, got = _run(rows[:16], [np.concatenate([rows[:16], missing])], table_cap=16, gen_table_cap=32)
    assert _check(st, got, rows[:16], [np.concatenate([rows[:16], missing])])['novel'] == 4
    with pytest.raises(CapmiError):                            # 17 in 16: the training set
        _run(rows, [rows[:1]], table_cap=16)
    st, got = _run(None, [rows[:16]], gen_table_cap=16, capacity_rows=17)
    assert got['novel_sentences'] == 1.0
    st.add(torch.from_numpy(rows[16:]).to(DEV))                # 17 in 16: the generated set
    with pytest.raises(CapmiError):
        st.compute()


def test_training_rows_with_unk_are_skipped():
    unk = 9
    train = _pad([[1, 9, 3], [1, 2, 3], [9], [4, 4]], 4)
    gen = _pad([[1, 9, 3], [1, 2, 3], [9], [4, 4], [4, 9]], 4)
    st, got = _run(train, [gen], unk=unk)
    want = _check(st, got, train, [gen], unk=unk)
    assert want['novel'] == 3 and _occupied(st.train_table) == 2
    st, got = _run(train, [gen], unk=0)                        # a vocabulary without UNK: nothing is skipped
    assert _check(st, got, train, [gen])['novel'] == 1 and _occupied(st.train_table) == 4


@pytest.mark.parametrize('v1', [33, 64, 65, 130])
def test_vocab_size_at_the_bitmap_word_edges(v1):
    from imagecaptioning.pytorch_amd._lib import CapmiError
    top = v1 - 1                                               # the largest id of the vocabulary
    ids = sorted({1, 31, 32, top - 1, top} | ({63, 64} if v1 > 64 else set()))
    gen = _pad([ids[:3], ids[3:], [top], [top, 1], []], 8)
    gen[4, 1:] = top                                           # behind the first 0: no word
    st, got = _run(None, [gen], vocab=top)
    want = _check(st, got, None, [gen])
    assert want['vocab_size'] == len(ids) and st.vocab_bits.numel() == (v1 + 31) // 32
    assert int(st.vocab_bits[0].item()) & 1 == 0               # token 0 is never counted
    with pytest.raises(CapmiError):                            # an id beyond the vocabulary: reported, nothing written for it
        _run(None, [_pad([[1, v1]], 8)], vocab=top)


def test_bad_count_rate():
    bad = [3, 17, 5]
    first = _pad([[1, 2, 3],                                   # ends in a bad word
                  [3, 17, 2],                                  # bad words inside, a good one last
                  [],                                          # empty: 0
                  [1, 2, 4, 6, 7, 17],                         # full width, no terminator, ends in a bad word
                  [5],
                  [2, 0, 3, 0, 0, 0]], 6)                      # the 3 is behind the first 0
    st, got = _run(None, [], first, bad=bad)
    want = _check(st, got, None, [], first, bad=bad)
    assert want['bad'] == 3 and got['bad_count_rate'] == 0.5 and 'novel_sentences' not in got and 'vocab_size' not in got
    st, got = _run(None, [], first, bad=[])                    # n_bad = 0
    assert _check(st, got, None, [], first)['bad'] == 0 and got['bad_count_rate'] == 0.0


# |float32 sum in index order - float64 sum| / float64 sum of the inputs below, measured on the CPU (numpy, sequential float32
# accumulation).  The kernel adds the same float32 inputs in double and in a fixed order, so 4 x this is what a float32 sum may miss.
# Observed on an MI355X: the device means equal the float64 ones to the last bit (deviation 0 for both).
MEASURED_PPL, MEASURED_ENT = 1.112e-07, 2.901e-09


def test_mean_perplexity_and_entropy():
    from imagecaptioning.pytorch_amd.sentstats import SentenceStats
    rng = np.random.default_rng(20240914)
    p = rng.uniform(1, 30, size=306).astype(np.float32)
    e = rng.uniform(0, 5, size=306).astype(np.float32)
    for x, measured in ((p, MEASURED_PPL), (e, MEASURED_ENT)):    # the stated figures are the ones this input gives
        s64 = x.astype(np.float64).sum()
        assert abs(float(np.cumsum(x, dtype=np.float32)[-1]) - s64) / s64 == pytest.approx(measured, rel=1e-3)
    records = []
    for _ in range(2):
        st = SentenceStats(None, DEV, 40, 0, [], 0)
        seq = torch.ones(306, 4, dtype=torch.long, device=DEV)
        for a, b in ((0, 5), (5, 305), (305, 306)):            # 300 rows in one launch: more rows than threads
            st.add_first(seq[a:b], torch.from_numpy(p[a:b]).to(DEV), torch.from_numpy(e[a:b]).to(DEV))
        got = st.compute()
        records.append(st.record.tobytes())
    want_p, want_e = S.means(p, e)
    err_p, err_e = abs(got['perplexity'] - want_p) / want_p, abs(got['entropy'] - want_e) / want_e
    print('sentstats means: relative deviation perplexity %.3e entropy %.3e' % (err_p, err_e))
    assert err_p <= 4 * MEASURED_PPL and err_e <= 4 * MEASURED_ENT
    assert records[0] == records[1] and int(st.record[3]) == 306


def test_rows_beyond_the_contract_are_refused():
    from imagecaptioning.pytorch_amd.sentstats import SentenceStats
    from imagecaptioning.pytorch_amd._lib import CapmiError
    with pytest.raises(ValueError):
        SentenceStats(np.zeros((2, 65), dtype=np.int64), DEV, 40, 0, [], 4)
    with pytest.raises(ValueError):
        SentenceStats(None, DEV, 65535, 0, [], 4)              # ids must stay below 65535
    st = SentenceStats(None, DEV, 65534, 0, [], 4)
    z = torch.zeros(1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        st.add(torch.zeros(1, 65, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError):
        st.add_first(torch.zeros(1, 65, dtype=torch.long, device=DEV), z, z)
    with pytest.raises(ValueError):
        st.add(torch.zeros(5, 4, dtype=torch.long, device=DEV))          # more rows than it was sized for
    st.add(torch.tensor([[65534, 1, 0, 0]], device=DEV))
    assert st.compute()['vocab_size'] == 2
    st.add(torch.tensor([[1, 65535, 0, 0]], device=DEV))
    with pytest.raises(CapmiError):
        st.compute()
    st.reset()
    st.add_first(torch.tensor([[65535, 0]], device=DEV), z, z)
    with pytest.raises(CapmiError):
        st.compute()
    with pytest.raises(CapmiError):                            # in the training rows: the constructor reports it
        SentenceStats(np.array([[1, 65535]], dtype=np.int64), DEV, 40, 0, [], 4)


# ---- end to end, at the synthetic sizes of tests/test_langeval_gpu.py
SMALL = ['--caption_model', 'updown', '--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--fc_feat_size', '24',
         '--att_feat_size', '24', '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6', '--max_length', '6',
         '--batch_size', '4', '--seq_per_img', '2', '--synthetic_images', '12']
LANG_KEYS = {'Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDEr'}
FIRST_KEYS = {'bad_count_rate', 'perplexity', 'entropy'}
N_KEYS = {'novel_sentences', 'vocab_size'}


def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


def _eval(tmp_path, extra):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    opt = _opts(SMALL + ['--num_images', '10', '--language_eval', '1', '--split', 'val', '--eval_results_dir', str(tmp_path)] + extra)
    loss, preds, lang_stats = E.main(opt)
    return opt, preds, lang_stats, json.load(open(tmp_path / 'capmi_val.json'))


def _first_numbers(preds, lang_stats):
    """the single-caption keys against the restatement on the returned predictions.  The means: float64 sums of at most 10 float32
    values on both sides, in two orders -- each side is within 10 roundings of 2^-53 of the exact mean."""
    want = S.strings_stats(set(), [], [p['caption'] for p in preds])
    assert lang_stats['bad_count_rate'] == want['bad_count_rate']
    want_p, want_e = S.means([p['perplexity'] for p in preds], [p['entropy'] for p in preds])
    assert lang_stats['perplexity'] == pytest.approx(want_p, rel=20 * 2.0 ** -53)
    assert lang_stats['entropy'] == pytest.approx(want_e, rel=20 * 2.0 ** -53)
    assert want_p > 0 and want_e > 0


def test_eval_entrypoint_sample_n_reports_the_five_keys(tmp_path):
    opt, preds, lang_stats, res = _eval(tmp_path, ['--sentence_stats', '1', '--sample_n', '3', '--sample_n_method', 'sample'])
    from captioning.data.synthetic_loader import SyntheticLoader
    assert FIRST_KEYS | N_KEYS <= set(lang_stats) and LANG_KEYS <= set(lang_stats)
    # <id>_<split>.json is written before the diversity numbers join lang_stats: the scorers' keys and the five new ones
    assert set(res['overall']) == LANG_KEYS | FIRST_KEYS | N_KEYS and len(preds) == 10
    assert res['overall'] == {k: lang_stats[k] for k in res['overall']}
    _first_numbers(preds, lang_stats)
    # the sample_n captions of the ten images that count, as <id>_<split>_n.json lists them (model.n_predictions cut at num_images)
    groups = json.load(open(tmp_path / 'capmi_val_n.json'))['div_stats']['ImgToEval']
    captions_n = [c['caption'] for g in groups.values() for c in g['individuals']]
    assert len(groups) == 10 and len(captions_n) == 30
    loader = SyntheticLoader(opt)
    want = S.strings_stats(S.training_strings(loader.get_vocab(), loader.training_captions()), captions_n, [])
    assert lang_stats['novel_sentences'] == want['novel_sentences'] and lang_stats['vocab_size'] == want['vocab_size']
    assert isinstance(lang_stats['vocab_size'], int) and 0 < lang_stats['novel_sentences'] <= 1


def test_eval_entrypoint_single_caption_reports_three_keys(tmp_path):
    opt, preds, lang_stats, res = _eval(tmp_path, ['--sentence_stats', '1'])
    assert set(lang_stats) == LANG_KEYS | FIRST_KEYS and res['overall'] == lang_stats
    _first_numbers(preds, lang_stats)


def test_eval_entrypoint_without_the_switch_is_unchanged(tmp_path):
    opt, preds, lang_stats, res = _eval(tmp_path, ['--sentence_stats', '0'])
    assert set(lang_stats) == LANG_KEYS and set(res['overall']) == LANG_KEYS


def test_trainer_history_carries_the_single_caption_keys(tmp_path):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    T.train(_opts(SMALL + ['--max_iters', '2', '--val_every', '2', '--val_images', '8', '--save_checkpoint_every', '2', '--language_eval', '1',
                           '--sentence_stats', '1', '--learning_rate', '0.01', '--checkpoint_path', str(tmp_path)]))
    infos = pickle.load(open(tmp_path / 'infos_capmi.pkl', 'rb'))
    stats = infos['histories']['val_result_history'][2]['lang_stats']
    assert set(stats) == LANG_KEYS | FIRST_KEYS
    assert 0 <= stats['bad_count_rate'] <= 1 and stats['perplexity'] > 0 and stats['entropy'] > 0
