"""Device diversity evaluation (csrc/langeval.hip capmi_diveval_*, diveval.py) against the float64 restatement
tests/diveval_ref64.py: Div1 / Div2 / gDiv1, mBLEU, self-CIDEr and the oracle scores of sample_n captions per image.  Integers
(distinct counts, token totals, the mBLEU counts, the gDiv1 count) must match exactly and K must be exactly symmetric; floats are
held within REL_TOL where K has full rank, and within the backward-error bound of a symmetric eigensolver where it has not.  Then
tools/eval.py end to end with --sample_n."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import diveval_ref64 as D
from test_langeval_gpu import R_KEYS, SMALL, _general as _langeval_general, _opts, _rel, _row

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
DEV = 'cuda:0'

# Largest relative deviation of a float (K, eig, self_cider, sentence Bleu_2, the oracle scores, every overall number) from
# diveval_ref64.py over the full-rank cases of this file, measured on an MI355X: MEASURED_REL.  The kernels work in double and in
# a fixed order; the deviation comes from the order of the n-gram sums (a dict's order in the restatement), the device's log /
# sqrt / pow / exp and, for eig, cyclic Jacobi against LAPACK's tridiagonal QL, both backward stable (lambda_min > 1e-3 keeps
# that relative).  The bound is 4 x the measured value.
MEASURED_REL = 3.313e-15       # general n = 2: 2.709e-15; n = 5: 3.171e-15; n = 32: 3.313e-15; two chunks (n = 5): 3.171e-15
REL_TOL = 4 * MEASURED_REL

OVERALL = ('Div1', 'Div2', 'gDiv1', 'mBLeu_1', 'mBLeu_2', 'mBLeu_3', 'mBLeu_4', 'self_cider')


def _general(n):
    """the 7 images and references of test_langeval_gpu._general, n captions per image of 3..8 tokens, vocabulary 12, L = 8; one
    caption copies most of a reference, one most of its neighbour, so that higher orders match and clip"""
    refs, _ = _langeval_general()
    rng = np.random.default_rng(20241017 + n)
    groups = [[_row(rng, int(rng.integers(3, 9)), 8, 12) for _ in range(n)] for _ in refs]
    groups[4][0] = refs[4][2].copy()
    groups[4][0][1] = groups[4][0][0]
    groups[2][1] = groups[2][0].copy()
    groups[2][1][2] = 1 + groups[2][1][2] % 11
    return refs, groups


def _degenerate():
    """n = 4, L = 8: rank-deficient K and missing orders"""
    refs, _ = _langeval_general()
    z = [0] * 8
    groups = [[[3, 4, 5, 6, 7, 0, 0, 0]] * 4,                                                          # identical captions
              [z] * 4,                                                                                 # all empty
              [[1, 2, 3, 4, 0, 0, 0, 0], z, [2, 3, 4, 5, 6, 0, 0, 0], [1, 2, 9, 9, 9, 9, 0, 0]],       # one empty among others
              [[5, 0, 0, 0, 0, 0, 0, 0], [5, 6, 0, 0, 0, 0, 0, 0], [5, 6, 7, 0, 0, 0, 0, 0], [6, 0, 0, 0, 0, 0, 0, 0]],   # orders missing
              [[1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1], [0, 1, 2, 3, 4, 5, 6, 7]],   # no terminating 0
              None,                                                                                    # an image without a group
              [[9, 9, 9, 9, 9, 9, 9, 9], [9, 9, 0, 0, 0, 0, 0, 0], [9, 0, 9, 9, 0, 0, 0, 0], [10, 9, 0, 0, 0, 0, 0, 0]]]
    return refs, [None if g is None else [np.array(r, dtype=np.int64) for r in g] for g in groups]


def _long():
    """n = 3, L = 64: the compiled bound, rows that fill it"""
    rng = np.random.default_rng(64)
    refs = [[_row(rng, 40, 64, 12)], [_row(rng, 64, 64, 12), _row(rng, 7, 64, 12)]]
    groups = [[_row(rng, 64, 64, 12), _row(rng, 64, 64, 12), _row(rng, 33, 64, 12)],
              [refs[1][0].copy(), refs[1][0].copy(), _row(rng, 1, 64, 12)]]
    return refs, groups


def _device_eval(refs, groups, n, oracle=True, chunks=None):
    """chunks: list of lists of image positions (or (position, group) pairs), one `add` each; default: one call, split order"""
    from imagecaptioning.pytorch_amd.langeval import LanguageEval
    from imagecaptioning.pytorch_amd.diveval import DiversityEval
    le = LanguageEval.from_gts([np.stack(image) for image in refs], DEV)
    de = DiversityEval(le, n, oracle=oracle)
    for chunk in (chunks if chunks is not None else [[i for i, g in enumerate(groups) if g is not None]]):
        rows = np.concatenate([np.stack(groups[i] if isinstance(i, int) else i[1]) for i in chunk])
        de.add([i if isinstance(i, int) else i[0] for i in chunk], torch.from_numpy(rows).to(DEV))
    overall, per_image = de.compute()
    return de, overall, per_image


def _check(de, overall, per_image, refs, groups, label, full_rank, gdiv1=None):
    """integers exact, K symmetric; floats within REL_TOL (full_rank) or the eigensolver's bound; returns the largest relative
    deviation of the floats held to REL_TOL (printed: run with -s to measure)"""
    n = de.n
    want = D.evaluate(refs, groups, oracle=de.oracle)
    seen = want['seen']
    np.testing.assert_array_equal(per_image['seen'], seen)
    assert de.n_added == int(seen.sum())
    np.testing.assert_array_equal(de.distinct.cpu().numpy()[seen], want['distinct'][seen])
    np.testing.assert_array_equal(de.tokens.cpu().numpy()[seen], want['tokens'][seen])
    np.testing.assert_array_equal(de.mbleu_stats.cpu().numpy()[seen], want['mbleu_stats'][seen])
    np.testing.assert_array_equal(de._totals.cpu().numpy(), want['totals'])
    assert overall['gDiv1'] == (want['overall']['gDiv1'] if gdiv1 is None else gdiv1)
    K = per_image['self_cider_mat'][seen]
    np.testing.assert_array_equal(K, K.transpose(0, 2, 1))
    assert all(np.isfinite(v) for v in overall.values()) and all(np.isfinite(per_image[k][seen]).all() for k in per_image)
    assert set(overall) == set(want['overall'])
    devs = [_rel(K, want['K'][seen]), _rel(per_image['individual_mBleu_2'][seen], want['sent_bleu2'][seen]),
            _rel(per_image['mBleu_2'][seen], want['sent_bleu2'][seen].mean(axis=1)),
            _rel([overall[k] for k in overall if k != 'self_cider'], [want['overall'][k] for k in overall if k != 'self_cider'])]
    if de.oracle:
        devs.append(_rel(per_image['scores'][seen], want['scores'][seen]))
    if full_rank:
        devs += [_rel(per_image['eig'][seen], want['eig'][seen]), _rel(per_image['self_cider'][seen], want['self_cider'][seen]),
                 _rel(overall['self_cider'], want['overall']['self_cider'])]
    else:
        # backward error of a symmetric eigensolver on K/10 (entries <= 1, norm <= n), both solvers: delta absolute on eig;
        # self_cider = -log(sqrt(l_max) / s) / log n with s = sum sqrt(l), and |sqrt(a) - sqrt(b)| <= sqrt(|a - b|)
        delta = 64 * n * n * 2.0 ** -52
        assert np.abs(per_image['eig'][seen] - want['eig'][seen]).max() <= delta, label
        s = np.sqrt(np.clip(want['eig'][seen], 0, None)).sum(axis=1)
        got, ref = per_image['self_cider'][seen], want['self_cider'][seen]
        assert (got[s == 0] == 0.0).all(), label
        bound = n * np.sqrt(delta) / (s[s > 0] * np.log(n))
        assert (np.abs(got - ref)[s > 0] <= bound).all(), (label, np.abs(got - ref)[s > 0], bound)
        assert abs(overall['self_cider'] - want['overall']['self_cider']) <= bound.sum() / len(s), label
    dev = max(devs)
    print('diveval %s: max relative deviation %.3e' % (label, dev))
    assert dev <= REL_TOL, (label, dev, devs)
    return dev


@pytest.mark.parametrize('n', [2, 5, 32])
def test_general_case_matches_the_restatement(n):
    refs, groups = _general(n)
    # condition, not measurement: the relative bound on eig and self_cider needs K/10 well away from singular
    want = D.evaluate(refs, groups, oracle=True)
    assert want['eig'].min() > 1e-3 and REL_TOL <= 1e-11
    de, overall, per_image = _device_eval(refs, groups, n)
    _check(de, overall, per_image, refs, groups, 'general n = %d' % n, full_rank=True)
    assert overall['oracle_CIDEr'] >= overall['avg_CIDEr'] > 0 and 0 < overall['self_cider'] < 1
    assert overall['mBLeu_2'] > 1e-3 and (overall['mBLeu_4'] > 1e-3 or n < 32)      # the case exercises the higher orders


def test_rank_deficient_and_degenerate_groups():
    refs, groups = _degenerate()
    de, overall, per_image = _device_eval(refs, groups, 4)
    _check(de, overall, per_image, refs, groups, 'degenerate', full_rank=False)
    assert per_image['self_cider'][1] == 0.0 and not per_image['self_cider_mat'][1].any()      # all empty: 0.0, nothing NaN
    assert abs(per_image['self_cider'][0]) < 1e-6                                             # identical captions: no diversity
    assert not per_image['seen'][5]


def test_rows_at_the_compiled_bound():
    refs, groups = _long()
    de, overall, per_image = _device_eval(refs, groups, 3)
    _check(de, overall, per_image, refs, groups, 'L = 64', full_rank=False)
    assert de.tokens.cpu().numpy().tolist() == [64 + 64 + 33, 64 + 64 + 1]


def test_chunks_in_another_order_give_the_same_bits():
    refs, groups = _general(5)
    de, overall, per_image = _device_eval(refs, groups, 5)
    de2, overall2, per_image2 = _device_eval(refs, groups, 5, chunks=[[5, 2, 6, 0], [3, 1, 4]])
    _check(de2, overall2, per_image2, refs, groups, 'two chunks', full_rank=True)
    assert overall2 == overall
    for k in per_image:
        np.testing.assert_array_equal(per_image2[k], per_image[k], err_msg=k)


def test_a_later_group_replaces_the_earlier_one():
    refs, groups = _general(5)
    other = [r.copy() for r in groups[5]]
    other[0][:3] = [11, 11, 11]                    # token 11 may occur nowhere else: gDiv1 still counts it after the replacement
    # image 2 first gets another group, then (in the same call: the later entry counts) its own; image 0 is replaced by a later
    # call; image 6 never gets a group
    de, overall, per_image = _device_eval(refs, groups, 5, chunks=[[(2, other), 0, 1, 2, 3], [4, 5, (0, other)]])
    final = list(groups)
    final[0], final[6] = other, None
    # gDiv1's bitmap is the union of everything added since reset(), replaced groups included
    union = set()
    for g in groups[:6] + [other]:
        union |= D.distinct(g, 1)
    _check(de, overall, per_image, refs, final, 'replacement', full_rank=False, gdiv1=float(len(union)))
    de.reset()
    de.add([1], torch.from_numpy(np.stack(groups[1])).to(DEV))
    assert de.compute()[0]['gDiv1'] == float(len(D.distinct(groups[1], 1)))


def test_bad_arguments_are_refused_before_any_launch():
    from imagecaptioning.pytorch_amd.langeval import LanguageEval
    from imagecaptioning.pytorch_amd.diveval import DiversityEval
    refs, groups = _general(2)
    le = LanguageEval.from_gts([np.stack(image) for image in refs], DEV)
    for n in (1, 33):
        with pytest.raises(ValueError, match='sample_n'):
            DiversityEval(le, n)
    de = DiversityEval(le, 3)
    with pytest.raises(ValueError, match='seqs'):                 # 7 rows are not 2 groups of 3
        de.add([0, 1], torch.zeros(7, 8, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match='seqs'):
        de.add([0], torch.zeros(3, 65, dtype=torch.long, device=DEV))
    with pytest.raises(ValueError, match='seqs'):
        de.add([0], torch.zeros(3, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='seqs'):
        de.add([0], torch.zeros(3, 8, dtype=torch.long))
    assert not de.seen.any() and not de.vocab_bits.any()          # nothing was launched


def _run_eval(tmp_path, name, extra):
    """tools/eval.py on the synthetic loader; returns (result tuple, out dir, the (positions, rows) every DiversityEval.add saw)"""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    from imagecaptioning.pytorch_amd import diveval
    out_dir = tmp_path / name
    seen_adds, orig = [], diveval.DiversityEval.add

    def spy(self, image_index, seqs):
        seen_adds.append((list(image_index), seqs.detach().reshape(-1, seqs.shape[-1]).cpu().numpy().copy()))
        return orig(self, image_index, seqs)
    diveval.DiversityEval.add = spy
    try:
        res = E.main(_opts(SMALL + ['--num_images', '6', '--language_eval', '1', '--split', 'val', '--eval_results_dir', str(out_dir)]
                           + extra))
    finally:
        diveval.DiversityEval.add = orig
    return res, out_dir, seen_adds


@pytest.mark.parametrize('method,extra', [('bs', []), ('dbs', ['--beam_size', '2']), ('sample', []), ('dtop5', [])])
def test_eval_entrypoint_reports_diversity(tmp_path, method, extra):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    from imagecaptioning.pytorch_amd.diveval import ORACLE_KEYS
    n = 3
    oracle_keys = {p + k for k in ORACLE_KEYS for p in ('oracle_', 'avg_')}
    single, single_dir, adds = _run_eval(tmp_path, 'single', ['--sample_n', '1'] + extra)
    assert set(single[2]) == set(R_KEYS) and not adds and sorted(os.listdir(single_dir)) == ['capmi_val.json']
    for oracle in (0, 1):
        res, out_dir, adds = _run_eval(tmp_path, 'n%d' % oracle, ['--sample_n', str(n), '--sample_n_method', method, '--eval_oracle',
                                                                  str(oracle)] + extra)
        loss, preds, lang_stats = res
        assert set(lang_stats) == set(R_KEYS) | set(OVERALL) | (oracle_keys if oracle else set())
        assert all(np.isfinite(v) for v in lang_stats.values())
        # the single-caption pass is what it was: the same loss, predictions, scores and file as with --sample_n 1
        assert loss == single[0] and preds == single[1] and {k: lang_stats[k] for k in R_KEYS} == single[2]
        assert json.load(open(out_dir / 'capmi_val.json')) == json.load(open(single_dir / 'capmi_val.json'))
        out = json.load(open(out_dir / 'capmi_val_n.json'))
        assert set(out) == ({'div_stats', 'self_cider', 'oracle'} if oracle else {'div_stats', 'self_cider'})
        assert out['div_stats']['overall'] == {k: lang_stats[k] for k in OVERALL if k != 'self_cider'}
        per = out['self_cider']['imgToEval']
        assert len(per) == 6 and set(per) == set(out['div_stats']['ImgToEval'])
        assert np.mean([v['self_cider'] for v in per.values()]) == pytest.approx(lang_stats['self_cider'], rel=1e-12, abs=1e-300)
        for v in out['div_stats']['ImgToEval'].values():
            assert len(v['individuals']) == n and all(isinstance(p['caption'], str) for p in v['individuals'])
            assert np.mean([p['mBleu_2'] for p in v['individuals']]) == pytest.approx(v['mBleu_2'], rel=1e-12)
        if oracle:
            assert lang_stats['oracle_CIDEr'] >= lang_stats['avg_CIDEr']
            for k in oracle_keys:
                assert np.mean([v[k] for v in out['oracle']['ImgToEval'].values()]) == pytest.approx(lang_stats[k], rel=1e-12, abs=1e-300)
        # rescoring the token rows the evaluator was given, through the restatement
        opt = _opts(SMALL + ['--split', 'val'])
        loader, _ = E.build_loader(opt, torch.device(DEV))
        rows, off, ids = loader.language_eval_refs('val')
        rows, off = np.asarray(rows), np.asarray(off)
        refs = [[rows[r] for r in range(off[i], off[i + 1])] for i in range(len(off) - 1)]
        groups = [None] * len(refs)
        for positions, seqs in adds:
            assert seqs.shape[0] == len(positions) * n
            for j, p in enumerate(positions):
                groups[p] = list(seqs[j * n:(j + 1) * n])
        assert sum(g is not None for g in groups) == 6
        want = D.evaluate(refs, groups, oracle=bool(oracle))
        delta = 64 * n * n * 2.0 ** -52
        s = np.sqrt(np.clip(want['eig'][want['seen']], 0, None)).sum(axis=1)
        bound = np.where(s > 0, n * np.sqrt(delta) / (np.maximum(s, 1e-300) * np.log(n)), 0.0)
        for k in lang_stats:
            if k in R_KEYS:
                continue
            if k == 'self_cider':
                assert abs(lang_stats[k] - want['overall'][k]) <= bound.mean(), (k, lang_stats[k], want['overall'][k])
            else:
                assert _rel(lang_stats[k], want['overall'][k]) <= REL_TOL, (k, lang_stats[k], want['overall'][k])
        pos_of = {str(ix): i for i, ix in enumerate(ids)}      # the synthetic loader's infos[k]['id'] is the image's ix
        for image_id, v in per.items():
            pos = pos_of[image_id]
            assert _rel(np.array(v['self_cider_mat']), want['K'][pos]) <= REL_TOL
            assert _rel([p['mBleu_2'] for p in out['div_stats']['ImgToEval'][image_id]['individuals']], want['sent_bleu2'][pos]) <= REL_TOL
