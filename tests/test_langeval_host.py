"""language_eval without a GPU: the float64 restatement (tests/langeval_ref64.py) against closed-form cases of coco-caption's
Cider / Bleu / Rouge formulas, the ctypes twin of capmi_langeval, and the option parsing of the entrypoints."""
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

import langeval_ref64 as R

PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')


def test_identical_hypothesis_scores_one_and_ten():
    # two images with disjoint vocabularies: every n-gram of image 0 is in 1 of 2 images -> idf = log 2 != 0
    refs = [[[1, 2, 3, 4, 5, 0, 0, 0]], [[6, 7, 8, 9, 10, 0, 0, 0]]]
    out = R.evaluate(refs, [[1, 2, 3, 4, 5, 0, 0, 0], [6, 7, 8, 9, 10, 0, 0, 0]])
    for k in range(1, 5):
        # (c + 1e-15) / (c + 1e-9): coco-caption's constants keep the ratio a hair below 1
        assert out['Bleu_%d' % k] == pytest.approx(1.0, abs=1e-8)
    assert out['ROUGE_L'] == pytest.approx(1.0, abs=1e-15)
    assert out['CIDEr'] == pytest.approx(10.0, rel=1e-14)
    np.testing.assert_allclose(out['cider_img'], [10.0, 10.0], rtol=1e-14)
    assert out['totals'].tolist() == [10, 8, 6, 4, 10, 8, 6, 4, 10, 10]


def test_zero_idf_gives_zero_cider():
    # one image: ref_len = log 1 = 0, every weight is 0 (the reason the case above needs two images)
    out = R.evaluate([[[1, 2, 3, 0]]], [[1, 2, 3, 0]])
    assert out['CIDEr'] == 0.0 and out['ROUGE_L'] == pytest.approx(1.0)


def test_disjoint_tokens_score_zero():
    refs = [[[1, 2, 3, 4, 0, 0]], [[1, 2, 3, 4, 0, 0]]]
    out = R.evaluate(refs, [[5, 6, 7, 8, 0, 0], [9, 10, 11, 5, 0, 0]])
    assert out['CIDEr'] == 0.0 and out['ROUGE_L'] == 0.0
    assert out['totals'][4:8].tolist() == [0, 0, 0, 0]
    for k in range(1, 5):
        assert out['Bleu_%d' % k] < 1e-5              # tiny / small, not a division by zero


def test_brevity_penalty_of_a_hypothesis_one_token_short():
    refs = [[[1, 2, 3, 4, 5, 6, 0, 0]], [[7, 8, 9, 0, 0, 0, 0, 0]]]
    out = R.evaluate(refs, [[1, 2, 3, 4, 5, 0, 0, 0], None])
    c, r = 5, 6
    assert out['totals'][8:].tolist() == [c, r]
    # every n-gram of the hypothesis is in the reference: precision 1, so Bleu_n is the penalty alone
    for k in range(1, 5):
        assert out['Bleu_%d' % k] == pytest.approx(math.exp(1 - r / c), rel=1e-8)
    # lcs = 5: P = 1, R = 5/6
    p, q, b2 = 1.0, 5 / 6, 1.2 ** 2
    assert out['ROUGE_L'] == pytest.approx((1 + b2) * p * q / (q + b2 * p), rel=1e-14)


def test_closest_reference_length_tie_goes_to_the_shorter():
    refs = [[[1, 2, 3, 4, 5, 6, 7, 0], [1, 2, 3, 0, 0, 0, 0, 0]]]       # lengths 7 and 3, hypothesis 5: |7-5| == |3-5|
    g, c, tl, rl = R.bleu_stats_image([1, 2, 3, 4, 5, 0, 0, 0], refs[0])
    assert (tl, rl) == (5, 3)
    refs = [[[1, 2, 3, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6, 7, 0]]]       # ... whatever the order of the references
    assert R.bleu_stats_image([1, 2, 3, 4, 5, 0, 0, 0], refs[0])[3] == 3


def test_clipping_uses_the_maximum_count_over_the_references():
    refs = [[2, 2, 3, 0, 0, 0], [2, 4, 0, 0, 0, 0]]
    g, c, tl, rl = R.bleu_stats_image([2, 2, 2, 2, 0, 0], refs)
    assert g == [4, 3, 2, 1] and c == [2, 1, 0, 0] and (tl, rl) == (4, 3)


def test_a_row_without_a_zero_is_a_full_length_caption_and_an_empty_one_scores_zero():
    assert R.caption([3, 4, 5]) == [3, 4, 5] and R.caption([0, 4, 5]) == []
    refs = [[[1, 2, 3, 4]], [[5, 6, 7, 0]]]
    out = R.evaluate(refs, [[0, 0, 0, 0], [5, 6, 7, 0]])
    assert out['cider_img'][0] == 0.0 and out['rouge_img'][0] == 0.0 and out['stats'][0] == ([0, 0, 0, 0], [0, 0, 0, 0], 0, 4)


def test_lcs_is_a_subsequence_not_a_substring():
    assert R.lcs([1, 2, 3, 4, 5], [1, 9, 3, 9, 5]) == 3 and R.lcs([], [1]) == 0 and R.lcs([1, 2], [2, 1]) == 1


def test_langeval_struct_layout_matches_header():
    """Field order of the ctypes struct == field order in include/capmi.h (same parsing as tests/test_abi.py)."""
    from imagecaptioning.pytorch_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'capmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)

    def fields(struct):
        body = re.search(r'typedef struct (?:%s )?\{([^{}]*?)\} %s;' % (struct, struct), src, flags=re.S).group(1)
        names = []
        for stmt in body.split(';'):
            stmt = stmt.strip()
            if not stmt:
                continue
            for part in stmt.split(','):
                names.append(re.findall(r'(\w+)\s*(?:\[\w+\])?$', part.strip())[0])
        return names

    assert fields('capmi_langeval') == [f[0] for f in _lib.LangEval._fields_]
    assert int(re.search(r'#define CAPMI_LANGEVAL_LMAX (\d+)', src).group(1)) == _lib.LANGEVAL_LMAX
    for name in ('TABLE_FULL', 'TOKEN', 'IMAGE'):
        assert int(re.search(r'#define CAPMI_LANGEVAL_E_%s (\d+)' % name, src).group(1)) == getattr(_lib, 'LANGEVAL_E_' + name)
    for fn in ('capmi_langeval_build', 'capmi_langeval_add', 'capmi_langeval_reduce'):
        assert fn in _lib.SIGNATURES


def test_entrypoints_accept_language_eval():
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import eval_ensemble as EE
    assert opts.parse_opt([]).language_eval == 0
    o = opts.parse_opt(['--language_eval', '1', '--eval_results_dir', 'x'])
    assert o.language_eval == 1 and o.eval_results_dir == 'x'
    # the ensemble tool takes it from its own command line, never from a member's training options
    assert EE.parse_args(['--ids', 'a', '--language_eval', '1'])[3] == {'language_eval': 1}
    assert 'language_eval' in EE.EVAL_KEYS


def test_loader_hands_out_the_references_of_a_split():
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    from captioning.data.synthetic_loader import SyntheticLoader
    ld = SyntheticLoader(opts.parse_opt(['--vocab_size', '20', '--seq_length', '6', '--synthetic_images', '5', '--batch_size', '2']))
    rows, off, ids = ld.language_eval_refs('val')
    assert rows.shape == (25, 6) and rows.dtype == np.int64 and off.tolist() == [0, 5, 10, 15, 20, 25] and ids == [0, 1, 2, 3, 4]
    np.testing.assert_array_equal(rows[10:15], ld.refs[2])
