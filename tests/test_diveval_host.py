"""Diversity evaluation without a GPU: the float64 restatement (tests/diveval_ref64.py) against the reference's own div_utils.py
(tests/golden/diveval_ref.npz) and closed-form cases of mBLEU / self-CIDEr, the ctypes twin of capmi_diveval, the new option and
the assembly of <id>_<split>_n.json."""
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import diveval_ref64 as D

PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')


def test_restatement_reproduces_the_reference_div_utils():
    z = np.load(os.path.join(GOLDEN, 'diveval_ref.npz'))
    groups = [list(g) for g in z['groups']]
    assert any(not D.R.caption(r) for g in groups for r in g)                        # the fixture holds an empty caption
    assert any(all((r == g[0]).all() for r in g) for g in groups)                    # and an image of identical captions
    for k, (mean, per) in ((1, (z['div1'], z['div1_img'])), (2, (z['div2'], z['div2_img']))):
        got_mean, got_per = D.div_n(groups, k)
        np.testing.assert_allclose(got_per, per, rtol=1e-15, atol=0)
        np.testing.assert_allclose(got_mean, mean, rtol=1e-15, atol=0)
    assert D.global_div_1(groups) == float(z['gdiv1'])
    # evaluate() reports the same three numbers (the references only feed the idf, which Div-n does not read)
    out = D.evaluate([[g[0]] for g in groups], groups)
    np.testing.assert_allclose([out['overall']['Div1'], out['overall']['Div2']], [z['div1'], z['div2']], rtol=1e-15, atol=0)
    assert out['overall']['gDiv1'] == float(z['gdiv1'])
    np.testing.assert_allclose(out['distinct'][:, 0] / (1e-6 + out['tokens']), z['div1_img'], rtol=1e-15, atol=0)


REFS = [[[1, 2, 3, 4, 5, 0, 0, 0]], [[6, 7, 8, 9, 10, 0, 0, 0]]]        # two images: idf = log 2 or log 2 - log 1, never 0


@pytest.mark.parametrize('n', [2, 5])
def test_identical_captions_have_no_diversity(n):
    groups = [[[1, 2, 3, 4, 5, 0, 0, 0]] * n, [[7, 7, 8, 9, 0, 0, 0, 0]] * n]
    out = D.evaluate(REFS, groups)
    np.testing.assert_allclose(out['K'], 10.0, rtol=1e-14)
    # K/10 is the all-ones matrix: one eigenvalue n, the others 0 up to eigvalsh's backward error (sqrt is not Lipschitz at 0)
    assert np.abs(out['self_cider']).max() <= n * np.sqrt(64 * n * n * 2.0 ** -52) / (np.sqrt(n) * np.log(n))
    for k in range(1, 5):
        assert out['overall']['mBLeu_%d' % k] == pytest.approx(1.0, abs=1e-8)       # (c + 1e-15) / (c + 1e-9): a hair below 1
    np.testing.assert_allclose(out['sent_bleu2'], 1.0, atol=1e-8)
    assert out['distinct'].tolist() == [[5, 4], [3, 3]] and out['tokens'].tolist() == [5 * n, 4 * n]


@pytest.mark.parametrize('n', [2, 5])
def test_disjoint_captions_are_fully_diverse(n):
    ln = 4
    groups = [[[1 + s * ln + j for j in range(ln)] + [0] * 4 for s in range(n)],
              [[100 + s * (ln + 1) + j for j in range(ln + 1)] + [0] * 3 for s in range(n)]]
    out = D.evaluate(REFS, groups)
    for i in range(2):
        np.testing.assert_allclose(out['K'][i], 10.0 * np.eye(n), rtol=1e-14, atol=0)
    np.testing.assert_allclose(out['self_cider'], 1.0, rtol=1e-14)
    total = np.array([n * ln, n * (ln + 1)], dtype=np.float64)
    np.testing.assert_allclose(out['distinct'][:, 0] / (1e-6 + out['tokens']), 1.0 / (1.0 + 1e-6 / total), rtol=1e-15)
    assert out['overall']['Div1'] == pytest.approx(np.mean(1.0 / (1.0 + 1e-6 / total)), rel=1e-15)
    assert out['overall']['mBLeu_1'] < 1e-10 and out['overall']['gDiv1'] == float(total.sum())


def test_all_empty_captions_score_zero_not_nan():
    out = D.evaluate(REFS, [[[0] * 8] * 3, [[1, 2, 3, 4, 0, 0, 0, 0], [0] * 8, [5, 6, 0, 0, 0, 0, 0, 0]]], oracle=True)
    assert out['self_cider'][0] == 0.0 and np.isfinite(out['self_cider']).all()
    assert all(np.isfinite(v) for v in out['overall'].values())
    assert out['overall']['oracle_CIDEr'] >= out['overall']['avg_CIDEr']


def test_ctypes_struct_matches_the_header():
    """field order of _lib.DivEval == capmi_diveval in include/capmi.h (tests/test_abi.py covers the two entry points)"""
    ctypes = pytest.importorskip('ctypes')
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'capmi.h')).read(), flags=re.S)
    body = re.search(r'typedef struct capmi_diveval \{([^{}]*?)\} capmi_diveval;', src, flags=re.S).group(1)
    names = [re.findall(r'(\w+)\s*$', part.strip())[0] for stmt in body.split(';') if stmt.strip() for part in stmt.split(',')]
    from imagecaptioning.pytorch_amd import _lib
    assert names == [f[0] for f in _lib.DivEval._fields_]
    assert _lib.DivEval.lang.size == ctypes.sizeof(_lib.LangEval)
    consts = dict(re.findall(r'#define CAPMI_DIVEVAL_(\w+) (\d+)', src))
    assert (int(consts['NMAX']), int(consts['NOUT']), int(consts['VOCAB_WORDS'])) == (_lib.DIVEVAL_NMAX, _lib.DIVEVAL_NOUT,
                                                                                      _lib.DIVEVAL_VOCAB_WORDS)


def test_eval_oracle_option_parses():
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    assert opts.parse_opt(['--eval_oracle', '0']).eval_oracle == 0
    assert opts.parse_opt(['--eval_oracle', '1', '--sample_n', '5', '--sample_n_method', 'dbs']).eval_oracle == 1
    from imagecaptioning.pytorch_amd.tools import eval_ensemble
    assert 'eval_oracle' in eval_ensemble.EVAL_KEYS


@pytest.mark.parametrize('oracle', [False, True])
def test_n_json_assembly(oracle):
    """tools/eval.assemble_n on a stubbed DiversityEval.compute(): the reference's layout of <id>_<split>_n.json"""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    from imagecaptioning.pytorch_amd.diveval import DIV_KEYS, ORACLE_KEYS
    rng = np.random.default_rng(3)
    m, n = 4, 3
    overall = {k: float(rng.random()) for k in DIV_KEYS + ('self_cider',)}
    per_image = {'individual_mBleu_2': rng.random((m, n)), 'self_cider': rng.random(m), 'self_cider_mat': rng.random((m, n, n))}
    per_image['mBleu_2'] = per_image['individual_mBleu_2'].mean(axis=1)
    if oracle:
        per_image['scores'] = rng.random((m, n, 6))
        for x, k in enumerate(ORACLE_KEYS):
            per_image['oracle_' + k], per_image['avg_' + k] = per_image['scores'][:, :, x].max(1), per_image['scores'][:, :, x].mean(1)
            overall['oracle_' + k], overall['avg_' + k] = float(per_image['oracle_' + k][[2, 0]].mean()), 0.5
    # two of the four images were evaluated, in another order than the split's
    groups = [(id_, [{'image_id': id_, 'caption': 'c%d' % j, 'perplexity': float(j)} for j in range(n)]) for id_ in ('b', 'a')]
    out = json.loads(json.dumps(E.assemble_n(overall, per_image, groups, {'a': 0, 'b': 2}, oracle)))
    assert set(out) == ({'div_stats', 'self_cider', 'oracle'} if oracle else {'div_stats', 'self_cider'})
    assert set(out['div_stats']) == {'overall', 'ImgToEval'} and set(out['self_cider']) == {'overall', 'imgToEval'}
    assert out['div_stats']['overall'] == {k: overall[k] for k in DIV_KEYS}
    assert out['self_cider']['overall'] == {'self_cider': overall['self_cider']}
    for id_, pos in (('a', 0), ('b', 2)):
        e = out['div_stats']['ImgToEval'][id_]
        assert e['mBleu_2'] == per_image['mBleu_2'][pos]
        assert [p['caption'] for p in e['individuals']] == ['c0', 'c1', 'c2']
        assert [p['mBleu_2'] for p in e['individuals']] == per_image['individual_mBleu_2'][pos].tolist()
        s = out['self_cider']['imgToEval'][id_]
        assert s['self_cider'] == per_image['self_cider'][pos] and s['self_cider_mat'] == per_image['self_cider_mat'][pos].tolist()
        if oracle:
            o = out['oracle']['ImgToEval'][id_]
            assert o['oracle_CIDEr'] == per_image['oracle_CIDEr'][pos] and o['avg_ROUGE_L'] == per_image['avg_ROUGE_L'][pos]
            assert [p['caption'] for p in o['captions']] == ['c0', 'c1', 'c2']
            assert o['captions'][1]['scores']['Bleu_3'] == per_image['scores'][pos, 1, 3]
    if oracle:
        assert set(out['oracle']['overall']) == {p + k for k in ORACLE_KEYS for p in ('oracle_', 'avg_')}
        assert np.mean([v['oracle_CIDEr'] for v in out['oracle']['ImgToEval'].values()]) == pytest.approx(
            out['oracle']['overall']['oracle_CIDEr'], rel=1e-12)
    # the groups' dicts are the prediction dicts themselves: sorting model.n_predictions later keeps the values attached
    assert all('mBleu_2' in p for _, caps in groups for p in caps)
