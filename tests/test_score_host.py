"""Scoring given captions (mode='score', imagecaptioning/pytorch_amd/score.py, csrc/score.hip, tools/eval.py --self_retrieval /
--score_json) without a GPU: the refusals, the shape rules of the two pairings, the tiling plan and the driver on a fake decoder
that counts its calls (capmi_score_step replaced by its float64 restatement tests/score_ref64.py), the host summary, the word
lookup, the bindings and the command line."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import score_ref64 as R
from test_att_trace_host import tiny_opt

FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')
ENTRIES = {'capmi_score_step': 12, 'capmi_retrieval_rank': 8}


def _model(name):
    from imagecaptioning.pytorch_amd.captioning import models
    if name == 'ensemble':
        return models.AttEnsemble([models.setup(tiny_opt('updown')), models.setup(tiny_opt('att2in2'))])
    return models.setup(tiny_opt(name))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals and shapes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FAMILIES + ('ensemble',))
def test_refusals_come_before_device_work(name):
    from imagecaptioning.pytorch_amd._lib import CapmiError
    model = _model(name).eval()
    assert model.last_score is None
    fc, att = torch.zeros(2, 20), torch.zeros(2, 4, 20)
    seqs = torch.tensor([[[3, 4, 0, 0, 0, 0]], [[5, 0, 0, 0, 0, 0]]])

    def call(s=seqs, **opt):
        return model(fc, att, s, None, mode='score', opt=opt)

    if name == 'ensemble':
        with pytest.raises(NotImplementedError, match='AttEnsemble.*one by one'):
            call()
        return
    with pytest.raises(NotImplementedError, match='output_logsoftmax'):
        call(output_logsoftmax=0)
    model.train()
    with pytest.raises(NotImplementedError, match=r'model\.eval\(\)'):
        call()
    model.eval()
    with pytest.raises(ValueError, match='score_norm'):
        call(score_norm='mean')
    with pytest.raises(ValueError, match='pairing'):
        call(pairing='all')
    with pytest.raises(ValueError, match='temperature'):
        call(temperature=0)
    with pytest.raises(ValueError, match='score_rows'):
        call(score_rows=0)
    with pytest.raises(ValueError, match=r'\[B, n, L\]'):
        call(seqs[:1])
    with pytest.raises(ValueError, match='image-major'):
        call(torch.zeros(3, 6, dtype=torch.long))
    with pytest.raises(ValueError, match='seq_length'):
        call(torch.zeros(2, 1, 7, dtype=torch.long))
    with pytest.raises(ValueError, match='integer'):
        call(torch.zeros(2, 1, 6))
    with pytest.raises(ValueError, match='cross'):
        call(pairing='cross')                                                # [B, n, L] is no list of captions
    # valid calls go on to the device check of a CPU tensor, which is no refusal of the option
    for s, opt in ((seqs, {}), (seqs.reshape(2, 6), dict(score_norm='length', temperature=2.0, suppress_UNK=1)),
                   (seqs.reshape(2, 6), dict(pairing='cross', score_rows=1)), (torch.zeros(4, 3, dtype=torch.long), {})):
        with pytest.raises(CapmiError, match='HIP device'):
            call(s, **opt)
    assert model.last_score is None


def test_models_without_a_stepper_refuse():
    from imagecaptioning.pytorch_amd.captioning.models.CaptionModel import CaptionModel
    from imagecaptioning.pytorch_amd import score

    class Bare(CaptionModel):
        pass
    with pytest.raises(NotImplementedError, match='single-step decoder'):
        score.check_options(Bare().eval(), {})
    assert score.check_options(_model('updown').eval(), None) == ('aligned', 'none', None)


def test_shape_rules():
    from imagecaptioning.pytorch_amd import score
    z = lambda *s: torch.zeros(*s, dtype=torch.long)                         # noqa: E731
    n, s = score.shape_of(z(3, 2, 6), 3, 6, 'aligned')
    assert n == 2 and s.shape == (3, 2, 6)
    n, s = score.shape_of(z(6, 4), 3, 6, 'aligned')                          # image-major rows, a shorter L
    assert n == 2 and s.shape == (3, 2, 4)
    n, s = score.shape_of(z(5, 6), 3, 6, 'cross')                            # C need not be a multiple of B
    assert n == 5 and s.shape == (5, 6)
    assert score.lengths(torch.tensor([[3, 4, 0, 5], [0, 1, 1, 1], [1, 2, 3, 4]])).tolist() == [2, 0, 4]
    assert score.default_rows(9488) * 9488 * 4 <= 512 << 20 < (score.default_rows(9488) + 1) * 9488 * 4
    assert score.default_rows(9488, 1000) == 2796 and score.default_rows(41, 32) * 41 * 4 <= 512 << 20


# ---------------------------------------------------------------------------------------------------------------------------
# the tiling plan and the driver on a fake decoder
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,n,rows', [(1, 1, 1), (3, 4, 1), (3, 4, 2), (3, 4, 5), (3, 4, 12), (3, 4, 100), (7, 3, 8), (2, 9, 4),
                                      (10, 10, 7)])
def test_plan_covers_every_pair_once_within_the_row_limit(B, n, rows):
    from imagecaptioning.pytorch_amd import score
    seen = np.zeros((B, n), int)
    tiles = score.plan(B, n, rows)
    for (i0, i1), caps in tiles:
        assert 0 <= i0 < i1 <= B
        for c0, c1 in caps:
            assert 0 <= c0 < c1 <= n and (i1 - i0) * (c1 - c0) <= rows
            seen[i0:i1, c0:c1] += 1
    assert (seen == 1).all()
    assert [t[0] for t in tiles] == sorted(set(t[0] for t in tiles))         # every image tile appears once: one prefill each
    if rows >= B * n:
        assert len(tiles) == 1 and len(tiles[0][1]) == 1


V1, L = 7, 5


def _table(image, prefix):
    """the logits of one (image, fed prefix): any deterministic function of both"""
    rng = np.random.default_rng(1000 * image + sum((k + 1) * 31 ** i for i, k in enumerate(prefix)) % 99991)
    return rng.normal(size=V1) * 2.0


class FakeDecoder:
    """step.py protocol over _table; counts what the driver does"""

    def __init__(self, images, rows_per_image, log):
        self.images, self.cap, self.log = images, rows_per_image, log
        self.prefix = None

    def step(self, t, it, rows_per_image):
        it = it.tolist()
        if t == 0:
            assert rows_per_image == 1 and it == [0] * len(self.images)
            self.prefix = [[(i, ())] for i in self.images]
            pre = [p[0] for p in self.prefix]
        else:
            assert rows_per_image == self.cap and len(it) == len(self.images) * self.cap
            flat = [p for img in self.prefix for p in img]
            assert len(flat) == len(it)
            flat = [(i, p + (v,)) for (i, p), v in zip(flat, it)]
            self.prefix = [flat[k * self.cap:(k + 1) * self.cap] for k in range(len(self.images))]
            pre = flat
        self.log['step_rows'].append(len(pre))
        return torch.from_numpy(np.stack([_table(i, p) for i, p in pre]).astype(np.float32))

    def reorder(self, parent, cur):
        assert cur == 1 and parent.shape == (len(self.images), self.cap) and not parent.any()
        self.prefix = [[img[0]] * self.cap for img in self.prefix]
        self.log['reorders'] += 1


def _fake_score_step(logits, tok, live, acc, cnt, tok_logp=None, inv_temperature=1.0, unk_col=-1):
    lp, live2, acc2, cnt2 = R.score_step(logits.numpy(), tok.numpy(), live.numpy().astype(bool), acc.numpy(), cnt.numpy(),
                                         inv_temperature, unk_col)
    was = live.numpy().astype(bool)
    if tok_logp is not None:
        tok_logp[torch.from_numpy(was)] = torch.from_numpy(lp[was]).float()
    acc.copy_(torch.from_numpy(acc2).float())
    cnt.copy_(torch.from_numpy(cnt2).int())
    live.copy_(torch.from_numpy(live2.astype(np.uint8)))


def _direct(image, seq, inv_t=1.0):
    rows, prefix = [], ()
    for v in seq:
        rows.append(_table(image, prefix))
        prefix += (int(v),)
    return R.score_caption(np.stack(rows), seq, inv_t)


@pytest.mark.parametrize('pairing', ('aligned', 'cross'))
@pytest.mark.parametrize('score_rows', (None, 1, 2, 3, 5, 8))
def test_driver_on_a_counting_decoder(monkeypatch, pairing, score_rows):
    from imagecaptioning.pytorch_amd import score
    monkeypatch.setattr(score.ops, 'score_step', _fake_score_step)
    B, n = 3, 4
    rng = np.random.default_rng(5)
    caps = rng.integers(1, V1, size=(B, n, L))
    for b in range(B):
        for j in range(n):
            caps[b, j, int(rng.integers(0, L + 1)):] = 0                    # lengths 0 .. L; 0: an empty caption, L: no end token
    caps[0, 0], caps[1, 1] = 0, rng.integers(1, V1, size=L)
    seqs = torch.from_numpy(caps) if pairing == 'aligned' else torch.from_numpy(caps[0])
    log = {'prepares': [], 'makes': 0, 'step_rows': [], 'reorders': 0}

    def prepare(i0, i1):
        log['prepares'].append((i0, i1))

        def make(rows_per_image):
            log['makes'] += 1
            return FakeDecoder(list(range(i0, i1)), rows_per_image, log)
        return make

    out = score.run(prepare, B, V1, seqs, pairing, 'cpu', score_rows, inv_temperature=0.5)
    limit = score_rows or score.default_rows(V1)
    tiles = score.plan(B, n, limit)
    assert log['prepares'] == [t[0] for t in tiles]                          # one prefill per image tile, images outside
    assert log['makes'] == sum(len(t[1]) for t in tiles) and max(log['step_rows']) <= limit
    for b in range(B):
        for j in range(n):
            seq = caps[b, j] if pairing == 'aligned' else caps[0, j]
            want, ln, tl = _direct(b, seq, 0.5)
            at = (b, j) if pairing == 'aligned' else (j, b)
            assert abs(float(out['logp'][at]) - want) < 1e-4 and int(out['len'][at]) == ln == min(L, int((seq != 0).cumprod().sum()) + 1)
            np.testing.assert_allclose(out['tok_logp'][at].numpy(), tl, atol=1e-4)
    if pairing == 'cross':
        assert out['logp'].shape == (n, B)
        assert score.run(prepare, B, V1, seqs, pairing, 'cpu', score_rows, keep_tok=False)['tok_logp'] is None
    with pytest.raises(ValueError, match=r'\[0, 7\)'):
        score.run(prepare, B, V1, seqs.clone().fill_(V1), pairing, 'cpu', score_rows)


# ---------------------------------------------------------------------------------------------------------------------------
# host arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def test_retrieval_summary_on_hand_made_ranks():
    from imagecaptioning.pytorch_amd import score
    s = score.retrieval_summary([1], pool_size=1, pools=1)                   # a pool of one image
    assert (s['R@1'], s['R@5'], s['R@10'], s['median_rank'], s['mean_rank'], s['MRR']) == (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    assert (s['pool_size'], s['pools'], s['captions']) == (1, 1, 1)
    s = score.retrieval_summary([3, 1, 12, 6])
    assert (s['R@1'], s['R@5'], s['R@10']) == (0.25, 0.5, 0.75) and s['median_rank'] == 4.5 and s['mean_rank'] == 5.5
    assert abs(s['MRR'] - (1 + 1 / 3 + 1 / 6 + 1 / 12) / 4) < 1e-15
    s = score.retrieval_summary([5, 5, 10, 11, 2])
    assert (s['R@1'], s['R@5'], s['R@10'], s['median_rank']) == (0.0, 0.6, 0.8, 5.0)
    for ranks in ([1], [3, 1, 12, 6], [5, 5, 10, 11, 2], list(range(1, 40))):
        want = R.summary(ranks)
        got = score.retrieval_summary(ranks)
        assert all(abs(got[k] - want[k]) < 1e-12 for k in want)
    with pytest.raises(ValueError):
        score.retrieval_summary([])
    with pytest.raises(ValueError):
        score.retrieval_summary([0, 1])


def test_reference_ranks_and_ties():
    S = np.array([[2., 5., 5., 1.], [3., 3., 3., 3.], [0., 1., 2., 3.]])
    assert R.retrieval(S, [2, 0, 0])[0].tolist() == [2, 1, 4] and R.retrieval(S, [1, 3, 3])[0].tolist() == [1, 4, 1]
    np.testing.assert_allclose(R.retrieval(S, [0, 1, 2])[1][1], -np.log(4))
    lp, live, acc, cnt = R.score_step(np.log([[0.5, 0.25, 0.25]] * 3), [1, 0, 2], [True, True, False], [1.0, 2.0, 3.0], [4, 5, 6])
    np.testing.assert_allclose(lp[:2], np.log([0.25, 0.5]))
    assert np.isnan(lp[2]) and live.tolist() == [True, False, False] and cnt.tolist() == [5, 6, 6] and acc[2] == 3.0
    total, n, tl = R.score_caption(np.log([[0.5, 0.25, 0.25]] * 4), [1, 2, 0, 0])
    assert n == 3 and abs(total - np.log(0.25 * 0.25 * 0.5)) < 1e-12 and tl[3] == 0


def test_word_lookup():
    from imagecaptioning.pytorch_amd import score
    vocab = {'1': 'a', '2': 'cat', '3': 'sits', '4': 'UNK'}
    rows, miss = score.encode_captions(['a cat sits', 'a okapi sits', ''], vocab, 4)
    assert rows.tolist() == [[1, 2, 3, 0], [1, 4, 3, 0], [0, 0, 0, 0]] and miss == [0, 1, 0]
    rows, miss = score.encode_captions(['a okapi sits', ['cat', 'zebra', 'gnu']], vocab, 4, oov='drop')
    assert rows.tolist() == [[1, 3, 0, 0], [2, 0, 0, 0]] and miss == [1, 2]
    rows, _ = score.encode_captions(['a cat sits a cat sits'], vocab, 4)     # cut at L words
    assert rows.tolist() == [[1, 2, 3, 1]]
    with pytest.raises(ValueError, match='okapi'):
        score.encode_captions(['a okapi'], {'1': 'a'}, 4)
    with pytest.raises(ValueError):
        score.encode_captions(['a'], vocab, 4, oov='error')


# ---------------------------------------------------------------------------------------------------------------------------
# bindings and command line
# ---------------------------------------------------------------------------------------------------------------------------
def test_new_entries_in_header_match_the_binding():
    from imagecaptioning.pytorch_amd import _lib, ops
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'capmi.h')).read(), flags=re.S)
    decl = dict((m.group(1), m.group(2).strip()) for m in
                re.finditer(r'\b(?:int|int64_t|const char \*)\s*(capmi_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    for name, nargs in ENTRIES.items():
        assert len(decl[name].split(',')) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib, name)
    kinds = {'float': _lib.C.c_float, 'int': _lib.C.c_int, 'int64_t': _lib.C.c_int64}
    for name in ENTRIES:                                                     # argument by argument: pointer, or the scalar type
        for arg, ctype in zip(decl[name].split(','), _lib.SIGNATURES[name]):
            want = _lib.C.c_void_p if '*' in arg else kinds[arg.split()[-2]]
            assert ctype is want, (name, arg)
    # the argument checks come before any launch
    one = _lib.C.c_void_p(16)
    step = _lib.lib.capmi_score_step
    assert step(None, 4, 1, 4, None, None, None, None, None, 1.0, -1, None) == _lib.EINVAL
    for ld, rows, V1, inv_t in ((4, 0, 4, 1.0), (4, 1, 0, 1.0), (3, 1, 4, 1.0), (4, 1, 4, 0.0), (4, 1, 4, -1.0),
                                (4, 1, 4, float('nan')), (4, 1, 4, float('inf'))):
        assert step(one, ld, rows, V1, one, one, one, one, None, inv_t, -1, None) == _lib.EINVAL
    rank = _lib.lib.capmi_retrieval_rank
    assert rank(None, 4, 1, 4, None, None, None, None) == _lib.EINVAL
    for ld, C, I in ((4, 0, 4), (4, 1, 0), (3, 1, 4)):
        assert rank(one, ld, C, I, one, one, None, None) == _lib.EINVAL
    with pytest.raises(_lib.CapmiError):
        ops.score_step(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.uint8), torch.zeros(2),
                       torch.zeros(2, dtype=torch.int32))                    # CPU tensors
    with pytest.raises(_lib.CapmiError):
        ops.retrieval_rank(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long))


def test_command_line(tmp_path):
    import argparse
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd'))
    from captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import eval as E
    d = opts.DEFAULTS
    assert (d['self_retrieval'], d['retrieval_pool'], d['score_norm'], d['score_json']) == (0, 1000, 'none', '')
    o = opts.parse_opt(['--self_retrieval', '1', '--retrieval_pool', '4', '--score_norm', 'length', '--score_json', 's.json'])
    assert (o.self_retrieval, o.retrieval_pool, o.score_norm, o.score_json) == (1, 4, 'length', 's.json')
    off = opts.parse_opt([])
    assert E.SelfRetrieval.load(off, None, {}) is None and E.CaptionScores.load(off, {}, 6) is None
    assert not {'self_retrieval', 'score_norm', 'score_json'} & set(E.eval_kwargs_of(o))
    assert E.SelfRetrieval.load(o, None, {}).pool == 4
    with pytest.raises(NotImplementedError, match='constraints_json'):
        E.SelfRetrieval.load(o, object(), {})
    o.sample_n = 3
    with pytest.raises(NotImplementedError, match='rerank'):
        E.SelfRetrieval.load(o, None, {})
    assert E.SelfRetrieval.load(o, None, {'rerank': 'mbr_bleu4'}).norm == 'length'
    with pytest.raises(ValueError, match='retrieval_pool'):
        E.SelfRetrieval(0)
    with pytest.raises(ValueError, match='score_norm'):
        E.SelfRetrieval(4, 'mean')
    vocab = {'1': 'a', '2': 'cat', '3': 'UNK'}
    path = tmp_path / 's.json'
    path.write_text(json.dumps({'7': ['a cat', 'a dog'], '9': 'cat', '11': []}))
    ns = argparse.Namespace(score_json=str(path), constraints_oov='error', score_norm='none', eval_results_dir=str(tmp_path), id='x')
    cs = E.CaptionScores.load(ns, vocab, 3)
    assert sorted(cs.by_id) == ['7', '9'] and cs.by_id['7'][1].tolist() == [[1, 2, 0], [1, 3, 0]] and cs.by_id['7'][2] == [0, 1]
    ns.constraints_oov = 'drop'
    assert E.CaptionScores.load(ns, vocab, 3).by_id['7'][1].tolist() == [[1, 2, 0], [1, 0, 0]]
    assert cs.missing_ids() == ['7', '9']                                    # nothing met yet: both are reported
    written = json.load(open(cs.write(ns, 'val')))
    assert written['missing_image_ids'] == ['7', '9'] and written['images'] == {} and os.path.basename(cs.write(ns, 'val')) == 'x_val_scores.json'
