"""Scoring given captions on the device (csrc/score.hip, imagecaptioning/pytorch_amd/score.py, mode='score', tools/eval.py
--self_retrieval / --score_json) against the float64 restatements tests/score_ref64.py and against the decode paths the suite
already trusts.

Tolerances, all taken from existing tests:
* kernel outputs against float64: rtol = atol = 1e-4, what tests/test_beam_gpu.py (lines 174-181, 216-224) allows the
  capmi_beam_logsoftmax rows of a search against the float64 golden values (test_sbs_gpu.py bounds the same rows plus one add by 1e-4);
* a family's stepper against its one-call greedy rollout: 1e-4 absolute for the LSTM families (test_att2in2_gpu.py /
  test_adaatt_gpu.py test_one_call_greedy_equals_stepper_greedy), 2e-3 for transformer / aoa, whose KV-cached decode
  test_model_api_gpu.py::test_baseline_size_xe_step_and_incremental_decode_consistency compares with that bound.
With untrained weights the scores of one caption across images are nearly equal, so no test compares end-to-end RANKS with a float64
replay of a model; score matrices are compared by tolerance and the rank logic on exact integer matrices."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import score_ref64 as R
from shapes import ragged_masks
from test_att_trace_host import tiny_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'imagecaptioning', 'pytorch_amd')
FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')
RTOL = ATOL = 1e-4
STEPPER_TOL = {name: 1e-4 for name in FAMILIES[:5]}
STEPPER_TOL.update(transformer=2e-3, aoa=2e-3)
ACC0, CNT0, TL0 = 123.25, -7, 9.5                # sentinels of rows that must stay untouched


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _strided(x, ld):
    """x [rows, V1] float32 on the device with `ld` floats between rows (ld > V1: row bases lose their 16-byte alignment)"""
    rows, V1 = x.shape
    buf = torch.full((rows, ld), 7777.0, dtype=torch.float32, device=DEV)
    buf[:, :V1] = _dev(x)
    return buf[:, :V1]


# ---------------------------------------------------------------------------------------------------------------------------
# capmi_score_step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V1', (3, 5, 67, 1024, 1025, 9488))    # 1024 / 1025: the last wave-per-row and the first workgroup-per-row width
def test_score_step_against_float64(V1):
    from imagecaptioning.pytorch_amd import ops
    worst = 0.0
    for rows in (1, 3, 130):
        for pad in (0, 3):
            for inv_t in (1.0, 2.0):
                rng = np.random.default_rng(17 * V1 + 3 * rows + pad + int(10 * inv_t))
                x = rng.uniform(-80, 80, size=(rows, V1)).astype(np.float32)
                x[:, 1] = -1000.0                                            # a column far below: it must vanish, not overflow
                unk = V1 - 1
                tok = rng.integers(0, V1, size=rows)
                tok[rng.random(rows) < 0.3] = 0                              # scored once, then dead
                tok[rng.random(rows) < 0.2] = unk                            # the suppressed column itself
                tok[rng.random(rows) < 0.1] = 1
                live0 = rng.random(rows) < 0.7                               # the others are dead on entry
                if rows > 1:
                    tok[0], live0[0], live0[1] = 0, True, False
                logits = _strided(x, V1 + pad)
                for with_tl in (True, False):
                    live = _dev(live0.astype(np.uint8))
                    acc = torch.full((rows,), ACC0, device=DEV)
                    cnt = torch.full((rows,), CNT0, dtype=torch.int32, device=DEV)
                    tl = torch.full((rows,), TL0, device=DEV) if with_tl else None
                    state = (live, acc, cnt, tl)
                    tokd = _dev(tok)
                    ops.score_step(logits, tokd, *state, inv_temperature=inv_t, unk_col=unk)
                    lp, live1, acc1, cnt1 = R.score_step(x, tok, live0, np.full(rows, ACC0), np.full(rows, CNT0), inv_t, unk)
                    what = (V1, rows, pad, inv_t, with_tl)
                    assert np.array_equal(live.cpu().numpy().astype(bool), live1), what
                    assert np.array_equal(cnt.cpu().numpy(), cnt1), what
                    got = acc.cpu().numpy()
                    np.testing.assert_allclose(got[live0], acc1[live0], rtol=RTOL, atol=ATOL, err_msg=str(what))
                    assert got[~live0].tobytes() == np.full(int((~live0).sum()), ACC0, np.float32).tobytes(), what
                    if with_tl:
                        g = tl.cpu().numpy()
                        np.testing.assert_allclose(g[live0], lp[live0], rtol=RTOL, atol=ATOL, err_msg=str(what))
                        assert g[~live0].tobytes() == np.full(int((~live0).sum()), TL0, np.float32).tobytes(), what
                        if live0.any():
                            worst = max(worst, float(np.abs(g[live0] - lp[live0]).max()))
                        assert (g[live0 & (tok == unk)] < -999).all()
                    # the same input again: the same bits
                    again = (_dev(live0.astype(np.uint8)), torch.full((rows,), ACC0, device=DEV),
                             torch.full((rows,), CNT0, dtype=torch.int32, device=DEV), torch.full((rows,), TL0, device=DEV) if with_tl else None)
                    ops.score_step(logits, tokd, *again, inv_temperature=inv_t, unk_col=unk)
                    assert all(torch.equal(a, b) for a, b in zip(state, again) if a is not None), what
                    # a second step: the rows that ended (and those dead on entry) keep their bits exactly
                    before = [t.clone() for t in state if t is not None]
                    tok2 = _dev(rng.integers(1, V1, size=rows))
                    ops.score_step(logits, tok2, *state, inv_temperature=inv_t, unk_col=-1)
                    dead = torch.from_numpy(~live1).to(DEV)
                    for a, b in zip(before, [t for t in state if t is not None]):
                        assert torch.equal(a[dead], b[dead]), what
                    assert np.array_equal(cnt.cpu().numpy()[live1], cnt1[live1] + 1), what
    print('score_step V1=%d: worst |tok_logp - float64| %.3g' % (V1, worst))


def test_score_step_refuses_bad_arguments_without_writing():
    from imagecaptioning.pytorch_amd import _lib, ops
    rows, V1 = 3, 9
    logits = torch.zeros(rows, V1, device=DEV)
    tok = torch.ones(rows, dtype=torch.long, device=DEV)
    live = torch.ones(rows, dtype=torch.uint8, device=DEV)
    acc = torch.full((rows,), ACC0, device=DEV)
    cnt = torch.full((rows,), CNT0, dtype=torch.int32, device=DEV)
    tl = torch.full((rows,), TL0, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()
    good = [p(logits), V1, rows, V1, p(tok), p(live), p(acc), p(cnt), p(tl), 1.0, -1, st]
    bad = []
    for i in (0, 4, 5, 6, 7):                                                # a null pointer (tok_logp may be one)
        bad.append([None if k == i else v for k, v in enumerate(good)])
    for i, v in ((2, 0), (2, -1), (3, 0), (1, V1 - 1), (9, 0.0), (9, -2.0), (9, float('nan'))):
        bad.append([v if k == i else g for k, g in enumerate(good)])
    for args in bad:
        assert _lib.lib.capmi_score_step(*args) == _lib.EINVAL, args
    torch.cuda.synchronize()
    assert (live == 1).all() and (acc == ACC0).all() and (cnt == CNT0).all() and (tl == TL0).all()
    for wrong in (dict(tok=tok.int()), dict(live=live.bool()), dict(acc=acc[:2]), dict(cnt=cnt.long()), dict(logits=logits.t())):
        kw = dict(logits=logits, tok=tok, live=live, acc=acc, cnt=cnt)
        kw.update(wrong)
        with pytest.raises(_lib.CapmiError):
            ops.score_step(**kw)
    assert (acc == ACC0).all() and (cnt == CNT0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# capmi_retrieval_rank
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('I', (1, 2, 37, 1000))
def test_retrieval_rank_against_float64(I):
    from imagecaptioning.pytorch_amd import _lib, ops
    for C in (1, 5, 64):
        rng = np.random.default_rng(100 * I + C)
        S = rng.integers(-2, 3, size=(C, I)).astype(np.float32)              # small integers: ties are real ties
        target = np.zeros(C, np.int64)
        for c in range(C):
            kind = c % 3
            if kind == 1:
                target[c] = I - 1
            elif kind == 2 and I >= 3:
                mid = I // 2
                S[c, mid - 1:mid + 2] = S[c, mid]                            # the target sits in the middle of a run of ties
                target[c] = mid
        Sd = _strided(S, I + 5)
        rank, post = ops.retrieval_rank(Sd, torch.from_numpy(target))
        want_rank, want_post = R.retrieval(S, target)
        assert rank.dtype == torch.int32 and np.array_equal(rank.cpu().numpy(), want_rank), (I, C)
        np.testing.assert_allclose(post.cpu().numpy(), want_post, rtol=RTOL, atol=ATOL)
        rank2, none = ops.retrieval_rank(Sd, _dev(target), log_post=False)
        assert none is None and torch.equal(rank, rank2)
        with pytest.raises(_lib.CapmiError):
            ops.retrieval_rank(Sd, torch.full((C,), I, dtype=torch.long))
    S = _dev(np.zeros((2, 3), np.float32))
    out = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    t = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    for args in ((None, 3, 2, 3, p(t), p(out), None, None), (p(S), 3, 2, 3, None, p(out), None, None), (p(S), 3, 2, 3, p(t), None, None, None),
                 (p(S), 3, 0, 3, p(t), p(out), None, None), (p(S), 3, 2, 0, p(t), p(out), None, None), (p(S), 2, 2, 3, p(t), p(out), None, None)):
        assert _lib.lib.capmi_retrieval_rank(*args) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (out == -5).all()


# ---------------------------------------------------------------------------------------------------------------------------
# every family through mode='score'
# ---------------------------------------------------------------------------------------------------------------------------
B_, L_, VOC, K_ = 3, 6, 40, 5
_models, _shared = {}, {}


def _family(name):
    from imagecaptioning.pytorch_amd.captioning import models
    if name not in _models:
        torch.manual_seed(31 + FAMILIES.index(name))
        vocab = {str(i): 'w%d' % i for i in range(1, VOC)}
        vocab[str(VOC)] = 'UNK'
        opt = tiny_opt(name, vocab_size=VOC, rnn_size=32, input_encoding_size=32, att_hid_size=32, d_model=32, d_ff=64, seq_length=L_,
                       max_length=L_, vocab=vocab)
        _models[name] = models.setup(opt).to(DEV).eval()
    return _models[name]


def _feats():
    gen = torch.Generator().manual_seed(5)
    return (torch.randn(B_, 20, generator=gen).to(DEV), torch.randn(B_, K_, 20, generator=gen).to(DEV),
            ragged_masks(B_, K=K_, lo=2).to(DEV))


def _greedy(name):
    """the family's greedy decode, computed once and left unchanged: (seq [B, L], seqLogprobs [B, L, V1])"""
    if name not in _shared:
        fc, att, masks = _feats()
        with torch.no_grad():
            seq, logp = _family(name)(fc, att, masks, opt=dict(sample_method='greedy', beam_size=1), mode='sample')
        _shared[name] = (seq.clone(), logp.clone())
    return _shared[name]


def _score(name, seqs, **opt):
    fc, att, masks = _feats()
    model = _family(name)
    out = model(fc, att, seqs, masks, mode='score', opt=opt)
    return out, model.last_score


@pytest.mark.parametrize('name', FAMILIES)
def test_aligned_scores_are_the_greedy_decodes_own_log_probs(name):
    seq, logp = _greedy(name)
    tol = STEPPER_TOL[name]
    out, last = _score(name, seq.unsqueeze(1))
    assert out.shape == (B_, 1) and sorted(last) == ['len', 'logp', 'perplexity', 'tok_logp']
    assert last['tok_logp'].shape == (B_, 1, L_) and all(v.is_cuda for v in last.values()) and torch.equal(out, last['logp'])
    live = torch.cat([seq.new_ones(B_, 1), (seq[:, :-1] > 0).long()], 1).cumprod(1).bool()     # up to and including the end token
    want = logp.gather(2, seq.unsqueeze(2)).squeeze(2)
    got = last['tok_logp'][:, 0]
    err = float(((got - want).abs() * live).max())
    print('%s: max |tok_logp - seqLogprobs| = %.3g (bound %g)' % (name, err, tol))
    assert err <= tol
    assert (got[~live] == 0).all() and last['len'][:, 0].tolist() == live.sum(1).tolist()
    assert float((last['logp'][:, 0] - (want * live).sum(1)).abs().max()) <= tol * L_
    # the flat, image-major form and the norms
    out2, last2 = _score(name, seq, score_norm='length')
    assert torch.equal(last2['logp'], last['logp']) and torch.equal(out2, last['logp'] / last['len'].float())
    assert torch.equal(last['perplexity'], torch.exp(-last['logp'] / last['len'].float()))


@pytest.mark.parametrize('name', FAMILIES)
def test_cross_scores_equal_aligned_scores_and_do_not_depend_on_the_tiling(name):
    seq, _ = _greedy(name)
    tol = STEPPER_TOL[name]
    caps = torch.cat([seq, torch.tensor([[5, 6, 7, 8, 9, 10]], device=DEV)])                  # C = 4; the last one has no end token
    aligned, _ = _score(name, caps.unsqueeze(0).expand(B_, 4, L_).contiguous())
    S, last = _score(name, caps, pairing='cross')
    assert S.shape == (4, B_) and last['tok_logp'] is None and last['len'].shape == (4, B_)
    assert last['len'][3].tolist() == [L_] * B_
    err = float((S - aligned.t()).abs().max())
    hook = {}
    St, last_t = _score(name, caps, pairing='cross', score_rows=2, score_tok_logp=1, _score_hook=hook)
    tiles = sorted({(h[0], h[1]) for h in hook['logits']})
    assert tiles == [((b, b + 1), (c, c + 2)) for b in range(B_) for c in (0, 2)]               # 1 image x 2 captions
    assert all(h[3].shape[0] <= 2 for h in hook['logits'])
    err_t = float((St - S).abs().max())
    print('%s: max |cross - aligned| = %.3g, |tiled - untiled| = %.3g (bound %g)' % (name, err, err_t, tol * L_))
    assert err <= tol * L_ and err_t <= tol * L_                             # a sum of up to L token log-probs, each within tol
    assert last_t['tok_logp'].shape == (4, B_, L_)
    assert float((last_t['tok_logp'].sum(2) - St).abs().max()) <= 1e-4
    _, a_last = _score(name, caps.unsqueeze(0).expand(B_, 4, L_).contiguous())
    assert float((last_t['tok_logp'] - a_last['tok_logp'].transpose(0, 1)).abs().max()) <= tol


@pytest.mark.parametrize('name', FAMILIES)
def test_temperature_agrees_with_the_float64_step_on_the_recorded_logits(name):
    seq, _ = _greedy(name)
    plain, _ = _score(name, seq.unsqueeze(1))
    hook = {}
    out, last = _score(name, seq.unsqueeze(1), temperature=2.0, _score_hook=hook)
    assert float((out - plain).abs().max()) > 1e-3                           # it changes the scores
    toks = seq.cpu().numpy()
    live, acc, cnt = np.ones(B_, bool), np.zeros(B_), np.zeros(B_, int)
    assert [h[2] for h in hook['logits']] == list(range(len(hook['logits'])))
    for _, _, t, logits in hook['logits']:
        _, live, acc, cnt = R.score_step(logits.cpu().numpy(), toks[:, t], live, acc, cnt, 0.5)
    np.testing.assert_allclose(out[:, 0].cpu().numpy(), acc, rtol=RTOL, atol=ATOL)
    assert last['len'][:, 0].tolist() == cnt.tolist()


def test_suppress_unk_and_out_of_range_tokens():
    seq = torch.tensor([[3, VOC, 4, 0, 0, 0]] * B_, device=DEV)
    _, a = _score('updown', seq.unsqueeze(1))
    _, b = _score('updown', seq.unsqueeze(1), suppress_UNK=1)
    d = (a['tok_logp'] - b['tok_logp'])[:, 0]
    assert torch.allclose(d[:, 1], torch.full((B_,), 1000.0, device=DEV), atol=1e-3) and (d[:, [0, 2, 3]].abs() <= 1e-6).all()
    with pytest.raises(ValueError, match=r'\[0, 41\)'):
        _score('updown', torch.full((B_, 1, L_), VOC + 1, device=DEV))


def test_refusals_launch_nothing(monkeypatch):
    from imagecaptioning.pytorch_amd import score
    from imagecaptioning.pytorch_amd.captioning import models
    calls = []
    monkeypatch.setattr(score.ops, 'score_step', lambda *a, **k: calls.append('score_step'))
    model = _family('updown')
    monkeypatch.setattr(model, '_decode_stepper', lambda *a, **k: calls.append('prefill'))
    fc, att, masks = _feats()
    seq = torch.ones(B_, 1, L_, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError, match='output_logsoftmax'):
        model(fc, att, seq, masks, mode='score', opt=dict(output_logsoftmax=0))
    model.train()
    try:
        with pytest.raises(NotImplementedError, match='eval'):
            model(fc, att, seq, masks, mode='score', opt={})
    finally:
        model.eval()
    with pytest.raises(ValueError, match='token ids'):
        model(fc, att, seq * 99, masks, mode='score', opt={})
    ens = models.AttEnsemble([model, _family('att2in2')]).eval()
    with pytest.raises(NotImplementedError, match='AttEnsemble'):
        ens(fc, att, seq, masks, mode='score', opt={})
    assert calls == [] and model.last_score is None


# ---------------------------------------------------------------------------------------------------------------------------
# tools/eval.py
# ---------------------------------------------------------------------------------------------------------------------------
def test_eval_entrypoint(tmp_path):
    from test_langeval_gpu import SMALL, _opts
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd import ops, score
    from imagecaptioning.pytorch_amd.tools import eval as E
    from captioning import models
    common = SMALL + ['--num_images', '10', '--split', 'val']
    with pytest.raises(NotImplementedError, match='rerank'):
        E.main(_opts(common + ['--self_retrieval', '1', '--sample_n', '3', '--eval_results_dir', str(tmp_path / 'no')]))
    out_dir = tmp_path / 'ret'
    _, preds = E.main(_opts(common + ['--self_retrieval', '1', '--retrieval_pool', '4', '--eval_results_dir', str(out_dir)]))
    assert sorted(os.listdir(out_dir)) == ['capmi_val_ret.json'] and len(preds) == 10
    written = json.load(open(out_dir / 'capmi_val_ret.json'))
    overall = written['overall']
    assert overall['pool_sizes'] == [4, 4, 2] and (overall['pool_size'], overall['pools'], overall['captions']) == (4, 3, 10)
    assert written['ranks'] == [p['retrieval_rank'] for p in preds]
    want = score.retrieval_summary(written['ranks'])
    assert all(overall[k] == want[k] for k in ('R@1', 'R@5', 'R@10', 'median_rank', 'mean_rank', 'MRR'))
    # the same model and images again: the ranks are capmi_retrieval_rank of score_captions' matrix
    opt = _opts(common)
    dev = torch.device('cuda:0')
    loader, opt.vocab = E.build_loader(opt, dev)
    torch.manual_seed(1234)
    model = models.setup(opt).to(dev).eval()
    inv = {w: int(i) for i, w in opt.vocab.items()}
    loader.reset_iterator('val')
    fc, att = [], []
    for _ in range(3):
        data = loader.get_batch('val')
        fc.append(data['fc_feats'].to(dev))
        att.append(data['att_feats'].to(dev))
    fc, att = torch.cat(fc)[:10], torch.cat(att)[:10]
    seqs = torch.zeros(10, opt.seq_length, dtype=torch.long)
    for k, p in enumerate(preds):
        ids = [inv[w] for w in p['caption'].split()]
        seqs[k, :len(ids)] = torch.tensor(ids, dtype=torch.long)
    for i0, i1 in ((0, 4), (4, 8), (8, 10)):
        S = score.score_captions(model, fc[i0:i1], att[i0:i1], None, seqs[i0:i1].to(dev), {'pairing': 'cross'})
        rank, post = ops.retrieval_rank(S, torch.arange(i1 - i0))
        assert rank.tolist() == [p['retrieval_rank'] for p in preds[i0:i1]]
        np.testing.assert_allclose(post.tolist(), [p['retrieval_log_post'] for p in preds[i0:i1]], rtol=RTOL, atol=ATOL)
        assert 1 <= min(rank.tolist()) and max(rank.tolist()) <= i1 - i0
    # --score_json: two captions for one image, and an image the split does not hold
    ident = preds[2]['image_id']
    caps = ['w3 w5 w7', 'w3 no-such-word w7 w9']
    path = tmp_path / 'caps.json'
    path.write_text(json.dumps({str(ident): caps, '999': ['w1']}))
    out_dir = tmp_path / 'given'
    E.main(_opts(common + ['--score_json', str(path), '--score_norm', 'length', '--eval_results_dir', str(out_dir)]))
    assert sorted(os.listdir(out_dir)) == ['capmi_val_scores.json']
    got = json.load(open(out_dir / 'capmi_val_scores.json'))
    assert got['missing_image_ids'] == ['999'] and list(got['images']) == [str(ident)] and got['score_norm'] == 'length'
    rows = got['images'][str(ident)]
    assert [r['caption'] for r in rows] == caps and [r['len'] for r in rows] == [4, 5] and [r['oov_words'] for r in rows] == [0, 1]
    enc, _ = score.encode_captions(caps, opt.vocab, opt.seq_length)
    assert enc[1, 1] == inv['UNK']
    direct = model(fc[2:3], att[2:3], enc.unsqueeze(0).to(dev), None, mode='score', opt={})
    for r, lp in zip(rows, direct[0].tolist()):
        assert abs(r['logp'] - lp) <= 1e-4 and abs(r['score'] - lp / r['len']) <= 1e-6 * abs(lp) and abs(r['perplexity'] - np.exp(-lp / r['len'])) <= 1e-4
