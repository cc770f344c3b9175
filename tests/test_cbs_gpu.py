"""Constrained beam search on the device (csrc/cbs.hip, beam.constrained_beam_search_steps, opt['constraints']) against the float64
replay tests/cbs_ref64.py: one selection step at every shape and variant, the finalisation on hand-built tables, the whole search on a
tiny model of every family, the equivalence with the ordinary beam search when nothing is required, and tools/eval.py end to end.

Fixture seeds of the selection cases: the replay must separate the last kept from the first dropped candidate of every (image,
target state) by more than 1e-3 (then the kept set cannot depend on float32 rounding).  A case's seed is the first of
seed0 + 100003 * i, i = 0, 1, ..., that does so, with seed0 = 7919 * b + 31 * V1 + 3 * B + 101 * C + 17 * W + 1009 * variant
(variant: its index in VARIANTS; W: the size of the word sets); the choice reads the replay alone, never the device.  i = 0 serves 1478 of the
1512 cases; the other 34 needed a later seed (each test prints its own count).  Shapes with S * b > 64 (C = 4 with b = 5) are checked to be refused.

The score bound 2^-22 * max(1, |score|) is two float32 ulps: the device's score is one rounded float32 add of float32 inputs."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import cbs_ref64 as R
from test_att_trace_host import tiny_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'imagecaptioning', 'pytorch_amd')
FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')
VARIANTS = ('root', 'plain', 'empty', 'ended', 'inf', 'two_sets', 'force_end', 'mixed')


def _words(rng, B, C, W, V1, variant):
    words = np.full((B, R.C_MAX, R.W_MAX), -1, np.int32)
    ncons = np.full(B, C, np.int32)
    if variant == 'mixed':
        ncons = np.array([(C - k) % (C + 1) for k in range(B)], np.int32)   # C, C - 1, ...: a batch runs with S of its largest C
    for k in range(B):
        pool = rng.permutation(np.arange(1, V1))
        need = C * W
        ids = pool[:need] if need <= len(pool) else rng.integers(1, V1, size=need)      # a small vocabulary repeats words
        for c in range(int(ncons[k])):
            words[k, c, :W] = ids[c * W:(c + 1) * W]
        if variant == 'two_sets' and ncons[k] >= 2:
            words[k, 1, 0] = words[k, 0, 0]                                  # one token satisfies two constraints in one move
    return words, ncons


def _case(B, b, C, W, V1, variant, seed):
    rng = np.random.default_rng(seed)
    S = 1 << C
    SB = S * b
    cur = 1 if variant == 'root' else SB
    words, ncons = _words(rng, B, C, W, V1, variant)
    x = rng.normal(size=(B, cur, V1)) * 2.0
    logp = x - np.log(np.exp(x).sum(-1, keepdims=True))
    if variant == 'inf' and V1 > 2:
        logp[rng.random(size=logp.shape) < 0.3] = -np.inf
    sums = -rng.uniform(0, 20, size=(B, SB))
    if cur == 1:
        sums[:] = 0.0
    else:
        for k in range(B):
            sums[k, (1 << int(ncons[k])) * b:] = -np.inf                     # states the image cannot reach stay empty
        if variant == 'ended':
            sums[rng.random(size=sums.shape) < 0.3] -= 1000.0
        if variant == 'empty':
            for k in range(B):
                s = int(rng.integers(0, S))
                sums[k, s * b:(s + 1) * b] = -np.inf                         # a whole state empty ...
                sums[k, int(rng.integers(0, SB))] = -np.inf                  # ... and one more slot
            logp[np.isneginf(sums)] = np.nan                                 # whatever an empty slot's row holds
    return logp.astype(np.float32), sums.astype(np.float32), words, ncons


def _fixture(B, b, C, W, V1, variant):
    seed0 = 7919 * b + 31 * V1 + 3 * B + 101 * C + 17 * W + 1009 * VARIANTS.index(variant)
    for i in range(50):
        inputs = _case(B, b, C, W, V1, variant, seed0 + 100003 * i)
        ref = R.select_step(*inputs, b, 1 << C, force_end=variant == 'force_end')
        if ref['gap'].min() > 1e-3:
            return i, inputs, ref
    raise AssertionError('no seed separates the candidates')


def _run_select(inputs, b, S, force_end):
    from imagecaptioning.pytorch_amd import ops
    logp, sums, words, ncons = inputs
    B, cur, V1 = logp.shape
    tables = ops.cbs_tables(torch.from_numpy(words), torch.from_numpy(ncons), V1, S, DEV)
    return ops.cbs_select(torch.from_numpy(logp.reshape(B * cur, V1)).to(DEV), torch.from_numpy(sums).to(DEV), tables, b, S,
                          force_end=force_end)


def _compare(out, ref, what):
    parent, token, score, nxt, ended, valid = (x.cpu().numpy() for x in out)
    assert np.array_equal(valid.astype(bool), ref['valid']), what
    assert np.array_equal(parent, ref['parent']), what
    assert np.array_equal(token, ref['token']), what
    assert np.array_equal(ended.astype(bool), ref['ended']), what
    v = ref['valid']
    assert np.isneginf(score[~v]).all() and np.isneginf(nxt[~v]).all(), what
    bound = 2.0 ** -22 * np.maximum(1.0, np.abs(ref['score'][v]))
    err = np.abs(score[v].astype(np.float64) - ref['score'][v])
    assert (err <= bound).all(), (what, float(err.max()))
    assert np.array_equal(nxt[v], np.where(ref['ended'][v], score[v] - np.float32(1000.0), score[v])), what
    return float(err.max()) if v.any() else 0.0


@pytest.mark.parametrize('V1', (5, 33, 257, 1031))
@pytest.mark.parametrize('b', (1, 2, 5))
def test_select_against_the_replay(b, V1):
    """B in {1, 3}; C in {0, 1, 2, 4}; word sets of 1, 3 and 8; the variants of VARIANTS"""
    from imagecaptioning.pytorch_amd import _lib, ops
    later, worst, n = 0, 0.0, 0
    for C in (0, 1, 2, 4):
        S = 1 << C
        if S * b > 64:
            with pytest.raises(_lib.CapmiError):
                z = torch.zeros(S * b, V1, device=DEV)
                ops.cbs_select(z, torch.zeros(1, S * b, device=DEV),
                               ops.cbs_tables(torch.full((1, 4, 8), -1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), V1, S, DEV),
                               b, S)
            continue
        for B in (1, 3):
            for W in (1, 3, 8):
                for variant in VARIANTS:
                    if (variant == 'two_sets' and C < 2) or (variant == 'mixed' and (C < 1 or B < 2)) or (C == 0 and W > 1):
                        continue
                    i, inputs, ref = _fixture(B, b, C, W, V1, variant)
                    later += i > 0
                    n += 1
                    out = _run_select(inputs, b, S, variant == 'force_end')
                    worst = max(worst, _compare(out, ref, (B, b, C, W, V1, variant, i)))
    print('cbs_select b=%d V1=%d: %d cases, %d needed a later seed, worst |score err| %.3g' % (b, V1, n, later, worst))


def test_select_with_long_chunk_lists():
    """V1 = 52999 at b = 5: 52 chunks, so a row's staged lists hold 260 entries -- more than one pass of the merge kernel's 256
    threads, where V1 = 1031 gives 10 -- and, V1 being odd, rows that start off the 16-byte grid.  B = 1, one constraint: 10 rows"""
    b, V1, C, W = 5, 52999, 1, 3
    for variant in ('plain', 'inf'):
        i, inputs, ref = _fixture(1, b, C, W, V1, variant)
        err = _compare(_run_select(inputs, b, 1 << C, False), ref, (1, b, C, W, V1, variant, i))
        print('cbs_select b=%d V1=%d %s: seed index %d, worst |score err| %.3g' % (b, V1, variant, i, err))


def test_select_order_ties_and_errors():
    """equal scores go to the lower flat index; a token in two sets moves once, to the state with both bits; bad tables are refused"""
    from imagecaptioning.pytorch_amd import _lib, ops
    V1, b, S = 9, 2, 4
    words = np.full((1, 4, 8), -1, np.int32)
    words[0, 0, :2] = (3, 5)
    words[0, 1, :2] = (5, 7)
    ncons = np.array([2], np.int32)
    logp = np.full((1, S * b, V1), -2.0, np.float32)                         # every candidate of a row ties
    sums = np.zeros((1, S * b), np.float32)
    sums[0, 3] = -np.inf
    ref = R.select_step(logp, sums, words, ncons, b, S)
    out = _run_select((logp, sums, words, ncons), b, S, False)
    _compare(out, ref, 'ties')
    tok = out[1].cpu().numpy()[0]
    par = out[0].cpu().numpy()[0]
    assert tok[:2].tolist() == [0, 1] and par[:2].tolist() == [0, 0]         # state 0 keeps its own lowest tokens
    assert (par[6], tok[6]) == (0, 5)                                        # state 3 is first reached by token 5 from slot 0
    t = lambda a: torch.from_numpy(a)                                        # noqa: E731
    for bad_words, bad_n in ((np.where(words == 3, 0, words), ncons), (np.where(words == 3, V1, words), ncons),
                             (words, np.array([3], np.int32))):
        with pytest.raises(_lib.CapmiError):
            ops.cbs_tables(t(bad_words), t(bad_n), V1, S, DEV)
    tables = ops.cbs_tables(t(words), t(ncons), V1, S, DEV)
    z = torch.zeros(S * b, V1, device=DEV)
    with pytest.raises(_lib.CapmiError):                                     # cur not in {1, S * b}
        ops.cbs_select(z[:3].contiguous(), torch.zeros(1, S * b, device=DEV), tables, b, S)
    with pytest.raises(_lib.CapmiError):                                     # S no power of two
        ops.cbs_select(torch.zeros(6, V1, device=DEV), torch.zeros(1, 6, device=DEV), tables, 2, 3)
    a, c = _run_select((logp, sums, words, ncons), b, S, False), _run_select((logp, sums, words, ncons), b, S, False)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def _tables(rng, L, B, b, S, ncons, ties):
    SB = S * b
    parent = rng.integers(0, SB, size=(L, B, SB)).astype(np.int32)
    parent[0] = 0
    token = rng.integers(0, 7, size=(L, B, SB)).astype(np.int64)
    score = -rng.uniform(0, 10, size=(L, B, SB))
    if ties:
        score = np.round(score)                                              # many equal keys: the step, then the slot, decide
    ended = rng.random(size=(L, B, SB)) < 0.5
    ended[L - 1] = True
    valid = rng.random(size=(L, B, SB)) < 0.8
    for k in range(B):
        valid[:, k, (1 << int(ncons[k])) * b:] = False
    return parent, token, score.astype(np.float32), ended, valid


@pytest.mark.parametrize('penalty', ('', 'avg_1.0', 'wu_0.7'))
@pytest.mark.parametrize('ties', (False, True))
def test_finalize_against_the_replay(penalty, ties):
    from imagecaptioning.pytorch_amd import beam, ops
    for L, B, b, C, no_full in ((1, 1, 1, 0, False), (5, 3, 2, 2, False), (5, 3, 2, 2, True), (8, 2, 5, 3, True), (7, 3, 3, 1, False),
                                (4, 2, 4, 4, True)):
        rng = np.random.default_rng(1000 * L + 10 * b + C + (5 if ties else 0))
        S = 1 << C
        ncons = np.array([max(C - k, 0) for k in range(B)], np.int32)
        parent, token, score, ended, valid = _tables(rng, L, B, b, S, ncons, ties)
        if no_full:                                                          # nothing ends in the full state: popcount decides
            for k in range(B):
                full = (1 << int(ncons[k])) - 1
                valid[:, k, full * b:(full + 1) * b] = False
            if B > 1:
                valid[:, B - 1] = False                                      # and an image with nothing recorded at all
        div = beam.length_divisors(penalty, L, torch.device(DEV))
        ref = R.finalize(parent, token, score, ended, valid, ncons, b, S, None if div is None else div.cpu().numpy())
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
        seq, lineage, length, state, p = ops.cbs_finalize(t(parent), t(token), t(score), t(ended.astype(np.uint8)),
                                                          t(valid.astype(np.uint8)), t(ncons), b, S, div)
        what = (L, B, b, C, no_full, penalty, ties)
        assert np.array_equal(seq.cpu().numpy(), ref['seq']), what
        assert np.array_equal(lineage.cpu().numpy(), ref['lineage']), what
        assert np.array_equal(length.cpu().numpy(), ref['length']), what
        assert np.array_equal(state.cpu().numpy(), ref['state']), what
        np.testing.assert_allclose(p.cpu().numpy(), ref['score'], rtol=2.0 ** -22, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------
# the whole search
# ---------------------------------------------------------------------------------------------------------------------------
B_, L_, VOC = 3, 6, 40
_models = {}


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


def _sample(model, **opt):
    gen = torch.Generator().manual_seed(5)
    fc, att = torch.randn(B_, 20, generator=gen).to(DEV), torch.randn(B_, 5, 20, generator=gen).to(DEV)
    with torch.no_grad():
        return model(fc, att, None, opt=opt, mode='sample')


@pytest.mark.parametrize('C', (1, 2))
@pytest.mark.parametrize('name', FAMILIES)
def test_search_on_a_tiny_model(name, C):
    """b = 2; image 0 has C constraints (words and ids mixed), image 1 one fewer, image 2 C again: every step's selection is the
    replay's on the device's own rows, the caption is the replay's pick and holds the required words, the log-probs are the rows"""
    model = _family(name)
    b, V1 = 2, VOC + 1
    cons = [[['w7', 'w8'], [11, 'w12', 13]][:C], [[21]][:C - 1], [['w30'], ['w31', 'w7']][:C]]
    hook = {}
    seq, logp = _sample(model, beam_size=b, constraints=cons, _cbs_tables=hook)
    assert seq.shape == (B_, L_) and logp.shape == (B_, L_, V1) and seq.dtype == torch.long
    S = 1 << C
    assert (hook['b'], hook['S']) == (b, S)
    words, ncons = hook['words'].numpy(), hook['ncons'].numpy()
    assert ncons.tolist() == [C, C - 1, C] and words[0, 0, :3].tolist() == [7, 8, -1]
    rows = hook['logp_rows'].cpu().numpy()
    dev = {k: hook[k].cpu().numpy() for k in ('parent', 'token', 'score', 'ended', 'valid')}
    sums = np.zeros((B_, S * b), np.float32)
    for t in range(L_):
        cur = 1 if t == 0 else S * b
        ref = R.select_step(rows[t, :B_ * cur].reshape(B_, cur, V1), sums, words, ncons, b, S, force_end=t == L_ - 1)
        for k in ('parent', 'token'):
            assert np.array_equal(dev[k][t], ref[k]), (name, C, t, k, float(ref['gap'].min()))
        assert np.array_equal(dev['valid'][t].astype(bool), ref['valid']) and np.array_equal(dev['ended'][t].astype(bool), ref['ended'])
        v = ref['valid']
        assert (np.abs(dev['score'][t][v] - ref['score'][v]) <= 2.0 ** -22 * np.maximum(1, np.abs(ref['score'][v]))).all()
        sums = np.where(v, np.where(ref['ended'], dev['score'][t] - np.float32(1000.0), dev['score'][t]), -np.inf).astype(np.float32)
    fin = R.finalize(dev['parent'], dev['token'], dev['score'], dev['ended'], dev['valid'], ncons, b, S)
    assert np.array_equal(seq.cpu().numpy(), fin['seq'])
    assert np.array_equal(hook['lineage'].cpu().numpy(), fin['lineage'])
    last = model.last_cbs
    assert sorted(last) == ['satisfied', 'score', 'state', 'total'] and all(x.shape == (B_,) and x.is_cuda for x in last.values())
    assert last['state'].tolist() == fin['state'].tolist() and last['total'].tolist() == ncons.tolist()
    assert last['satisfied'].tolist() == [R.popcount(s) for s in fin['state']]
    toks = seq.cpu().tolist()
    for k in range(B_):
        for c in range(int(ncons[k])):
            want = set(int(w) for w in words[k, c] if w >= 0)
            assert bool(want & set(toks[k])) == bool(want & set(fin['seq'][k].tolist()))
            if (fin['state'][k] >> c) & 1:
                assert want & set(toks[k]), (k, c, toks[k])
    assert last['satisfied'].tolist() == last['total'].tolist()              # L = 6 leaves room for two words: all are met
    lin = hook['lineage'].long()
    for t in range(L_):
        for k in range(B_):
            row = hook['logp_rows'][t, lin[t, k]] if lin[t, k] >= 0 else torch.zeros(V1, device=DEV)
            assert torch.equal(logp[k, t], row)
    if name in ('updown', 'adaatt'):                                         # return_attention rides the lineage
        seq2, _ = _sample(model, beam_size=b, constraints=cons, return_attention=1)
        assert torch.equal(seq, seq2) and model.last_attention['att'].shape[:2] == (B_, L_)


@pytest.mark.parametrize('name', FAMILIES)
def test_no_constraint_is_the_ordinary_beam_search(name):
    model = _family(name)
    model.bad_endings_ix = [3, 4, 5]
    for b, extra in ((2, {}), (3, dict(temperature=0.8, suppress_UNK=1, decoding_constraint=1, remove_bad_endings=1,
                                      length_penalty='wu_0.5')), (5, dict(length_penalty='avg_1.0', temperature=1.3))):
        seq0, logp0 = _sample(model, beam_size=b, sample_n=1, **extra)
        seq, logp = _sample(model, beam_size=b, sample_n=1, constraints=[[] for _ in range(B_)], **extra)
        assert torch.equal(seq, seq0), (name, b, extra)
        assert torch.equal(logp, logp0), (name, b, extra)
        assert model.last_cbs['total'].tolist() == [0] * B_ and model.last_cbs['state'].tolist() == [0] * B_


def test_refusals_reach_the_model():
    model = _family('updown')
    with pytest.raises(ValueError, match='w99'):
        _sample(model, beam_size=2, constraints=[[['w99']], [], []])
    with pytest.raises(ValueError, match='lists 2 images'):
        _sample(model, beam_size=2, constraints=[[], []])
    with pytest.raises(NotImplementedError):
        _sample(model, beam_size=2, constraints=[[], [], []], sample_method='sample')


def test_eval_entrypoint(tmp_path):
    from test_langeval_gpu import SMALL, _opts
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    common = SMALL + ['--num_images', '4', '--split', 'val', '--language_eval', '1', '--beam_size', '2']
    _, vocab = E.build_loader(_opts(common), torch.device(DEV))
    _, plain, _ = E.main(_opts(common + ['--eval_results_dir', str(tmp_path / 'plain')]))
    assert all('constraints_total' not in p for p in plain) and sorted(os.listdir(tmp_path / 'plain')) == ['capmi_val.json']
    ids = [p['image_id'] for p in plain][:3]
    w = [vocab[str(i)] for i in (5, 6, 9)]
    spec = {str(ids[0]): [[w[0], w[1]], [w[2]]], str(ids[1]): [[w[1], 'no-such-word']], str(ids[2]): [['no-such-word']]}
    path = tmp_path / 'cons.json'
    path.write_text(json.dumps(spec))
    with pytest.raises(ValueError, match='no-such-word'):
        E.main(_opts(common + ['--eval_results_dir', str(tmp_path / 'err'), '--constraints_json', str(path)]))
    out_dir = tmp_path / 'cbs'
    loss, preds, stats = E.main(_opts(common + ['--eval_results_dir', str(out_dir), '--constraints_json', str(path),
                                                '--constraints_oov', 'drop']))
    assert sorted(os.listdir(out_dir)) == ['capmi_val.json', 'capmi_val_cbs.json']
    assert len(preds) == 4 and all(np.isfinite(v) for v in stats.values())
    by_id = {p['image_id']: p for p in preds}
    assert by_id[ids[0]]['constraints_total'] == 2 and by_id[ids[1]]['constraints_total'] == 1
    assert by_id[ids[2]]['constraints_total'] == 0                           # its only word was dropped, and the constraint with it
    written = json.load(open(out_dir / 'capmi_val_cbs.json'))
    assert written['overall']['dropped_words'] == 2 and written['overall']['dropped_constraints'] == 1
    assert written['overall']['images'] == 4 and written['overall']['constrained_images'] == 2
    rows = {r['image_id']: r for r in written['images']}
    full = 0
    for p in preds:
        assert (rows[p['image_id']]['constraints_satisfied'], rows[p['image_id']]['constraints_total']) == \
            (p['constraints_satisfied'], p['constraints_total'])
        full += p['constraints_total'] > 0 and p['constraints_satisfied'] == p['constraints_total']
    assert written['overall']['fully_satisfied'] == full / 2
    cap = by_id[ids[0]]['caption'].split()
    if by_id[ids[0]]['constraints_satisfied'] == 2:
        assert (w[0] in cap or w[1] in cap) and w[2] in cap
