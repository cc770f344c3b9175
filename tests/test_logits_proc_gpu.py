"""The logits processors on the device (csrc/logits_proc.hip, imagecaptioning/pytorch_amd/logits_proc.py): the kernel bit for bit
against tests/logits_proc_ref.py with the history in both forms, then greedy / sampled / beam / stochastic / constrained decoding of
the tiny golden models with the options on -- the properties of every caption, and greedy and beam search against a host replay
that steps the model's own stepper and edits the rows with the restatement.

The end-to-end fixtures are logit-bias perturbations, fixed by reasoning and not by a search (there is nothing random in them, so no
seed: SEED below only draws the injected Gumbel noise).  The tiny models' own logits stay within a few units, a bias of BIAS = 30
decides the token whatever they say, and Gumbel noise over the 31 * 8 * 9 draws of a call stays below 15:
  'repeat'  words 3 and 4 get +BIAS, the end token -BIAS.  Without the options every caption is 8 words over {3, 4} (one of them may
            be a required word in the constrained search): 7 bigrams of 4 kinds, so a bigram repeats (pigeonhole; with a required
            word in between, 5 or 6 bigrams), and every run of 3 such words holds one of the banned 33, 44, 343, 434.
  'short'   the end token gets +BIAS: without the options every caption ends at once, length 0 < min_length.
So with the options off EVERY row violates every property (the vacuity guards assert at least half), and with them on a violation
can only come from the code under test."""
import json
import os

import numpy as np
import pytest
import torch

import logits_proc_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 20261021
BIAS = 30.0
BANNED = [[3, 3], [4, 4], [3, 4, 3], [4, 3, 4]]
ON = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_length=6, bad_words=BANNED)


# ------------------------------------------------------------------------------------------------ the kernel
def _histories(rng, rows, t):
    """[rows, t] over a 6-word alphabet (n-grams recur); about a quarter of the rows finished: 0 from some step on"""
    h = rng.integers(1, 7, size=(rows, max(t, 1)))[:, :t]
    for r in range(rows):
        if t and rng.random() < 0.25:
            h[r, rng.integers(0, t):] = 0
    return h


def _tables(rng, hist, B, W, L):
    """the search core's tables [L, B, W] holding `hist` [B * W, t] behind shuffled parents: row b * W + j is slot j of step t - 1
    and sits at slot sigma_s[b][j] of every earlier step s"""
    t = hist.shape[1]
    token = rng.integers(1, 7, size=(L, B, W))                    # junk wherever no history passes
    parent = rng.integers(0, W, size=(L, B, W))
    for b in range(B):
        sigma = [rng.permutation(W) for _ in range(t)]
        if t:
            sigma[t - 1] = np.arange(W)
        for s in range(t):
            for j in range(W):
                token[s, b, sigma[s][j]] = hist[b * W + j, s]
                parent[s, b, sigma[s][j]] = sigma[s - 1][j] if s else 0
    return token.astype(np.int64), parent.astype(np.int32)


def _launch(x, t, L, opts, seq=None, token=None, parent=None, cur=1, exempt=None):
    from imagecaptioning.pytorch_amd import logits_proc as LP
    rows, V1 = x.shape
    proc = LP.Processor(opts, L)
    y = torch.from_numpy(x).to(DEV)
    if seq is not None:
        proc.dense(y, rows, V1, t, torch.from_numpy(seq).to(DEV), cur)
    else:
        proc.search(y, rows, V1, t, torch.from_numpy(token).to(DEV), torch.from_numpy(parent).to(DEV), cur,
                    None if exempt is None else torch.from_numpy(exempt).to(DEV))
    return y.cpu().numpy()


def _same_bits(a, b, what):
    assert np.array_equal(np.isneginf(a), np.isneginf(b)), what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


SPLIT = {1: (1, 1), 7: (1, 7), 65: (5, 13)}                         # rows -> (B, W) of the back-pointer form


@pytest.mark.parametrize('V1', (31, 9488))
@pytest.mark.parametrize('rows', (1, 7, 65))
def test_kernel_against_the_restatement_bit_for_bit(rows, V1):
    """L in {4, 20, 64}, n in {1, 2, 3, 4, 8}, t in {0, n - 2, n - 1, L - 1}; n alone and all four options at once; the history
    dense and through shuffled parent pointers"""
    rng = np.random.default_rng(1000 * rows + V1)
    B, W = SPLIT[rows]
    base = (-np.abs(rng.normal(size=(rows, V1))) * 3).astype(np.float32)
    base[rng.random(size=base.shape) < 0.02] = -np.inf             # rows that an earlier constraint has edited
    blocked = penalised = 0
    for L in (4, 20, 64):
        for n in (1, 2, 3, 4, 8):
            for t in sorted({0, max(n - 2, 0), n - 1, L - 1}):
                if t >= L:
                    continue
                hist = _histories(rng, rows, t)
                for opts in (dict(no_repeat_ngram_size=n),
                             dict(no_repeat_ngram_size=n, repetition_penalty=1.3, min_length=L // 2 + 1,
                                  bad_words=[[5], [3, 4], [1, 2, 1, 2], [6, 6, 2]])):
                    want = np.stack([R.process(base[r], hist[r], t, L, opts) for r in range(rows)])
                    seq = np.zeros((rows, L), np.int64)
                    seq[:, :t] = hist
                    seq[:, t:] = 99                                          # columns from t on are not history
                    what = (rows, V1, L, n, t, sorted(opts))
                    _same_bits(_launch(base.copy(), t, L, opts, seq=seq), want, ('dense',) + what)
                    if t == 0:
                        token, parent = _tables(rng, hist, rows, 1, L)       # the root step: one row per image
                        got = _launch(base.copy(), t, L, opts, token=token, parent=parent, cur=1)
                    else:
                        token, parent = _tables(rng, hist, B, W, L)
                        for r in range(rows):
                            assert R.history_from_parents(token, parent, t, r) == hist[r].tolist()
                        got = _launch(base.copy(), t, L, opts, token=token, parent=parent, cur=W)
                    _same_bits(got, want, ('parents',) + what)
                    blocked += int((np.isneginf(want) & ~np.isneginf(base)).sum())
                    penalised += int(((want != base) & ~np.isneginf(want)).sum())
    assert blocked > 0 and penalised > 0                                      # the cases do edit rows


def test_kernel_spares_exempt_words_and_leaves_defaults_alone():
    rng = np.random.default_rng(5)
    B, W, V1, L, t = 2, 3, 31, 8, 5
    base = (-np.abs(rng.normal(size=(B * W, V1)))).astype(np.float32)
    hist = np.array([[1, 2, 1, 2, 1]] * (B * W))
    token, parent = _tables(rng, hist, B, W, L)
    exempt = np.array([[2, -1], [-1, -1]], np.int32)                          # image 0 spares word 2, image 1 nothing
    opts = dict(no_repeat_ngram_size=2)
    got = _launch(base.copy(), t, L, opts, token=token, parent=parent, cur=W, exempt=exempt)
    want = np.stack([R.process(base[r], hist[r], t, L, opts, exempt=(2,) if r < W else ()) for r in range(B * W)])
    _same_bits(got, want, 'exempt')
    assert not np.isneginf(got[:W]).any() and np.isneginf(got[W:, 2]).all()
    # every option at its default: no launch, the rows keep their bits
    from imagecaptioning.pytorch_amd import _lib, logits_proc as LP
    from imagecaptioning.pytorch_amd._lib import lib, ptr, stream_ptr
    import ctypes as C
    y = torch.from_numpy(base).to(DEV)
    p = LP.struct(0, 1.0, 0, [])
    seq = torch.zeros(B * W, L, dtype=torch.long, device=DEV)
    assert lib.capmi_logits_process(ptr(y), V1, B * W, V1, 3, L, C.byref(p), ptr(seq), L, None, None, 0, 1, None, 0, stream_ptr()) == 0
    assert np.array_equal(y.cpu().numpy().view(np.uint32), base.view(np.uint32))
    # a history longer than the kernel's LDS buffer is refused, as is a step outside [0, L)
    p = LP.struct(2, 1.0, 0, [])
    seq = torch.zeros(B * W, 65, dtype=torch.long, device=DEV)
    assert lib.capmi_logits_process(ptr(y), V1, B * W, V1, 3, 65, C.byref(p), ptr(seq), 65, None, None, 0, 1, None, 0,
                                    stream_ptr()) == _lib.EINVAL
    assert lib.capmi_logits_process(ptr(y), V1, B * W, V1, 8, L, C.byref(p), ptr(seq), 65, None, None, 0, 1, None, 0,
                                    stream_ptr()) == _lib.EINVAL
    assert np.array_equal(y.cpu().numpy().view(np.uint32), base.view(np.uint32))


# ------------------------------------------------------------------------------------------------ end to end
NAMES = ('updown', 'transformer', 'ensemble')
_cache = {}


def _bias_of(model):
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    if isinstance(model, AttEnsemble):
        return [b for m in model.models for b in _bias_of(m)]
    return [p for n, p in model.named_parameters() if n in ('logit.bias', 'model.generator.proj.bias')]


def _model(name, fixture):
    """the tiny golden model(s) with the fixture's logit bias (see the module docstring)"""
    from test_ensemble_gpu import ensemble, family_model, inputs
    key = (name, fixture)
    if key not in _cache:
        model = ensemble(['updown', 'att2in2']) if name == 'ensemble' else family_model(name)
        biases = _bias_of(model)
        assert len(biases) == (2 if name == 'ensemble' else 1)
        with torch.no_grad():
            for b in biases:
                if fixture == 'repeat':
                    b[3] += BIAS
                    b[4] += BIAS
                    b[0] -= BIAS
                else:
                    b[0] += BIAS
        _cache[key] = model
    return (_cache[key],) + tuple(inputs()[:3])


def _sample(model, fc, att, am, **opt):
    torch.manual_seed(SEED)
    model._rng_calls = 0
    with torch.no_grad():
        return model(fc, att, am, opt=opt, mode='sample')


def _gumbel(rows, L=8, V1=31):
    return torch.from_numpy(np.random.default_rng(SEED).gumbel(size=(L, rows, V1)).astype(np.float32)).to(DEV)


def _caption(row):
    row = [int(v) for v in row]
    return row[:row.index(0)] if 0 in row else row


def _repeats(cap, n, spare=()):
    """an n-gram of the caption occurs twice (n-grams that end in a spared word do not count)"""
    grams = [tuple(cap[i:i + n]) for i in range(len(cap) - n + 1) if cap[i + n - 1] not in spare]
    return len(set(grams)) < len(grams)


def _has_banned(cap, banned):
    return any(cap[i:i + len(b)] == list(b) for b in banned for i in range(len(cap) - len(b) + 1))


MODES = {'greedy': dict(), 'sample': dict(sample_method='sample', sample_n=2), 'beam': dict(beam_size=3, sample_n=1),
         'sbs': dict(sample_method='sbs', sample_n=3), 'cbs': dict(beam_size=3, constraints=[[[7]], [[7]], [[9, 10]]])}


def _decode(name, fixture, mode, on):
    model, fc, att, am = _model(name, fixture)
    opt = dict(MODES[mode])
    if mode == 'sample':
        opt['_gumbel'] = _gumbel(3 * 2)
    if mode == 'sbs':
        opt['_gumbel'] = _gumbel(3 * 3)
    seq, logp = _sample(model, fc, att, am, **opt, **on)
    return [_caption(r) for r in seq.cpu().tolist()], seq, logp


# AttEnsemble refuses sbs and constraints (CaptionModel._sbs_refusal / _cbs_refusal, as before): no such cases
CASES = [(n, m) for n in NAMES for m in sorted(MODES) if not (n == 'ensemble' and m in ('sbs', 'cbs'))]


@pytest.mark.parametrize('name,mode', CASES)
def test_no_ngram_twice_and_no_banned_sequence(name, mode):
    spare = (7, 9, 10) if mode == 'cbs' else ()                              # cbs: the n-gram rule spares the required words
    off, _, _ = _decode(name, 'repeat', mode, {})
    assert 2 * sum(_repeats(c, 2, spare) for c in off) >= len(off), off      # vacuity guard: without the options they do repeat
    assert 2 * sum(_has_banned(c, BANNED) for c in off) >= len(off), off
    on, _, logp = _decode(name, 'repeat', mode, ON)
    assert len(on) == len(off)
    for c in on:
        assert not _repeats(c, 2, spare), (c, on)
        assert not _has_banned(c, BANNED), (c, on)
        assert len(c) >= 6, (c, on)
    assert bool(torch.isneginf(logp).any())                                   # the stored rows are the edited ones
    if mode == 'cbs':
        assert all(7 in c for c in on[:2]) and (9 in on[2] or 10 in on[2])    # and the constraints are still met


@pytest.mark.parametrize('name,mode', CASES)
def test_min_length(name, mode):
    off, _, _ = _decode(name, 'short', mode, {})
    assert 2 * sum(len(c) < 7 for c in off) >= len(off), off                 # vacuity guard: without the option they end early
    for m, least in ((3, 3), (100, 7)):                                      # L = 8: min(m, L - 1)
        on, _, _ = _decode(name, 'short', mode, dict(min_length=m))
        assert all(len(c) >= least for c in on), (m, on)
        if mode in ('greedy', 'beam') and m == 3:
            assert all(len(c) == 3 for c in on), on                          # and the biased end token is taken as soon as it may be


def _stepper_factory(model, fc, att, am):
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    if isinstance(model, AttEnsemble):
        return model._stepper_factory(fc, att, am)
    return model._decode_stepper(fc, att, am, model.seq_length)


def _rows(logits, hists, t, L, opts):
    lp = torch.log_softmax(logits.float(), -1).cpu().numpy()
    return np.stack([R.process(lp[r], hists[r], t, L, opts) for r in range(lp.shape[0])])


def _close(got, want, what):
    """the tolerance of tests/test_contrastive_gpu.py / test_att2in2_gpu.py for seqLogprobs; -inf where and only where the replay has it"""
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what
    fin = ~np.isneginf(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=2e-5, atol=5e-6, err_msg=str(what))


@pytest.mark.parametrize('name', NAMES)
def test_greedy_equals_the_host_replay(name):
    model, fc, att, am = _model(name, 'repeat')
    B, L, V1 = 3, 8, 31
    seq, logp = _sample(model, fc, att, am, **ON)
    with torch.no_grad():
        dec = _stepper_factory(model, fc, att, am)(1)
        it = torch.zeros(B, dtype=torch.long, device=DEV)
        want = np.zeros((B, L), np.int64)
        live = np.ones(B, bool)
        got_logp = logp.cpu().numpy()
        for t in range(L):
            rows = _rows(dec.step(t, it, 1), want, t, L, ON)
            if not live.any():
                break
            _close(got_logp[live, t], rows[live], (name, t))
            tok = np.where(live, rows.argmax(1), 0)                          # argmax: the first of equal values
            want[:, t] = tok
            live &= tok > 0
            it = torch.from_numpy(tok).to(DEV)
    assert np.array_equal(seq.cpu().numpy(), want), (seq.tolist(), want.tolist())


@pytest.mark.parametrize('name', NAMES)
def test_beam_equals_the_host_replay(name):
    """capmi_beam_select's rule restated: candidates sums + logp in float32, the larger first, equal ones by the lower flat index;
    an ended beam goes on 1000 lower; the caption is the best finished beam (the earliest of equal ones)"""
    model, fc, att, am = _model(name, 'repeat')
    B, L, V1, bd = 3, 8, 31, 3
    seq, logp = _sample(model, fc, att, am, beam_size=bd, sample_n=1, **ON)
    token, parent = np.zeros((L, B, bd), np.int64), np.zeros((L, B, bd), np.int64)
    score, ended = np.zeros((L, B, bd), np.float32), np.zeros((L, B, bd), bool)
    rows_all = np.zeros((L, B * bd, V1), np.float32)
    with torch.no_grad():
        dec = _stepper_factory(model, fc, att, am)(bd)
        it, cur = torch.zeros(B, dtype=torch.long, device=DEV), 1
        sums = np.zeros((B, 1), np.float32)
        for t in range(L):
            hists = [R.history_from_parents(token, parent, t, r) for r in range(B * cur)]
            rows = _rows(dec.step(t, it, cur), hists, t, L, ON)
            rows_all[t, :B * cur] = rows
            nxt = np.zeros((B, bd), np.float32)
            for b in range(B):
                cand = (sums[b][:, None] + rows[b * cur:(b + 1) * cur]).reshape(-1)
                order = np.argsort(-cand, kind='stable')[:bd]
                parent[t, b], token[t, b], score[t, b] = order // V1, order % V1, cand[order]
                ended[t, b] = (token[t, b] == 0) | (t == L - 1)
                nxt[b] = np.where(ended[t, b], score[t, b] - np.float32(1000.0), score[t, b])
            sums = nxt
            if t == L - 1:
                break
            dec.reorder(torch.from_numpy(parent[t].astype(np.int32)).to(DEV), cur)
            it, cur = torch.from_numpy(token[t].reshape(-1)).to(DEV), bd
    got_seq, got_logp = seq.cpu().numpy(), logp.cpu().numpy()
    for b in range(B):
        fin = [(score[t, b, j], t, j) for t in range(L) for j in range(bd) if ended[t, b, j]]
        p, t, j = sorted(fin, key=lambda x: -x[0])[0]
        toks, rows = [], []
        for s in range(t, -1, -1):
            toks.append(int(token[s, b, j]))
            rows.append(rows_all[s, b if s == 0 else b * bd + parent[s, b, j]])
            j = parent[s, b, j]
        toks, rows = toks[::-1], rows[::-1]
        assert got_seq[b].tolist() == toks + [0] * (L - len(toks)), (name, b, got_seq[b].tolist(), toks)
        _close(got_logp[b, :len(toks)], np.stack(rows), (name, b))
        cap = _caption(toks)
        assert not _repeats(cap, 2) and not _has_banned(cap, BANNED) and len(cap) >= 6


@pytest.mark.parametrize('name', NAMES)
def test_defaults_are_bit_identical(name):
    model, fc, att, am = _model(name, 'repeat')
    defaults = dict(no_repeat_ngram_size=0, repetition_penalty=1.0, min_length=0, bad_words=None)
    for opt in (dict(), dict(beam_size=3, sample_n=1)):
        a = _sample(model, fc, att, am, **opt)
        b = _sample(model, fc, att, am, **opt, **defaults)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (name, opt)


def test_eval_entrypoint(tmp_path):
    from test_langeval_gpu import SMALL, _opts
    from imagecaptioning.pytorch_amd.tools import eval as E
    common = SMALL + ['--num_images', '4', '--split', 'val', '--language_eval', '1', '--beam_size', '3']
    _, vocab = E.build_loader(_opts(common), torch.device(DEV))
    bad = tmp_path / 'f.json'
    bad.write_text(json.dumps([vocab['5'], '%s %s' % (vocab['6'], vocab['7']), [vocab['8'], vocab['9'], vocab['6']]]))
    out_dir = tmp_path / 'out'
    opt = _opts(common + ['--eval_results_dir', str(out_dir), '--no_repeat_ngram_size', '2', '--min_length', '4',
                          '--repetition_penalty', '1.2', '--bad_words_json', str(bad)])
    _, preds, stats = E.main(opt)
    L = opt.max_length
    written = json.load(open(out_dir / 'capmi_val.json'))
    assert written['logits_processors'] == {'no_repeat_ngram_size': 2, 'repetition_penalty': 1.2, 'min_length': 4,
                                            'bad_words': [[5], [6, 7], [8, 9, 6]]}
    assert set(written) == {'overall', 'imgToEval', 'logits_processors'} and all(np.isfinite(v) for v in stats.values())
    assert len(preds) == 4 and all(set(p) == {'image_id', 'caption', 'perplexity', 'entropy'} for p in preds)
    banned = [[vocab['5']], [vocab['6'], vocab['7']], [vocab['8'], vocab['9'], vocab['6']]]
    for p in preds:
        words = p['caption'].split()
        assert not _repeats(words, 2) and not _has_banned(words, banned) and len(words) >= min(4, L - 1), p
    # without the options the file has no such key
    E.main(_opts(common + ['--eval_results_dir', str(tmp_path / 'plain')]))
    assert set(json.load(open(tmp_path / 'plain' / 'capmi_val.json'))) == {'overall', 'imgToEval'}
