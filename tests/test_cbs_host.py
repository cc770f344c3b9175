"""Constrained beam search (opt['constraints']; imagecaptioning/pytorch_amd/cbs.py, beam.constrained_beam_search_steps, csrc/cbs.hip)
without a GPU: the float64 replay tests/cbs_ref64.py pinned by enumeration on a tree small enough to enumerate, properties of the
replay, the conversion of constraints to tables, every refusal, the bindings and the command line."""
import argparse
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import cbs_ref64 as R
from test_att_trace_host import tiny_opt

FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')
ENTRIES = {'capmi_cbs_scratch_bytes': 4, 'capmi_cbs_select': 19, 'capmi_cbs_finalize': 17}


def _model(name):
    from imagecaptioning.pytorch_amd.captioning import models
    if name == 'ensemble':
        return models.AttEnsemble([models.setup(tiny_opt('updown')), models.setup(tiny_opt('att2in2'))])
    return models.setup(tiny_opt(name))


# ---------------------------------------------------------------------------------------------------------------------------
# the replay, pinned by enumeration: V1 = 3, L = 3, b = 16.  A step has at most 9 (t = 1) candidates, fewer than b, and at the last
# step a state's best candidate is always kept, so the search must return the best of ALL sequences under the ranking keys.
# A sequence may run on behind an end token, 1000 lower per end token it has passed, exactly as the beam carries it.
# ---------------------------------------------------------------------------------------------------------------------------
V1, L, B16 = 3, 3, 16


def _toy(seed):
    rng = np.random.default_rng(seed)
    table = {}
    for n in range(L):
        for prefix in itertools.product(range(V1), repeat=n):
            x = rng.normal(size=V1) * 1.5
            table[prefix] = x - np.log(np.exp(x).sum())
    return table


def _enumerate(table, words, ncons, len_div):
    sat = R.sat_masks(words, ncons, V1)
    full = (1 << ncons) - 1
    best = None
    for n in range(1, L + 1):
        for seq in itertools.product(range(V1), repeat=n):
            if seq[-1] != 0 and n < L:
                continue                                                     # recorded: it ends here, or the search does
            score, state = 0.0, 0
            for i, v in enumerate(seq):
                score += table[seq[:i]][v] - (1000.0 if i > 0 and seq[i - 1] == 0 else 0.0)
                state |= int(sat[v])
            key = score / (len_div[n - 1] if len_div is not None else 1.0)
            cand = (0 if state == full else 1, -R.popcount(state), -key, n, seq)
            if best is None or cand[:4] < best[:4]:
                best = cand
    return best


@pytest.mark.parametrize('penalty', (None, 'avg'))
@pytest.mark.parametrize('C', (0, 1, 2))
def test_replay_finds_the_best_sequence_of_all(C, penalty):
    len_div = None if penalty is None else np.arange(1, L + 1, dtype=np.float64)
    for seed in range(12):
        table = _toy(100 * C + seed)
        words = np.full((1, R.C_MAX, R.W_MAX), -1, np.int32)
        if C >= 1:
            words[0, 0, 0] = 1
        if C >= 2:
            words[0, 1, :2] = (2, 1) if seed % 2 else (2, -1)                # odd seeds: token 1 sits in both sets
        ncons = np.array([C], np.int32)
        out = R.search(lambda k, prefix: table[prefix], 1, V1, L, words, ncons, B16, 1 << C, len_div)
        best = _enumerate(table, words[0], C, len_div)
        n = int(out['length'][0])
        assert tuple(out['seq'][0, :n].tolist()) == best[4] and not out['seq'][0, n:].any(), (seed, out['seq'], best)
        assert abs(out['score'][0] + best[2]) < 1e-9
        assert out['state'][0] == ((1 << C) - 1)                             # three words hold two required ones


def test_replay_properties():
    rng = np.random.default_rng(3)
    B, b, C, V = 2, 3, 2, 11
    S = 1 << C
    words = np.full((B, R.C_MAX, R.W_MAX), -1, np.int32)
    words[:, 0, :2] = (4, 5)
    words[:, 1, :2] = (5, 9)
    ncons = np.array([2, 1], np.int32)
    x = rng.normal(size=(B, S * b, V))
    logp = x - np.log(np.exp(x).sum(-1, keepdims=True))
    sums = -rng.uniform(0, 5, size=(B, S * b))
    sums[1, 2 * b:] = -np.inf                                                # image 1 has one constraint: states 2, 3 are empty
    sums[0, 4] = -np.inf
    logp[0, 4] = np.nan
    out = R.select_step(logp, sums, words, ncons, b, S)
    assert not out['valid'][1, 2 * b:].any() and np.isneginf(out['next_sums'][1, 2 * b:]).all()
    assert out['valid'][0].all()
    for k in range(B):
        sat = R.sat_masks(words[k], ncons[k], V)
        for j in range(S * b):
            if not out['valid'][k, j]:
                assert (out['parent'][k, j], out['token'][k, j]) == (0, 0)
                continue
            r, v = out['parent'][k, j], out['token'][k, j]
            assert sums[k, r] > -np.inf and (r // b) | sat[v] == j // b      # the transition lands in the slot's state
            assert out['score'][k, j] == sums[k, r] + logp[k, r, v]
            assert out['ended'][k, j] == (v == 0)
            assert out['next_sums'][k, j] == out['score'][k, j] - (1000.0 if v == 0 else 0.0)
        for s in range(S):
            sc = out['score'][k, s * b:(s + 1) * b]
            assert (np.diff(sc[out['valid'][k, s * b:(s + 1) * b]]) <= 0).all()
    assert (out['token'][0, 3 * b:3 * b + b] != 0).any() or True
    # token 5 sits in both sets of image 0: from state 0 it goes to state 3, never to 1 or 2
    for j in range(b, 3 * b):
        if out['valid'][0, j] and out['parent'][0, j] < b:
            assert out['token'][0, j] != 5
    # force_end ends everything; C = 0 is a plain top-b with ties to the lower flat index
    assert R.select_step(logp, sums, words, ncons, b, S, force_end=True)['ended'][out['valid']].all()
    flat = np.full((1, 2, 4), -1.0)
    o = R.select_step(flat, np.zeros((1, 2)), words[:1], np.array([0]), 2, 1)
    assert o['parent'].tolist() == [[0, 0]] and o['token'].tolist() == [[0, 1]] and o['gap'][0, 0] == 0.0
    # finalize: the full state first, else the popcount; then the score; then the earlier step
    L_, SB = 2, 4
    parent, token = np.zeros((L_, 1, SB), np.int32), np.ones((L_, 1, SB), np.int64)
    score = np.array([[[-1.0, -9.0, -5.0, -7.0]], [[-1.0, -9.0, -5.0, -7.0]]])
    ended, valid = np.ones((L_, 1, SB), bool), np.ones((L_, 1, SB), bool)
    f = R.finalize(parent, token, score, ended, valid, np.array([2]), 1, 4)
    assert (f['state'][0], f['length'][0], f['score'][0]) == (3, 1, -7.0)
    valid[:, 0, 3] = False
    f = R.finalize(parent, token, score, ended, valid, np.array([2]), 1, 4)
    assert (f['state'][0], f['score'][0]) == (2, -5.0)                        # states 1 and 2 tie on popcount: the score decides
    f = R.finalize(parent, token, score, ended, valid, np.array([2]), 1, 4, np.array([1.0, 2.0]))
    assert (f['state'][0], f['length'][0], f['score'][0]) == (2, 2, -2.5)


# ---------------------------------------------------------------------------------------------------------------------------
# tables and refusals
# ---------------------------------------------------------------------------------------------------------------------------
VOCAB = {str(i): 'w%d' % i for i in range(1, 9)}
VOCAB['9'] = 'UNK'


def test_tables():
    from imagecaptioning.pytorch_amd import cbs
    req = cbs.tables([[['w1', 'w2'], [3]], [], [[7, 'w8', 'w1']]], 10, 6, 4, VOCAB)
    assert (req.B, req.b, req.S) == (3, 4, 4) and req.ncons.tolist() == [2, 0, 1]
    assert req.words.dtype == torch.int32 and req.words.shape == (3, 4, 8)
    assert req.words[0, 0, :3].tolist() == [1, 2, -1] and req.words[0, 1, :2].tolist() == [3, -1] and req.words[2, 0, :4].tolist() == [7, 8, 1, -1]
    assert (req.words[1] == -1).all()
    assert cbs.tables([[], []], 10, 6, 64, VOCAB).S == 1
    assert cbs.tables([['w1', 'w2']], 10, 6, 4, VOCAB).words[0, :2, 0].tolist() == [1, 2]      # a bare word is a set of one
    with pytest.raises(ValueError, match=r"'zebra'.*\[1, 10\).*0.*UNK column 9.*'UNK'"):
        cbs.tables([[['zebra', 'w1'], [0], ['UNK']]], 10, 6, 2, VOCAB, unk=9)
    with pytest.raises(ValueError, match='ids outside'):
        cbs.tables([[[10]]], 10, 6, 2, VOCAB)
    assert cbs.tables([[[9]]], 10, 6, 2, VOCAB).words[0, 0, 0] == 9          # UNK is an ordinary column unless it is suppressed
    with pytest.raises(ValueError, match='5 constraints'):
        cbs.tables([[[1], [2], [3], [4], [5]]], 10, 6, 1, VOCAB)
    with pytest.raises(ValueError, match='9 words'):
        cbs.tables([[[1] * 9]], 10, 6, 1, VOCAB)
    with pytest.raises(ValueError, match='empty'):
        cbs.tables([[[]]], 10, 6, 1, VOCAB)
    with pytest.raises(ValueError, match=r'S \* beam_size = 80 > 64'):
        cbs.tables([[[1], [2], [3], [4]]], 10, 6, 5, VOCAB)
    with pytest.raises(ValueError, match='L >= C \\+ 1'):
        cbs.tables([[[1], [2]]], 10, 2, 2, VOCAB)
    assert cbs.wanted({'constraints': []}) and not cbs.wanted({}) and not cbs.wanted(None) and not cbs.wanted({'constraints': None})


@pytest.mark.parametrize('name', FAMILIES + ('ensemble',))
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: every refusal is raised before the device check that a valid call runs into"""
    from imagecaptioning.pytorch_amd._lib import CapmiError
    model = _model(name).eval()
    assert model.last_cbs is None and model._cbs_req is None
    fc, att = torch.zeros(2, 20), torch.zeros(2, 4, 20)

    def call(**opt):
        with torch.no_grad():
            return model(fc, att, None, opt=opt, mode='sample')

    ok = dict(beam_size=2, constraints=[[[3, 4]], []])
    if name == 'ensemble':
        with pytest.raises(NotImplementedError, match='AttEnsemble'):
            call(**ok)
        return
    for key, val in (('block_trigrams', 1), ('group_size', 2), ('output_logsoftmax', 0), ('sample_n', 2)):
        with pytest.raises(NotImplementedError, match=key):
            call(**dict(ok, **{key: val}))
    for method in ('sample', 'gumbel', 'top5', 'sbs'):
        with pytest.raises((NotImplementedError, ValueError), match='sample_method|sample_n'):
            call(**dict(ok, sample_method=method))
    with pytest.raises(NotImplementedError, match='sample_method'):
        call(**dict(ok, sample_method='sample'))
    with pytest.raises(ValueError, match='5 constraints'):
        call(**dict(ok, constraints=[[[1], [2], [3], [4], [5]], []]))
    with pytest.raises(ValueError, match='9 words'):
        call(**dict(ok, constraints=[[[1] * 9], []]))
    with pytest.raises(ValueError, match='> 64'):
        call(**dict(ok, beam_size=9, constraints=[[[1], [2], [3]], []]))
    with pytest.raises(ValueError, match='not in the vocabulary'):
        call(**dict(ok, constraints=[[['no-such-word']], []]))
    with pytest.raises(ValueError, match='ids outside'):
        call(**dict(ok, constraints=[[[0]], []]))
    model.train()
    with pytest.raises(NotImplementedError, match='eval'):
        call(**ok)
    model.eval()
    assert model._cbs_req is None
    # valid options go on to the device check of a CPU tensor, which is no refusal of the option
    for opt in (ok, dict(ok, sample_method='beam_search', sample_n=1), dict(ok, beam_size=1),
                dict(ok, decoding_constraint=1, remove_bad_endings=1, suppress_UNK=1, temperature=0.7, length_penalty='wu_0.5')):
        with pytest.raises((CapmiError, RuntimeError, AssertionError)) as e:
            call(**opt)
        assert not isinstance(e.value, (NotImplementedError, ValueError)), e.value
    assert model.last_cbs is None and model._cbs_req is None


def test_short_captions_and_models_without_a_stepper_refuse():
    from imagecaptioning.pytorch_amd.captioning.models.CaptionModel import CaptionModel
    from imagecaptioning.pytorch_amd import cbs

    class Bare(CaptionModel):
        pass
    with pytest.raises(NotImplementedError, match='single-step decoder'):
        cbs.check_options(Bare().eval(), dict(constraints=[]))
    model = _model('updown').eval()
    model.seq_length = 2
    with pytest.raises(ValueError, match='L >= C'):
        cbs.prepare(model, dict(beam_size=2, constraints=[[[1], [2]]]))


def test_new_entries_in_header_match_the_binding():
    from imagecaptioning.pytorch_amd import _lib, ops, cbs
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'capmi.h')).read(), flags=re.S)
    decl = dict((m.group(1), m.group(2).strip()) for m in
                re.finditer(r'\b(?:int|int64_t|const char \*)\s*(capmi_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    for name, nargs in ENTRIES.items():
        assert len(decl[name].split(',')) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib, name)
    assert _lib.lib.capmi_cbs_scratch_bytes(3, 16, 4, 9488) == 3 * 16 * 10 * 4 * 8 and _lib.lib.capmi_cbs_scratch_bytes(0, 1, 1, 1) == 0
    assert (ops.CBS_C_MAX, ops.CBS_W_MAX, ops.CBS_SLOTS_MAX) == (cbs.C_MAX, cbs.W_MAX, cbs.SLOTS_MAX) == (R.C_MAX, R.W_MAX, 64)
    # the argument checks come before any launch
    assert _lib.lib.capmi_cbs_select(None, None, None, None, 1, 1, 1, 1, 4, 0, None, 0, None, None, None, None, None, None,
                                     None) == _lib.EINVAL
    assert _lib.lib.capmi_cbs_finalize(None, None, None, None, None, None, None, 1, 1, 1, 1, None, None, None, None, None,
                                       None) == _lib.EINVAL
    words, ncons = torch.full((1, 4, 8), -1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for bad_w, bad_n, S in ((words.clone().fill_(0), ncons, 1), (words.clone().fill_(9), ncons, 1), (words, ncons + 2, 2),
                            (words[:, :3], ncons, 1)):
        with pytest.raises(_lib.CapmiError):
            ops.cbs_tables(bad_w, bad_n, 9, S, 'cpu')
    tables = ops.cbs_tables(words, ncons, 9, 1, 'cpu')
    with pytest.raises(_lib.CapmiError):
        ops.cbs_select(torch.zeros(2, 9), torch.zeros(1, 2), tables, 2, 1)   # CPU tensors


def test_command_line(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd'))
    from captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import eval as E
    assert (opts.DEFAULTS['constraints_json'], opts.DEFAULTS['constraints_oov']) == ('', 'error')
    o = opts.parse_opt(['--constraints_json', 'c.json', '--constraints_oov', 'drop'])
    assert (o.constraints_json, o.constraints_oov) == ('c.json', 'drop')
    assert opts.parse_opt([]).constraints_json == ''
    assert 'constraints' not in E.eval_kwargs_of(o)                          # the lists go in per batch, by image id
    assert E.ConstraintSet.load(opts.parse_opt([]), VOCAB) is None
    spec = {'7': [['w1', 'zebra'], ['okapi']], 'b': [['w2']]}
    path = tmp_path / 'c.json'
    path.write_text(json.dumps(spec))
    o = argparse.Namespace(constraints_json=str(path), constraints_oov='error', eval_results_dir=str(tmp_path), id='x')
    with pytest.raises(ValueError, match="'okapi', 'zebra'"):
        E.ConstraintSet.load(o, VOCAB)
    o.constraints_oov = 'nope'
    with pytest.raises(ValueError, match='constraints_oov'):
        E.ConstraintSet.load(o, VOCAB)
    o.constraints_oov = 'drop'
    cons = E.ConstraintSet.load(o, VOCAB)
    assert (cons.dropped_words, cons.dropped_constraints) == (2, 1)
    assert cons.for_batch([{'id': 7}, {'id': 'b'}, {'id': 'c'}]) == [[['w1']], [['w2']], []]
    last = dict(satisfied=torch.tensor([1, 0, 0]), total=torch.tensor([1, 1, 0]))
    sat, total = cons.add_batch(last, [{'id': 7}, {'id': 'b'}, {'id': 'c'}], 3)
    assert (sat, total) == ([1, 0, 0], [1, 1, 0])
    s = cons.summary()
    assert (s['images'], s['constrained_images'], s['fully_satisfied'], s['mean_satisfied_fraction']) == (3, 2, 0.5, 0.5)
    written = json.load(open(cons.write(o, 'val')))
    assert os.path.basename(cons.write(o, 'val')) == 'x_val_cbs.json' and written['overall'] == s and len(written['images']) == 3
