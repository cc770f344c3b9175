"""The logits processors (no_repeat_ngram_size, repetition_penalty, min_length, bad_words; imagecaptioning/pytorch_amd/logits_proc.py)
without a GPU: the restatement of tests/logits_proc_ref.py on cases whose answer is written out here, the ABI, every refusal, the
defaults and the command line."""
import argparse
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import logits_proc_ref as R
from test_att_trace_host import tiny_opt

V1, L = 10, 6
INF = float('inf')


def _row():
    return -np.arange(1, V1 + 1, dtype=np.float32)            # row[v] = -(v + 1)


def _blocked(out):
    return set(np.nonzero(np.isneginf(out))[0].tolist())


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_bigram_blocking_blocks_what_followed_the_last_word():
    # history 5 7 5: the last word is 5, and 5 was followed by 7 -> 7 is blocked, nothing else
    out = R.process(_row(), [5, 7, 5], 3, L, dict(no_repeat_ngram_size=2))
    assert _blocked(out) == {7}
    keep = [v for v in range(V1) if v != 7]
    assert np.array_equal(out[keep], _row()[keep])
    # history 5 7: the last word 7 was followed by nothing yet
    assert _blocked(R.process(_row(), [5, 7], 2, L, dict(no_repeat_ngram_size=2))) == set()


def test_unigram_blocking_blocks_every_emitted_word():
    assert _blocked(R.process(_row(), [5, 7, 5], 3, L, dict(no_repeat_ngram_size=1))) == {5, 7}
    assert _blocked(R.process(_row(), [], 0, L, dict(no_repeat_ngram_size=1))) == set()


def test_trigram_blocking_is_inactive_before_step_n_minus_1():
    assert _blocked(R.process(_row(), [5], 1, L, dict(no_repeat_ngram_size=3))) == set()
    assert _blocked(R.process(_row(), [5, 7, 2, 5, 7], 5, L, dict(no_repeat_ngram_size=3))) == {2}


def test_penalty_is_applied_once_for_a_word_seen_three_times():
    out = R.process(_row(), [4, 4, 2, 4], 4, L, dict(repetition_penalty=1.5))
    want = _row()
    want[4] = np.float32(-5.0) * np.float32(1.5)              # -7.5, not -5 * 1.5^3
    want[2] = np.float32(-3.0) * np.float32(1.5)
    assert np.array_equal(out, want) and out[4] == np.float32(-7.5)


def test_min_length_is_clipped_at_the_last_step():
    # L = 6: the end token must stay reachable at t = 5 whatever min_length says
    for t in range(L):
        out = R.process(_row(), [3] * t, t, L, dict(min_length=100))
        assert _blocked(out) == ({0} if t < L - 1 else set()), t
    assert _blocked(R.process(_row(), [3, 3], 2, L, dict(min_length=2))) == set()
    assert _blocked(R.process(_row(), [3], 1, L, dict(min_length=2))) == {0}


def test_a_two_word_bad_sequence_fires_only_after_its_first_word():
    opts = dict(bad_words=[[6, 8]])
    assert _blocked(R.process(_row(), [2, 6], 2, L, opts)) == {8}
    assert _blocked(R.process(_row(), [6, 2], 2, L, opts)) == set()
    assert _blocked(R.process(_row(), [], 0, L, opts)) == set()
    assert _blocked(R.process(_row(), [], 0, L, dict(bad_words=[[9]]))) == {9}           # a one-word entry: always
    assert _blocked(R.process(_row(), [1, 2, 3], 3, L, dict(bad_words=[[1, 2, 3, 4], [2, 3, 5]]))) == {4, 5}


def test_eos_is_never_blocked_by_ngrams_the_penalty_or_bad_words():
    # no processed history holds 0 (such a row is finished), so column 0 can only be hit by min_length
    opts = dict(no_repeat_ngram_size=1, repetition_penalty=2.0, bad_words=[[3], [5, 7]])
    out = R.process(_row(), [5, 7, 5], 3, L, opts)
    assert out[0] == np.float32(-1.0) and _blocked(out) == {3, 5, 7}


def test_a_finished_row_is_untouched():
    opts = dict(no_repeat_ngram_size=1, repetition_penalty=2.0, min_length=5, bad_words=[[3]])
    assert np.array_equal(R.process(_row(), [5, 0, 0], 3, L, opts), _row())


def test_a_penalised_and_blocked_word_ends_blocked_and_exempt_words_are_spared():
    out = R.process(_row(), [5, 7, 5], 3, L, dict(no_repeat_ngram_size=2, repetition_penalty=1.25))
    assert np.isneginf(out[7]) and out[5] == np.float32(-6.0) * np.float32(1.25)
    assert _blocked(R.process(_row(), [5, 7, 5], 3, L, dict(no_repeat_ngram_size=2), exempt=(7,))) == set()


def test_history_from_parents_follows_the_parents():
    # 1 image, W = 2, 3 steps.  step 0: slots (3, 4) from the root; step 1: slot 0 = (4 ->) 5, slot 1 = (3 ->) 6; step 2: slot 0
    # continues slot 1
    tokens = np.array([[[3, 4]], [[5, 6]], [[7, 8]]])
    parents = np.array([[[0, 0]], [[1, 0]], [[1, 1]]])
    assert R.history_from_parents(tokens, parents, 0, 0) == []
    assert R.history_from_parents(tokens, parents, 1, 1) == [4]
    assert R.history_from_parents(tokens, parents, 2, 0) == [4, 5]
    assert R.history_from_parents(tokens, parents, 2, 1) == [3, 6]
    assert R.history_from_parents(tokens, parents, 3, 0) == [3, 6, 7]


# ------------------------------------------------------------------------------------------------ the ABI
def test_ctypes_struct_and_prototype_match_the_header():
    from imagecaptioning.pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'capmi.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    kinds = {'int': C.c_int, 'float': C.c_float, 'int64_t': C.c_int64}
    args = re.search(r'int capmi_logits_process\((.*?)\);', hdr, re.S).group(1)
    want = [C.c_void_p if '*' in a else kinds[a.split()[-2]] for a in (x.strip() for x in args.replace('\n', ' ').split(','))]
    got = [C.c_void_p if (isinstance(a, type) and issubclass(a, C._Pointer)) else a for a in _lib.SIGNATURES['capmi_logits_process']]
    assert got == want
    body = re.search(r'typedef struct \{([^{}]*?)\} capmi_logits_proc;', hdr, re.S).group(1)
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (CAPMI_LP_\w+) (\d+)', hdr)}
    fields = []
    for stmt in (s.strip() for s in body.split(';')):
        if stmt:
            m = re.match(r'(int|float)\s+(\w+)(?:\[(\w+)\])?$', stmt)
            base = kinds[m.group(1)]
            fields.append((m.group(2), base if m.group(3) is None else base * macros[m.group(3)]))
    assert [(n, C.sizeof(t)) for n, t in fields] == [(n, C.sizeof(t)) for n, t in _lib.LogitsProc._fields_]
    assert [n for n, _ in fields] == [n for n, _ in _lib.LogitsProc._fields_]
    assert (macros['CAPMI_LP_HIST_MAX'], macros['CAPMI_LP_NGRAM_MAX'], macros['CAPMI_LP_BAD_MAX'], macros['CAPMI_LP_BAD_LEN']) == \
        (_lib.LP_HIST_MAX, _lib.LP_NGRAM_MAX, _lib.LP_BAD_MAX, _lib.LP_BAD_LEN) == (64, 8, 16, 4)
    assert macros['CAPMI_LP_BAD_IDS'] == 64


def test_struct_is_filled_row_by_row():
    from imagecaptioning.pytorch_amd import logits_proc as LP
    p = LP.struct(*LP.params(dict(no_repeat_ngram_size=3, repetition_penalty=1.2, min_length=4, bad_words=[[7], [1, 2, 3, 4], 9])))
    assert (p.no_repeat_ngram_size, p.min_length, p.n_bad) == (3, 4, 3) and p.repetition_penalty == np.float32(1.2)
    assert list(p.bad_len)[:4] == [1, 4, 1, 0] and list(p.bad_words)[:12] == [7, 0, 0, 0, 1, 2, 3, 4, 9, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ refusals
def _model(name='updown'):
    from imagecaptioning.pytorch_amd.captioning import models
    return models.setup(tiny_opt(name)).eval()


FC, ATT = torch.zeros(2, 20), torch.zeros(2, 3, 20)


def _call(model, **opt):
    return model(FC, ATT, None, opt=opt, mode='sample')


BAD_VALUES = [dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True),
              dict(repetition_penalty=0.9), dict(repetition_penalty=float('nan')), dict(repetition_penalty='x'),
              dict(min_length=-1), dict(min_length=1.5),
              dict(bad_words=[[1]] * 17), dict(bad_words=[[1, 2, 3, 4, 5]]), dict(bad_words=[[3, 0]]), dict(bad_words=[[0]]),
              dict(bad_words=[[]]), dict(bad_words=[[-2]]), dict(bad_words=[['man']]), dict(bad_words='man')]


@pytest.mark.parametrize('bad', BAD_VALUES, ids=[repr(b)[:40] for b in BAD_VALUES])
def test_range_checks_raise_value_errors_before_any_device_work(bad):
    from imagecaptioning.pytorch_amd import logits_proc as LP
    with pytest.raises(ValueError, match=list(bad)[0]):
        LP.params(bad)
    with pytest.raises(ValueError, match=list(bad)[0]):
        _call(_model(), **bad)                                 # CPU tensors: a call that got further would fail in the device check


def test_the_limits_themselves_are_accepted():
    from imagecaptioning.pytorch_amd import logits_proc as LP
    assert LP.params(dict(no_repeat_ngram_size=8, repetition_penalty=1, min_length=0, bad_words=[[1, 2, 3, 4]] * 16)) == \
        (8, 1.0, 0, [[1, 2, 3, 4]] * 16)
    assert LP.params({}) == (0, 1.0, 0, [])


ON = [dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.2), dict(min_length=3), dict(bad_words=[[4]])]


@pytest.mark.parametrize('on', ON, ids=[list(o)[0] for o in ON])
@pytest.mark.parametrize('name', ('updown', 'transformer'))
def test_refusals_come_before_any_device_work(name, on):
    from imagecaptioning.pytorch_amd._lib import CapmiError
    model = _model(name)
    model.train()
    with pytest.raises(NotImplementedError, match='test-time options'):
        with torch.no_grad():
            _call(model, **on)
    with pytest.raises(NotImplementedError, match='train_beam_size > 1'):
        _call(model, beam_size=2, **on)                       # train mode, gradients enabled: the training beam search
    model.eval()
    with pytest.raises(NotImplementedError, match='output_logsoftmax=0'):
        _call(model, output_logsoftmax=0, **on)
    with pytest.raises(NotImplementedError, match='group_size > 1'):
        _call(model, group_size=2, **on)
    with pytest.raises(NotImplementedError, match='group_size > 1'):
        _call(model, group_size=2, beam_size=4, **on)
    with pytest.raises(NotImplementedError, match="'contrastive'.*different kernel"):
        _call(model, sample_method='contrastive', **on)
    with pytest.raises(NotImplementedError, match="mode='score'.*not edited"):
        model(FC, ATT, torch.zeros(2, 1, 5, dtype=torch.long), None, mode='score', opt=dict(on))
    # past every refusal: the device check
    for more in (dict(), dict(beam_size=2), dict(sample_method='sbs', sample_n=2), dict(sample_method='top3'),
                 dict(constraints=[[['w1']], [['w2']]], beam_size=2)):
        with pytest.raises(CapmiError, match='HIP device'):
            _call(model, **more, **on)


def test_the_older_refusals_of_block_trigrams_stand():
    model = _model()
    with pytest.raises(NotImplementedError, match='block_trigrams'):
        _call(model, sample_method='sbs', sample_n=2, block_trigrams=1, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError, match='block_trigrams'):
        _call(model, constraints=[[['w1']], [['w2']]], beam_size=2, block_trigrams=1, no_repeat_ngram_size=2)


def test_ensemble_refuses_train_mode_and_takes_the_options():
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    ens = AttEnsemble([_model('updown'), _model('att2in2')])
    ens.train()
    with pytest.raises(NotImplementedError, match='test-time options'):
        with torch.no_grad():
            _call(ens, no_repeat_ngram_size=2)
    ens.eval()
    with pytest.raises(ValueError, match='no_repeat_ngram_size'):
        with torch.no_grad():
            _call(ens, no_repeat_ngram_size=9)


def test_a_caption_longer_than_the_history_buffer_is_refused():
    model = _model()
    model.seq_length = 65
    with pytest.raises(ValueError, match='seq_length = 65'):
        _call(model, no_repeat_ngram_size=2)


# ------------------------------------------------------------------------------------------------ defaults
def test_defaults_do_not_ask_for_the_stepped_sampler():
    from imagecaptioning.pytorch_amd import decode, logits_proc as LP
    assert not decode.wants_options({}) and not LP.wanted({}) and not LP.wanted(None)
    for k, v in (('no_repeat_ngram_size', 0), ('repetition_penalty', 1.0), ('repetition_penalty', 1), ('min_length', 0),
                 ('bad_words', None), ('bad_words', [])):
        assert not decode.wants_options({k: v}) and not LP.wanted({k: v}), (k, v)
        assert LP.make({k: v}, 16) is None
    assert not decode.wants_options(dict(no_repeat_ngram_size=0, repetition_penalty=1.0, min_length=0, bad_words=None))
    for on in ON:
        assert decode.wants_options(on) and LP.wanted(on)


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_and_defaults(tmp_path):
    from imagecaptioning.pytorch_amd import logits_proc as LP
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import eval as E, eval_ensemble as EE
    d = opts.DEFAULTS
    assert (d['no_repeat_ngram_size'], d['repetition_penalty'], d['min_length'], d['bad_words_json'], d['block_trigrams']) == (0, 1.0, 0, '', 0)
    kw = E.eval_kwargs_of(opts.parse_opt([]))
    assert (kw['no_repeat_ngram_size'], kw['repetition_penalty'], kw['min_length'], kw['bad_words']) == (0, 1.0, 0, [])
    assert not LP.wanted(kw)
    o = opts.parse_opt(['--no_repeat_ngram_size', '3', '--repetition_penalty', '1.2', '--min_length', '4', '--bad_words_json', 'f.json'])
    kw = E.eval_kwargs_of(o)
    assert (kw['no_repeat_ngram_size'], kw['repetition_penalty'], kw['min_length'], o.bad_words_json) == (3, 1.2, 4, 'f.json')
    assert opts.parse_opt(['--bad_words', 'a man', 'top']).bad_words == ['a man', 'top']
    assert LP.bad_word_ids(['a man', 'top', [2, 1]], {'1': 'a', '2': 'man', '3': 'top'}) == [[1, 2], [3], [2, 1]]
    assert set(LP.KEYS) <= set(E.SAMPLE_KEYS)
    assert {'no_repeat_ngram_size', 'repetition_penalty', 'min_length', 'bad_words_json'} <= set(EE.EVAL_KEYS)
    _, _, _, explicit = EE.parse_args(['--ids', 'a', 'b', '--no_repeat_ngram_size', '2'])
    opt = EE.build_opt({'opt': argparse.Namespace(caption_model='updown', no_repeat_ngram_size=5, min_length=7)}, explicit)
    assert (opt.no_repeat_ngram_size, opt.min_length, opt.repetition_penalty) == (2, 0, 1.0)


def test_bad_words_file_goes_through_the_vocabulary(tmp_path):
    from imagecaptioning.pytorch_amd import logits_proc as LP
    vocab = {'1': 'a', '2': 'man', '3': 'on', '4': 'UNK'}
    f = tmp_path / 'bad.json'
    f.write_text(json.dumps(['man', 'a man', ['on', 'a', 'man']]))
    assert LP.bad_words_from_file(str(f), vocab) == [[2], [1, 2], [3, 1, 2]]
    f.write_text(json.dumps(['zebra on', 'man']))
    with pytest.raises(ValueError, match="not in the vocabulary: 'zebra'"):
        LP.bad_words_from_file(str(f), vocab)
    assert LP.bad_words_from_file(str(f), vocab, 'drop') == [[2]]
    f.write_text(json.dumps({'a': 1}))
    with pytest.raises(ValueError, match='JSON list'):
        LP.bad_words_from_file(str(f), vocab)
