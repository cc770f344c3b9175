"""Contrastive search (sample_method 'contrastive', decode.contrastive_steps) without a GPU: every refusal, the command line, the
float64 replay (tests/contrastive_ref64.py) against the real reference's greedy fixture, and a case worked out by hand."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import contrastive_ref64 as R
from test_att_trace_host import tiny_opt


def _model(name='updown'):
    from imagecaptioning.pytorch_amd.captioning import models
    return models.setup(tiny_opt(name)).eval()


FC, ATT = torch.zeros(2, 20), torch.zeros(2, 3, 20)


def _call(model, **opt):
    return model(FC, ATT, None, opt=dict(opt, sample_method='contrastive'), mode='sample')


# ------------------------------------------------------------------------------------------------ refusals (CPU tensors: a call
# that got past them would fail in the device check or in a launch instead)
def test_parse_sample_method_still_has_no_such_sampler_but_the_dispatch_knows_the_name():
    from imagecaptioning.pytorch_amd import decode
    from imagecaptioning.pytorch_amd.captioning.models.utils import parse_sample_method
    with pytest.raises(NotImplementedError):
        parse_sample_method('contrastive', 1.0)
    assert decode.contrastive({'sample_method': 'contrastive'}) and not decode.contrastive({}) and not decode.contrastive(None)
    assert decode.wants_options({'sample_method': 'contrastive'}) and not decode.wants_options({'sample_method': 'greedy'})
    assert decode.contrastive_params({}) == (0.6, 4)
    assert decode.contrastive_params({'penalty_alpha': 0, 'contrastive_k': 32}) == (0.0, 32)


@pytest.mark.parametrize('name', ('updown', 'newfc', 'att2in2', 'adaatt', 'aoa'))
def test_refusals_come_before_any_device_work(name):
    model = _model(name)
    model.train()
    with pytest.raises(NotImplementedError, match='test-time option'):
        _call(model)
    model.eval()
    with pytest.raises(NotImplementedError, match='output_logsoftmax=0'):
        _call(model, output_logsoftmax=0)
    with pytest.raises(ValueError, match='deterministic.*identical'):
        _call(model, sample_n=3)
    with pytest.raises(ValueError, match='beam_size must be 1'):
        _call(model, beam_size=2)
    with pytest.raises(ValueError, match='group_size must be 1'):
        _call(model, group_size=2)
    for alpha in (-0.01, 1.01, float('nan'), 'x', None):
        with pytest.raises(ValueError, match='penalty_alpha'):
            _call(model, penalty_alpha=alpha)
    for k in (0, 33, -1, 2.5, None):
        with pytest.raises(ValueError, match='contrastive_k'):
            _call(model, contrastive_k=k)
    with pytest.raises(ValueError, match="model's own probabilities"):
        _call(model, temperature=0.7)
    with pytest.raises(NotImplementedError, match='distractors'):
        _call(model, distractors=torch.zeros(2, 1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match='constraints'):
        _call(model, constraints=[[['w1']], [['w2']]])
    with pytest.raises(NotImplementedError, match='return_attention.*one row per caption per step'):
        _call(model, return_attention=1)
    # past every refusal: the device check (a CapmiError, not one of the above)
    from imagecaptioning.pytorch_amd._lib import CapmiError
    with pytest.raises(CapmiError, match='HIP device'):
        _call(model, penalty_alpha=0.6, contrastive_k=4)


@pytest.mark.parametrize('name,kw', (('transformer', {}), ('aoa', dict(out_res=1)), ('aoa', dict(out_res=1, decoder_type='LSTM'))))
def test_decoders_without_a_kept_pre_logit_row_refuse_by_name(name, kw):
    """the Transformer's final LayerNorm row is a per-step temporary; AoA with out_res 1 forms the logit operand inside the GEMM --
    refused per model, every other AoA variant decodes (test_refusals_come_before_any_device_work reaches the device check)"""
    from imagecaptioning.pytorch_amd.captioning import models
    model = models.setup(tiny_opt(name, **kw)).eval()
    assert model._contrastive_refusal
    assert name != 'aoa' or (type(model)._contrastive_refusal is None and _model('aoa')._contrastive_refusal is None)
    with pytest.raises(NotImplementedError, match="'contrastive' is not implemented for %s" % type(model).__name__):
        _call(model)


def test_ensemble_refuses():
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    ens = AttEnsemble([_model('updown'), _model('att2in2')]).eval()
    with pytest.raises(NotImplementedError, match='AttEnsemble: a mixture has no single hidden state'):
        with torch.no_grad():
            _call(ens)


def test_train_sample_method_is_refused():
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    with pytest.raises(NotImplementedError, match="train_sample_method 'contrastive'"):
        LossWrapper(_model(), synthetic.updown_opt(train_sample_method='contrastive'))
    LossWrapper(_model(), synthetic.updown_opt(train_sample_method='sample'))


def test_sample_n_method_is_refused_where_it_is_parsed():
    from imagecaptioning.pytorch_amd.tools import eval as E
    ns = argparse.Namespace
    for method in ('contrastive',):
        with pytest.raises(ValueError, match='sample_n_method.*deterministic'):
            E.rerank_kwargs(ns(rerank='mbr_ciderd', rerank_prior='uniform', sample_n=4, sample_n_method=method))
        with pytest.raises(ValueError, match='sample_n_method.*deterministic'):
            E.eval_split_n(None, [], FC, ATT, None, {}, ns(sample_n=4, sample_n_method=method, beam_size=1))


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_and_defaults():
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import eval as E, eval_ensemble as EE
    assert opts.DEFAULTS['penalty_alpha'] == 0.6 and opts.DEFAULTS['contrastive_k'] == 4
    o = opts.parse_opt(['--sample_method', 'contrastive'])
    kw = E.eval_kwargs_of(o)
    assert (kw['sample_method'], kw['penalty_alpha'], kw['contrastive_k'], kw['beam_size']) == ('contrastive', 0.6, 4, 1)
    o = opts.parse_opt(['--sample_method', 'contrastive', '--penalty_alpha', '0.35', '--contrastive_k', '7'])
    kw = E.eval_kwargs_of(o)
    assert kw['penalty_alpha'] == 0.35 and kw['contrastive_k'] == 7 and isinstance(kw['contrastive_k'], int)
    # the ensemble tool takes the flags from the command line, never from a member's training run, and hands them on
    assert {'penalty_alpha', 'contrastive_k'} <= set(EE.EVAL_KEYS)
    _, _, _, explicit = EE.parse_args(['--ids', 'a', 'b', '--sample_method', 'contrastive', '--contrastive_k', '3'])
    opt = EE.build_opt({'opt': argparse.Namespace(caption_model='updown', contrastive_k=9, penalty_alpha=0.9)}, explicit)
    assert (opt.sample_method, opt.contrastive_k, opt.penalty_alpha) == ('contrastive', 3, 0.6)
    assert E.eval_kwargs_of(opt)['contrastive_k'] == 3


def test_ctypes_prototypes_match_the_header():
    import ctypes as C
    from imagecaptioning.pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'capmi.h')).read()
    kinds = {'int': C.c_int, 'float': C.c_float, 'int64_t': C.c_int64}
    for name in ('capmi_contrastive_topk', 'capmi_contrastive_select'):
        args = re.search(r'int %s\((.*?)\);' % name, hdr, re.S).group(1)
        want = [C.c_void_p if '*' in a else kinds[a.split()[-2]] for a in (x.strip() for x in args.replace('\n', ' ').split(','))]
        assert _lib.SIGNATURES[name] == want, name
    assert int(re.search(r'#define CAPMI_CONTRASTIVE_KMAX (\d+)', hdr).group(1)) == _lib.CONTRASTIVE_KMAX == 32


# ------------------------------------------------------------------------------------------------ the replay
def _att2in2():
    z = np.load(os.path.join(GOLDEN, 'att2in2_tiny.npz'))
    P = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('P.')}
    t = lambda k: torch.from_numpy(z[k])           # noqa: E731
    return z, P, t


@pytest.mark.parametrize('k,alpha', [(4, 0.0), (1, 0.6), (1, 0.0), (31, 0.0)])
def test_replay_without_a_penalty_or_a_choice_is_the_references_greedy_decode(k, alpha):
    """alpha = 0 (the score is the probability) and k = 1 (one candidate) on the float64 step of tests/att2in2_ref64.py reproduce
    greedy_seq of the real reference's fixture: the replay's stepping, reordering and finished-row handling are the reference's"""
    z, P, t = _att2in2()
    step, state, N = R.family_step('att2in2', P, t('fc'), t('att'), t('att_masks'))
    L, V1 = z['greedy_seq'].shape[1], z['greedy_logp'].shape[2]
    out = R.search(step, state, N, V1, L, k, alpha)
    assert np.array_equal(out['seq'].numpy(), z['greedy_seq'])
    assert bool((out['choice'] == 0).all())
    live = out['was_unfinished'].numpy()
    got = (out['lps'] * out['was_unfinished'].unsqueeze(2)).numpy()
    ref = z['greedy_logp']
    steps = live.any(0)                           # the reference leaves its loop once every row has finished
    np.testing.assert_allclose(got[:, steps], ref[:, steps], rtol=2e-5, atol=5e-6)


def test_replay_differs_from_greedy_under_a_penalty():
    """the other direction: with a penalty the same replay leaves the greedy caption somewhere (else the tests above say nothing)"""
    z, P, t = _att2in2()
    step, state, N = R.family_step('att2in2', P, t('fc'), t('att'), t('att_masks'))
    out = R.search(step, state, N, z['greedy_logp'].shape[2], z['greedy_seq'].shape[1], 4, 0.9)
    assert not np.array_equal(out['seq'].numpy(), z['greedy_seq']) and bool((out['choice'] > 0).any())


def _toy_step(it, state):
    """A 2-row toy decoder over V1 = 4 whose hidden state is a fixed unit vector per input token: token 1 -> e0 (BOS gives e0 too),
    token 2 -> e1, token 3 -> (e0 + e1) / sqrt 2.  The logits do not depend on the state: p = (0.05, 0.5, 0.3, 0.15) after BOS."""
    E = torch.tensor([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [2 ** -0.5, 2 ** -0.5]], dtype=R.F64)
    logits = torch.tensor([0.05, 0.5, 0.3, 0.15], dtype=R.F64).log().repeat(it.shape[0], 1)
    return logits, E[it], state


def test_a_repeated_hidden_state_loses_to_the_runner_up_by_hand():
    """Row 0 and row 1 alike (2 rows).  After BOS the history is {e0}.  k = 2 candidates: token 1 (p 0.5, hidden e0: cosine 1 with the
    history) and token 2 (p 0.3, hidden e1: cosine 0).
      alpha 0.6: score(1) = 0.4 * 0.5 - 0.6 * 1 = -0.4, score(2) = 0.4 * 0.3 - 0 = 0.12  -> token 2
      alpha 0.1: score(1) = 0.9 * 0.5 - 0.1 * 1 = 0.35, score(2) = 0.9 * 0.3 - 0 = 0.27  -> token 1
    Step 2 at alpha 0.6, history {e0, e1}: token 1 scores 0.2 - 0.6 = -0.4 and token 2 scores 0.12 - 0.6 = -0.48 -> token 1."""
    state = (torch.zeros(2, 1, dtype=R.F64),)
    hi = R.search(_toy_step, state, 2, 4, 2, 2, 0.6)
    lo = R.search(_toy_step, state, 2, 4, 2, 2, 0.1)
    assert hi['seq'].tolist() == [[2, 1], [2, 1]] and hi['choice'].tolist() == [[1, 0], [1, 0]]
    assert lo['seq'].tolist() == [[1, 1], [1, 1]] and lo['choice'].tolist() == [[0, 0], [0, 0]]
    assert abs(hi['score_gap'] - 0.08) < 1e-12 and abs(lo['score_gap'] - 0.08) < 1e-12     # 0.12 + 0.4 = 0.52, then 0.08; 0.08 twice
    assert abs(hi['topk_gap'] - np.log(0.3 / 0.15)) < 1e-12
    # the one-launch restatement agrees on the first step
    tok = np.array([[1, 2], [1, 2]])
    lp = np.log(np.array([[0.5, 0.3], [0.5, 0.3]]))
    g = np.array([[[1.0, 0.0], [0.0, 1.0]]] * 2)
    hist = np.array([[[1.0, 0.0]]] * 2)
    one = R.select(tok, lp, g, hist, 0.6, np.array([True, False]))
    assert one['choice'].tolist() == [1, 1] and one['parent'].tolist() == [1, 3] and one['token'].tolist() == [2, 0]
    assert one['unfinished'].tolist() == [True, False] and np.allclose(one['gap'], 0.52) and np.allclose(one['inv'], 1.0)


def test_candidates_at_minus_infinity_and_zero_vectors():
    tok = np.array([[3, 1, 2], [3, 1, 2]])
    lp = np.array([[np.log(0.4), -np.inf, -np.inf], [-np.inf, -np.inf, -np.inf]])
    g = np.zeros((2, 3, 2))
    g[:, 1] = [1.0, 0.0]
    hist = np.array([[[1.0, 0.0]]] * 2)
    one = R.select(tok, lp, g, hist, 1.0, np.array([True, True]))
    # row 0: candidate 0 is a zero vector (cosine 0, score -0), the others are -inf; row 1: all -inf -> candidate 0
    assert one['choice'].tolist() == [0, 0] and one['token'].tolist() == [3, 3]
    assert one['score'][0, 0] == 0.0 and np.isneginf(one['score'][0, 1:]).all() and np.isinf(one['inv']).all()
