"""The float64 restatement of the BLEU-4 and self-CIDEr rewards (tests/rewards_ref64.py) against hand-derived known answers, the
call-site arithmetic against tests/golden/reward_mix.npz (recorded from the reference's own rewards.py / losses.py with the three
scorer objects stubbed, tests/golden/make_reward_mix.py), and the refusal of self_cider_reward_weight outside
new_self_critical.  CPU only."""
import argparse
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import rewards_ref64 as W

TINY, SMALL = 1e-15, 1e-9


def _z():
    return np.load(os.path.join(GOLDEN, 'reward_mix.npz'))


def _bleu_of(guess, correct, testlen, reflen):
    b = 1.0
    for g, c in zip(guess, correct):
        b *= (c + TINY) / (g + SMALL)
    b **= 0.25
    ratio = (testlen + TINY) / (reflen + SMALL)
    return b * math.exp(1 - 1 / ratio) if ratio < 1 else b


def test_host_constants_match_the_header():
    from imagecaptioning.pytorch_amd import _lib
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'capmi.h')).read()
    assert int(re.search(r'#define CAPMI_CIDERD_COOKED_BYTES (\d+)', src).group(1)) == _lib.CIDERD_COOKED_BYTES == DeviceCiderD.COOKED_BYTES
    assert int(re.search(r'#define CAPMI_SELF_CIDER_NMAX (\d+)', src).group(1)) == _lib.SELF_CIDER_NMAX == DeviceCiderD.SELF_CIDER_NMAX


def test_tokens_keep_the_first_zero():
    assert W.tokens_of([3, 4, 0, 0, 7]) == [3, 4, 0]
    assert W.tokens_of([0, 5, 5]) == [0]
    assert W.tokens_of([3, 4, 5]) == [3, 4, 5]                     # no 0: the whole row


def test_hypothesis_equal_to_its_only_reference_scores_one():
    row = [5, 6, 7, 8, 0, 0]                                       # five words, the 0 among them
    assert W.bleu_stats(row, [row]) == ([5, 4, 3, 2], [5, 4, 3, 2], 5, 5)
    b = W.bleu4(row, [row])
    assert b == pytest.approx(_bleu_of([5, 4, 3, 2], [5, 4, 3, 2], 5, 5), rel=1e-15)
    assert 0 < 1 - b < 1e-9                                        # 1 up to tiny / small


def test_eos_at_step_zero_is_one_word():
    hyp, ref = [0, 3, 4, 5], [3, 4, 5, 0]
    assert W.bleu_stats(hyp, [ref]) == ([1, 0, 0, 0], [1, 0, 0, 0], 1, 4)     # the unigram (0,) matches the reference's 0
    want = ((1 + TINY) / (1 + SMALL) * (TINY / SMALL) ** 3) ** 0.25 * math.exp(1 - 1 / ((1 + TINY) / (4 + SMALL)))
    assert W.bleu4(hyp, [ref]) == pytest.approx(want, rel=1e-14)


def test_repeated_unigram_is_clipped_by_the_reference_maximum():
    hyp = [7, 7, 7, 0]
    refs = [[7, 1, 2, 0], [7, 7, 1, 0]]                            # at most two 7s in one reference, one (7, 7)
    guess, correct, tl, rl = W.bleu_stats(hyp, refs)
    assert guess == [4, 3, 2, 1] and correct == [2 + 1, 1, 0, 0] and (tl, rl) == (4, 4)
    assert W.bleu4(hyp, refs) == pytest.approx(_bleu_of(guess, correct, 4, 4), rel=1e-14)


def test_brevity_penalty():
    hyp, ref = [3, 4, 0, 0, 0, 0], [3, 4, 5, 6, 7, 0]
    guess, correct, tl, rl = W.bleu_stats(hyp, [ref])
    assert (tl, rl) == (3, 6) and correct == [3, 1, 0, 0]          # 3, 4 and the 0; (3, 4); nothing longer
    want = _bleu_of(guess, correct, 3, 6)
    assert W.bleu4(hyp, [ref]) == pytest.approx(want, rel=1e-14)
    assert want == pytest.approx(_bleu_of(guess, correct, 3, 3) * math.exp(1 - (6 + SMALL) / (3 + TINY)), rel=1e-12)


def test_closest_length_tie_goes_to_the_shorter_reference():
    hyp = [3, 4, 5, 0]                                              # four words; references of three and five
    refs = [[3, 4, 5, 6, 0], [3, 4, 0, 0, 0]]
    assert W.bleu_stats(hyp, refs)[2:] == (4, 3)
    assert W.bleu_stats(hyp, refs[::-1])[2:] == (4, 3)
    assert W.bleu4(hyp, refs) == pytest.approx(_bleu_of(*W.bleu_stats(hyp, refs)), rel=1e-14)      # ratio > 1: no penalty


@pytest.mark.parametrize('n', [2, 5])
def test_self_cider_of_identical_captions_is_zero(n):
    df = {(3,): 2.0, (4,): 1.0}
    K, eig, s = W.self_cider_parts([[3, 4, 5, 6, 0]] * n, df, 40)
    np.testing.assert_allclose(K, 10.0, rtol=1e-14)
    assert abs(s) <= n * np.sqrt(64 * n * n * 2.0 ** -52) / (np.sqrt(n) * np.log(n))
    assert W.self_cider_scores([[3, 4, 5, 6, 0]] * (2 * n), n, df, 40).shape == (2,)


@pytest.mark.parametrize('n', [2, 5])
def test_self_cider_of_captions_sharing_no_ngram_is_one(n):
    group = [[10 * i + 1, 10 * i + 2, 10 * i + 3, 10 * i + 4] for i in range(n)]     # no 0: not even the EOS word is shared
    K, eig, s = W.self_cider_parts(group, {}, 40)
    np.testing.assert_allclose(K, 10.0 * np.eye(n), rtol=1e-14, atol=0)
    assert s == pytest.approx(1.0, rel=1e-14)


def test_self_cider_without_any_weight_is_zero_not_nan():
    # every n-gram occurs in every image: log(ref_len) - log(df) = 0
    group = [[3, 0], [3, 0]]
    df = {(3,): 40.0, (0,): 40.0, (3, 0): 40.0}
    K, eig, s = W.self_cider_parts(group, df, 40)
    assert not K.any() and s == 0.0


@pytest.mark.parametrize('i', [0, 1, 2])
def test_restated_mix_is_the_references_call_site(i):
    z = _z()
    B, L = int(z['B']), z['seq'].shape[1]
    N = z['seq'].shape[0]
    cw, bw = z['pairs'][i]
    np.testing.assert_array_equal(z['calls_%d' % i], [2 * (cw > 0), 2 * (bw > 0)])      # a weight of 0 skips that scorer
    np.testing.assert_allclose(W.self_critical_reward(cw, bw, z['cider'], z['bleu'], B, L), z['reward_%d' % i], rtol=0, atol=1e-15)
    np.testing.assert_allclose(W.mix(cw, bw, z['cider'][:N], z['bleu'][:N]), z['scores_%d' % i], rtol=0, atol=1e-15)


def _struct_opt(z, lt='new_self_critical'):
    cw, bw, sw = z['struct_weights']
    return argparse.Namespace(structure_loss_type=lt, train_sample_n=int(z['n']), entropy_reward_weight=0,
                              self_cider_reward_weight=float(sw), cider_reward_weight=float(cw), bleu_reward_weight=float(bw))


@pytest.mark.parametrize('red', ['mean', 'none'])
def test_restated_structure_loss_is_the_references(red):
    z = _z()
    n = int(z['n'])
    cw, bw, sw = z['struct_weights']
    N = z['seq'].shape[0]
    np.testing.assert_allclose([W.D.self_cider_of(np.linalg.eigvalsh(k / 10)) for k in z['K']], z['self_cider'], rtol=0, atol=1e-12)
    scores = W.mix(cw, bw, z['cider'][:N], z['bleu'][:N])
    np.testing.assert_allclose(scores.reshape(-1, n), z['struct_%s_reward' % red], rtol=1e-6)
    logp = torch.log_softmax(torch.from_numpy(z['logits']).double(), 2)
    sel = logp.gather(2, torch.from_numpy(z['seq']).unsqueeze(2)).squeeze(2).numpy()
    loss = W.nsc_loss(sel, z['seq'], W.nsc_weights(scores, n, z['self_cider'], sw), red)
    np.testing.assert_allclose(loss, z['struct_%s_loss' % red], rtol=2e-6, atol=1e-6)


@pytest.mark.parametrize('red', ['mean', 'none'])
def test_product_structure_loss_on_injected_scores(red, monkeypatch):
    """StructureLosses' host arithmetic (the route of CPU tensors) with the fixture's scorer outputs injected"""
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    z = _z()
    N = z['seq'].shape[0]
    cw, bw, sw = z['struct_weights']
    monkeypatch.setattr(losses, 'get_scores', lambda gts, seq, opt, as_tensor=False: W.mix(cw, bw, z['cider'][:N], z['bleu'][:N]))
    monkeypatch.setattr(losses, 'get_self_cider_scores', lambda gts, seq, opt, as_tensor=False: z['self_cider'].copy())
    x = torch.log_softmax(torch.from_numpy(z['logits']), 2).requires_grad_(True)
    o = losses.StructureLosses(_struct_opt(z))(x, torch.from_numpy(z['seq']), [None] * int(z['B']), reduction=red)
    np.testing.assert_allclose(o['reward'].numpy(), z['struct_%s_reward' % red], rtol=1e-6)
    np.testing.assert_allclose(o['loss'].detach().numpy(), z['struct_%s_loss' % red], rtol=1e-5, atol=1e-6)
    loss = o['loss']
    (loss if red == 'mean' else (loss * torch.linspace(0.5, 1.5, loss.numel()).view_as(loss)).sum()).backward()
    np.testing.assert_allclose(x.grad.numpy(), z['struct_%s_grad' % red], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('lt', ['seqnll', 'risk', 'softmax_margin', 'best_of_n', 'max_margin', 'multi_margin', 'real_softmax_margin'])
def test_self_cider_weight_is_refused_outside_new_self_critical(lt):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    z = _z()
    x = torch.log_softmax(torch.from_numpy(z['logits']), 2)
    with pytest.raises(NotImplementedError, match='self_cider_reward_weight'):
        losses.StructureLosses(_struct_opt(z, lt))(x, torch.from_numpy(z['seq']), [None] * int(z['B']))
