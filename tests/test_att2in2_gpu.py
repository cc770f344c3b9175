"""Att2in2 (caption_model att2in2, configs/a2i2*.yml) on a real MI355X.

* against the real reference's fixture (tests/golden/att2in2_tiny.npz): XE log-probs / loss / gradients, greedy, beam 3,
  train mode with the recorded dropout masks, a RewardCriterion gradient through the sparse route;
* against the fp64 restatement (tests/att2in2_ref64.py, pinned to that fixture on the host) at the a2i2.yml size
  (R = E = A = 512, att_feat 2048, V1 9488, K 36 ragged): XE, SCST with injected Gumbel noise, scheduled sampling;
* the stepper against the one-call rollout, decode options, edge cases and a short tools/train.py run.
"""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import att2in2_ref64 as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')


def opt_(**kw):
    V = kw.pop('V', 30)
    o = argparse.Namespace(caption_model='att2in2', vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1,
                           drop_prob_lm=0.0, seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=12,
                           use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def golden_model(flatten=False, **kw):
    from imagecaptioning.pytorch_amd.captioning import models
    z = np.load(os.path.join(GOLDEN, 'att2in2_tiny.npz'))
    model = models.setup(opt_(**kw))
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('P.')})
    model = model.to(DEV)
    if flatten:
        model.flatten_parameters_()
    t = lambda k: torch.from_numpy(z[k]).to(DEV)           # noqa: E731
    return z, model, t


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def check_grads(model, z, prefix, rtol=5e-4):
    for k, p in model.named_parameters():
        r = z[prefix + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), r, rtol=rtol, atol=1e-6 + 2e-5 * np.abs(r).max(), err_msg=k)


def check_rel(model, P, att, am):
    """every gradient within 1e-3 of the fp64 restatement's, relative to its largest element.  att_embed units whose
    pre-activation is within 1e-4 of zero for some (image, region) are left out of that layer's comparison: there the fp32
    and fp64 ReLU gates may differ (about a dozen units of 512 at this size)."""
    P64 = {k: v.detach() for k, v in P.items()}
    pre = att.double()[:, :int(am.sum(1).max())] @ P64['att_embed.0.weight'].t() + P64['att_embed.0.bias']
    live = am[:, :pre.shape[1]].bool()
    edge = (pre.abs() < 1e-4)[live].any(0)
    assert int(edge.sum()) <= pre.shape[-1] // 20, int(edge.sum())
    keep = ~edge
    for k, p in model.named_parameters():
        a, b = p.grad, P[k].grad
        if k == 'core.attention.alpha_net.bias':     # exactly 0 (the softmax is shift invariant): compare absolutely
            assert float(a.abs().max()) < 1e-6 and float(b.abs().max()) < 1e-9, k
            continue
        if k.startswith('att_embed.'):
            a, b = a[keep], b[keep]
        assert rel(a, b) < 1e-3, k


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize('flatten', [False, True])
def test_golden_xe_logp_loss_and_grads(flatten):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    z, model, t = golden_model(flatten)
    model.train()                  # drop_prob_lm 0: dropout is the identity
    labels, masks = t('labels'), t('masks')
    logp = model(t('fc'), t('att'), labels[..., :-1], t('att_masks'))
    np.testing.assert_allclose(logp.detach().cpu().numpy(), z['xe_logp'], rtol=2e-5, atol=5e-6)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    np.testing.assert_allclose(loss.item(), z['xe_loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, z, 'xe_grad.')


def test_golden_greedy_and_beam3():
    z, model, t = golden_model()
    model.eval()
    with torch.no_grad():
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        assert np.array_equal(seq.cpu().numpy(), z['greedy_seq'])
        np.testing.assert_allclose(slp.cpu().numpy(), z['greedy_logp'], rtol=2e-5, atol=5e-6)
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1},
                         mode='sample')
        assert np.array_equal(seq.cpu().numpy(), z['beam3_seq'])
        np.testing.assert_allclose(slp.cpu().numpy(), z['beam3_logp'], rtol=2e-5, atol=5e-6)


def test_golden_train_mode_with_recorded_dropout_masks():
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    z, model, t = golden_model(drop_prob_lm=0.5)
    T_steps = z['train_logp'].shape[1] - 1
    d_att, d_x, d_o = ref.unpack_drops(z, 'train', T_steps)
    model._drop_masks = dict(drop_att=d_att.to(DEV), drop_xt=d_x.to(DEV), drop_out=d_o.to(DEV))
    model.train()
    labels, masks = t('labels'), t('masks')
    logp = model(t('fc'), t('att'), labels[..., :-1], None)
    np.testing.assert_allclose(logp.detach().cpu().numpy(), z['train_logp'], rtol=2e-5, atol=5e-6)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    np.testing.assert_allclose(loss.item(), z['train_loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, z, 'train_grad.')


def test_golden_reward_criterion_grads_sparse_route():
    from imagecaptioning.pytorch_amd.captioning.modules.losses import RewardCriterion
    z, model, t = golden_model(flatten=True)
    model.eval()
    seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy', 'sample_n': 2}, mode='sample')
    assert np.array_equal(seq.cpu().numpy(), z['rl_seq'])
    loss = RewardCriterion()(slp, seq, t('rl_reward'))
    np.testing.assert_allclose(loss.item(), z['rl_loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, z, 'rl_grad.')


# ---------------------------------------------------------------------------------------------- a2i2.yml size
def full_model(seed=0, drop=0.0):
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(seed)
    o = opt_(V=9487, input_encoding_size=512, rnn_size=512, att_hid_size=512, fc_feat_size=2048, att_feat_size=2048,
             drop_prob_lm=drop, seq_length=16, max_length=20)
    model = models.setup(o)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    return model.to(DEV)


def full_inputs(B=10, K=36, seed=1):
    g = torch.Generator().manual_seed(seed)
    att = torch.randn(B, K, 2048, generator=g).clamp_min(0).to(DEV)
    am = torch.ones(B, K)
    for b in range(B):
        am[b, 10 + (b * 7) % 27:] = 0
    am[3] = 1                                            # one full row: clip_att keeps K = 36
    return torch.zeros(B, 2048, device=DEV), att, am.to(DEV)


def params64(model):
    return {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}


def test_full_size_xe_vs_restatement():
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    model = full_model()
    model.train()
    fc, att, am = full_inputs()
    B, n, T = 10, 5, 16
    g = torch.Generator().manual_seed(2)
    labels = torch.zeros(B, n, T + 2, dtype=torch.long)
    for b in range(B):
        for j in range(n):
            ln = int(torch.randint(5, T, (1,), generator=g))
            labels[b, j, 1:1 + ln] = torch.randint(1, 9488, (ln,), generator=g)
    masks = (labels > 0).float()
    masks[..., :2] = 1
    labels, masks = labels.to(DEV), masks.to(DEV)
    logp = model(fc, att, labels[..., :-1], am)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    model.zero_grad()
    loss.backward()
    P = params64(model)
    logp_r = ref.xe(P, att, am, labels[..., :-1])
    assert float((logp.detach().double() - logp_r.detach()).abs().max()) < 1e-4
    tgt = labels[..., 1:].reshape(B * n, -1)[:, :logp_r.shape[1]]
    m = masks[..., 1:].reshape(B * n, -1)[:, :logp_r.shape[1]].double()
    loss_r = -(logp_r.gather(2, tgt.unsqueeze(2)).squeeze(2) * m).sum() / m.sum()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, att, am)


def test_full_size_scst_sample_and_grads_vs_restatement():
    """SCST rollouts at bs 10 x 5, L = 20: sampled rows with injected Gumbel noise in eval numerics (the rollout's tokens are
    the restatement's arg-max), RewardCriterion loss and every gradient."""
    from imagecaptioning.pytorch_amd.captioning.modules.losses import RewardCriterion
    model = full_model(seed=3)
    model.eval()
    fc, att, am = full_inputs(seed=4)
    B, n, L = 10, 5, 20
    N = B * n
    gum = -torch.log(-torch.log(torch.rand(L, N, 9488, generator=torch.Generator().manual_seed(5)).clamp(1e-10, 1 - 1e-7)))
    gum = gum.to(DEV)
    seq, slp = model(fc, att, am, opt={'sample_method': 'sample', 'sample_n': n, '_gumbel': gum}, mode='sample')
    reward = torch.randn(N, 1, generator=torch.Generator().manual_seed(6)).repeat(1, L).to(DEV)
    loss = RewardCriterion()(slp, seq, reward)
    model.zero_grad()
    loss.backward()
    P = params64(model)
    seq_r, slp_r = ref.rollout(P, att, am, n, L, gumbel=gum)
    assert torch.equal(seq.cpu(), seq_r.cpu()), 'sampled tokens differ'
    assert float((slp.detach().double() - slp_r.detach()).abs().max()) < 1e-4
    sel = slp_r.gather(2, seq_r.unsqueeze(2)).squeeze(2)
    m = torch.cat([torch.ones(N, 1, dtype=ref.D, device=DEV), (seq_r > 0).double()[:, :-1]], 1)
    loss_r = -(sel * reward.double() * m).sum() / m.sum()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, att, am)


def test_full_size_scheduled_sampling_vs_restatement():
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    model = full_model(seed=7)
    model.train()
    fc, att, am = full_inputs(seed=8)
    B, n, T = 10, 5, 16
    N = B * n
    g = torch.Generator().manual_seed(9)
    labels = torch.randint(1, 9488, (B, n, T + 2), generator=g)
    labels[..., 0] = 0
    labels[..., T + 1:] = 0
    labels = labels.to(DEV)
    masks = torch.ones(B, n, T + 2, device=DEV)
    coin = (torch.rand(T + 1, N, generator=g) < 0.25)
    coin[0] = False
    gum = -torch.log(-torch.log(torch.rand(T + 1, N, 9488, generator=g).clamp(1e-10, 1 - 1e-7)))
    model.ss_prob = 0.25
    model._ss_coin, model._ss_gumbel = coin.to(DEV), gum.to(DEV).contiguous()
    logp = model(fc, att, labels[..., :-1], am)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    model.zero_grad()
    loss.backward()
    P = params64(model)
    logp_r = ref.xe(P, att, am, labels[..., :-1], ss_coin=coin.to(DEV), ss_gumbel=gum.to(DEV))
    assert float((logp.detach().double() - logp_r.detach()).abs().max()) < 1e-4
    tgt = labels[..., 1:].reshape(N, -1)
    loss_r = -logp_r.gather(2, tgt.unsqueeze(2)).squeeze(2).mean()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, att, am)


# ---------------------------------------------------------------------------------------------- stepper, options, edges
def test_one_call_greedy_equals_stepper_greedy():
    from imagecaptioning.pytorch_amd import decode
    model = full_model(seed=11)
    model.eval()
    fc, att, am = full_inputs(seed=12)
    with torch.no_grad():
        seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'sample_n': 2}, mode='sample')
        st = model._stepper(att, am)(2)
        seq_s, slp_s = decode.sample_steps(model, st, 10, model.seq_length, {'sample_method': 'greedy', 'sample_n': 2}, DEV)
    assert torch.equal(seq, seq_s)
    assert float((slp - slp_s).abs().max()) < 1e-4


def test_decode_options_run_through_the_stepper():
    z, model, t = golden_model()
    model.eval()
    with torch.no_grad():
        for o in ({'block_trigrams': 1}, {'remove_bad_endings': 1}, {'decoding_constraint': 1}, {'sample_method': 'top3'}):
            seq, slp = model(t('fc'), t('att'), t('att_masks'), opt=dict(o), mode='sample')
            assert seq.shape == (3, 8) and slp.shape == (3, 8, 31) and bool(((seq >= 0) & (seq <= 30)).all())
        model.bad_endings_ix = [29]
        seq, _ = model(t('fc'), t('att'), t('att_masks'), opt={'remove_bad_endings': 1}, mode='sample')
        assert not bool(((seq[:, :-1] == 29) & (seq[:, 1:] == 0)).any())
        seq, _ = model(t('fc'), t('att'), t('att_masks'), opt={'decoding_constraint': 1}, mode='sample')
        assert not bool(((seq[:, 1:] == seq[:, :-1]) & (seq[:, 1:] > 0)).any())


def test_get_logprobs_state_matches_the_rollout():
    z, model, t = golden_model()
    model.eval()
    with torch.no_grad():
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        fc, att, patt, am = model._prepare_feature(t('fc'), t('att'), t('att_masks'))
        state = model.init_hidden(3)
        it = torch.zeros(3, dtype=torch.long, device=DEV)
        for s in range(3):
            logp, state = model.get_logprobs_state(it, fc, att, patt, am, state)
            assert state[0].shape == (1, 3, 16)
            np.testing.assert_allclose(logp[seq[:, s] > 0].cpu().numpy(), slp[:, s][seq[:, s] > 0].cpu().numpy(), rtol=1e-5, atol=1e-5)
            it = seq[:, s].clone()


def test_edge_cases_eos_mixed_lengths_k1_and_full_mask():
    z, model, t = golden_model()
    model.eval()
    P = {k: v.detach().cpu() for k, v in model.named_parameters()}
    with torch.no_grad():
        # immediate EOS for every row, and mixed lengths
        model.logit.bias[0] += 50.0
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        assert int(seq.abs().sum()) == 0 and float(slp[:, 1:].abs().max()) == 0.0
        model.logit.bias[0] -= 50.0
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        seq_r, slp_r = ref.rollout(P, t('att').cpu(), t('att_masks').cpu(), 1, 8)
        assert torch.equal(seq.cpu(), seq_r)
        lens = (seq > 0).sum(1)
        assert int(lens.min()) < int(lens.max())
        np.testing.assert_allclose(slp.cpu().numpy(), slp_r.numpy(), rtol=2e-5, atol=5e-6)
        # K = 1
        att1 = t('att')[:, :1].contiguous()
        seq, slp = model(t('fc'), att1, None, opt={'sample_method': 'greedy'}, mode='sample')
        seq_r, slp_r = ref.rollout(P, att1.cpu(), None, 1, 8)
        assert torch.equal(seq.cpu(), seq_r)
        np.testing.assert_allclose(slp.cpu().numpy(), slp_r.numpy(), rtol=2e-5, atol=5e-6)
        # an all-ones mask equals att_masks=None
        ones = torch.ones(3, 6, device=DEV)
        a = model(t('fc'), t('att'), ones, opt={'sample_method': 'greedy'}, mode='sample')
        b = model(t('fc'), t('att'), None, opt={'sample_method': 'greedy'}, mode='sample')
        assert torch.equal(a[0], b[0])
        assert float((a[1] - b[1]).abs().max()) < 1e-6


def test_tools_train_xe_scst_nsc_with_resume(tmp_path):
    """tools/train.py on synthetic data: XE (the a2i2.yml schedule: scheduled sampling from epoch 0), self-critical after a
    resume, then new_self_critical; losses finite, the XE loss falls over 30 steps."""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import opts, rewards
    small = ['--caption_model', 'att2in2', '--rnn_size', '64', '--input_encoding_size', '64', '--att_hid_size', '32',
             '--fc_feat_size', '48', '--att_feat_size', '48', '--vocab_size', '60', '--synthetic_regions', '7', '--seq_length', '8',
             '--max_length', '8', '--batch_size', '4', '--seq_per_img', '3', '--synthetic_images', '16', '--losses_log_every', '2',
             '--checkpoint_path', str(tmp_path), '--scheduled_sampling_start', '0']
    l0 = T.train(opts.parse_opt(small + ['--max_iters', '1']))
    l1 = T.train(opts.parse_opt(small + ['--max_iters', '30', '--save_checkpoint_every', '30', '--learning_rate', '0.01',
                                         '--reduce_on_plateau', '0']))
    assert np.isfinite(l0) and np.isfinite(l1)
    assert l1 < l0, 'XE loss should fall on a 16-image synthetic set (%.3f -> %.3f)' % (l0, l1)
    rewards.reset_scorer()
    l2 = T.train(opts.parse_opt(small + ['--max_iters', '33', '--self_critical_after', '0', '--train_sample_n', '3',
                                         '--save_checkpoint_every', '33', '--start_from', str(tmp_path)]))
    assert np.isfinite(l2)
    rewards.reset_scorer()
    l3 = T.train(opts.parse_opt(small + ['--max_iters', '36', '--structure_after', '0', '--structure_loss_type', 'new_self_critical',
                                         '--train_sample_n', '3', '--start_from', str(tmp_path)]))
    assert np.isfinite(l3)
