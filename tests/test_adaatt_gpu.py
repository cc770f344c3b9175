"""AdaAtt (caption_model adaatt / adaattmo) on a real MI355X.

* against the real reference's fixture (tests/golden/adaatt_tiny.npz), both variants: XE log-probs / loss / gradients (flat and
  un-flat parameters), greedy, beam 3, train mode with the recorded dropout masks injected, a RewardCriterion gradient through the
  sparse route, scheduled sampling with the recorded inputs;
* the sentinel attention kernels alone against fp64 torch, with the in-kernel Philox tile mask;
* against the fp64 restatement (tests/adaatt_ref64.py, pinned to that fixture on the host) at the a2i2-like size
  (R = E = A = 512, V1 9488, B 10, n 5, K 36 ragged, dropout 0.5 injected): XE, SCST with injected Gumbel noise, scheduled sampling;
* the stepper against the one-call rollout, get_logprobs_state, decode options, edge cases, an AttEnsemble with an Att2in2 member
  and a short tools/train.py + tools/eval.py run.

Tolerances are those of tests/test_att2in2_gpu.py for the same quantities (same arithmetic: bf16x3 split GEMMs, fp32 pointwise).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
import adaatt_ref64 as ref
import att2in2_ref64 as ref_a2
from test_adaatt_host import Fixture, ss_draws, VARIANTS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')


def opt_(name='adaatt', **kw):
    V = kw.pop('V', 30)
    o = argparse.Namespace(caption_model=name, vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1,
                           drop_prob_lm=0.0, seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=16,
                           use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def golden_model(name, flatten=False, **kw):
    from imagecaptioning.pytorch_amd.captioning import models
    fx = Fixture(name)
    model = models.setup(opt_(name, **kw))
    model.load_state_dict(fx.params())
    model = model.to(DEV)
    if flatten:
        model.flatten_parameters_()
    return fx, model, lambda k: fx.t(k).to(DEV)


def check_grads(model, fx, prefix, rtol=5e-4):
    for k, p in model.named_parameters():
        r = fx[prefix + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), r, rtol=rtol, atol=1e-6 + 2e-5 * np.abs(r).max(), err_msg=k)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check_rel(model, P, fc, att, am):
    """every gradient within 1e-3 of the fp64 restatement's, relative to its largest element (the bound test_att2in2_gpu.py
    uses).  fc_embed / att_embed units whose pre-activation is within 1e-4 of zero somewhere are left out of that layer's
    comparison: there the fp32 and fp64 ReLU gates may differ."""
    P64 = {k: v.detach() for k, v in P.items()}
    K = att.shape[1] if am is None else int(am.sum(1).max())
    pre = att.double()[:, :K] @ P64['att_embed.0.weight'].t() + P64['att_embed.0.bias']
    live = torch.ones(pre.shape[:2], dtype=torch.bool, device=pre.device) if am is None else am[:, :K].bool()
    edge_att = (pre.abs() < 1e-4)[live].any(0)
    edge_fc = ((fc.double() @ P64['fc_embed.0.weight'].t() + P64['fc_embed.0.bias']).abs() < 1e-4).any(0)
    assert int(edge_att.sum()) <= pre.shape[-1] // 20 and int(edge_fc.sum()) <= pre.shape[-1] // 20
    for k, p in model.named_parameters():
        a, b = p.grad, P[k].grad
        if k == 'core.attention.alpha_net.bias':     # exactly 0 (the softmax is shift invariant): compare absolutely
            assert float(a.abs().max()) < 1e-6 and float(b.abs().max()) < 1e-9, k
            continue
        if k.startswith('att_embed.'):
            a, b = a[~edge_att], b[~edge_att]
        if k.startswith('fc_embed.'):
            a, b = a[~edge_fc], b[~edge_fc]
        assert rel(a, b) < 1e-3, (k, rel(a, b))


# ---------------------------------------------------------------------------------------------- the reference's fixture
@pytest.mark.parametrize('flatten', [False, True])
@pytest.mark.parametrize('name', VARIANTS)
def test_golden_xe_logp_loss_and_grads(name, flatten):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    fx, model, t = golden_model(name, flatten)
    model.train()                  # drop_prob_lm 0: dropout is the identity
    labels, masks = t('labels'), t('masks')
    logp = model(t('fc'), t('att'), labels[..., :-1], t('att_masks'))
    np.testing.assert_allclose(logp.detach().cpu().numpy(), fx['xe_logp'], rtol=2e-5, atol=5e-6)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    np.testing.assert_allclose(loss.item(), fx['xe_loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, fx, 'xe_grad.')


@pytest.mark.parametrize('name', VARIANTS)
def test_golden_greedy_and_beam3(name):
    fx, model, t = golden_model(name)
    model.eval()
    with torch.no_grad():
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        assert np.array_equal(seq.cpu().numpy(), fx['greedy_seq'])
        np.testing.assert_allclose(slp.cpu().numpy(), fx['greedy_logp'], rtol=2e-5, atol=5e-6)
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1},
                         mode='sample')
        assert np.array_equal(seq.cpu().numpy(), fx['beam3_seq'])
        np.testing.assert_allclose(slp.cpu().numpy(), fx['beam3_logp'], rtol=2e-5, atol=5e-6)


def inject(model, drops):
    model._drop_masks = {'drop_' + k: v.to(DEV).contiguous() for k, v in drops.items()}


@pytest.mark.parametrize('name', VARIANTS)
def test_golden_train_mode_with_recorded_dropout_masks(name):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    fx, model, t = golden_model(name, drop_prob_lm=0.5)
    T_steps = fx['train_logp'].shape[1] - 1
    inject(model, ref.unpack_drops(fx.z, name + '.train', T_steps))
    model.train()
    labels, masks = t('labels'), t('masks')
    logp = model(t('fc'), t('att'), labels[..., :-1], None)
    np.testing.assert_allclose(logp.detach().cpu().numpy(), fx['train_logp'], rtol=2e-5, atol=5e-6)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    np.testing.assert_allclose(loss.item(), fx['train_loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, fx, 'train_grad.')


@pytest.mark.parametrize('name', VARIANTS)
def test_golden_reward_criterion_grads_sparse_route(name):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import RewardCriterion
    fx, model, t = golden_model(name, flatten=True)
    model.eval()
    seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy', 'sample_n': 2}, mode='sample')
    assert np.array_equal(seq.cpu().numpy(), fx['rl_seq'])
    loss = RewardCriterion()(slp, seq, t('rl_reward'))
    np.testing.assert_allclose(loss.item(), fx['rl_loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, fx, 'rl_grad.')


@pytest.mark.parametrize('name', VARIANTS)
def test_golden_scheduled_sampling_with_recorded_inputs(name):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    fx, model, t = golden_model(name)
    coin, gum = ss_draws(fx)
    model.train()
    model.ss_prob = float(0.6)
    model._ss_coin, model._ss_gumbel = coin.to(DEV), gum.to(DEV).contiguous()
    labels, masks = t('labels'), t('masks')
    logp = model(t('fc'), t('att'), labels[..., :-1], t('att_masks'))
    np.testing.assert_allclose(logp.detach().cpu().numpy(), fx['ss_logp'], rtol=2e-5, atol=5e-6)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    np.testing.assert_allclose(loss.item(), fx['ss_loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, fx, 'ss_grad.')


# ---------------------------------------------------------------------------------------------- the sentinel attention alone
def tile_struct(mask=None, p=0.0, seed=0, row0=0):
    from imagecaptioning.pytorch_amd import _lib
    d = _lib.TileDrop()
    d.mask, d.p, d.seed, d.row0 = (None if mask is None else mask.data_ptr()), float(p), int(seed), int(row0)
    return d


def sentinel_inputs(T, B, n, K, A, R, masked, seed):
    g = torch.Generator().manual_seed(seed)
    N = B * n
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    d = dict(fre=r(T, N, A), hoe=r(T, N, A), fr=r(T, N, R), ho=r(T, N, R), p_att=r(B, K, A), att=r(B, K, R), w=0.3 * r(A), b=r(1),
             d_ctx=r(T, N, R))
    mask = None
    if masked:
        mask = torch.ones(B, K)
        for b in range(B):
            mask[b, 1 + (b * 5) % K:] = 0           # region 0 valid for every image
        mask[B - 1] = 1
    return {k: v.to(DEV).contiguous() for k, v in d.items()}, (None if mask is None else mask.to(DEV))


def sentinel_ref(d, mask, n, tile):
    """fp64 torch: (pi [T,N,K+1], ctx [T,N,R]) and the gradients of sum(ctx * d_ctx)"""
    x = {k: v.double().requires_grad_(True) for k, v in d.items() if k != 'd_ctx'}
    pe = torch.cat([x['fre'].unsqueeze(2), x['p_att'].repeat_interleave(n, 0).unsqueeze(0).expand(x['fre'].shape[0], -1, -1, -1)], 2)
    hA = torch.tanh(pe + x['hoe'].unsqueeze(2))
    if tile is not None:
        hA = hA * tile.double()
    pi = F.softmax(hA @ x['w'] + x['b'], dim=2)
    if mask is not None:
        m = mask.double().repeat_interleave(n, 0)
        pi = pi * torch.cat([m[:, :1], m], 1)
        pi = pi / pi.sum(2, keepdim=True)
    val = torch.cat([x['fr'].unsqueeze(2), x['att'].repeat_interleave(n, 0).unsqueeze(0).expand(x['fr'].shape[0], -1, -1, -1)], 2)
    ctx = (pi.unsqueeze(3) * val).sum(2) + x['ho']
    (ctx * d['d_ctx'].double()).sum().backward()
    return pi.detach(), ctx.detach(), {k: v.grad for k, v in x.items()}


def sentinel_run(d, mask, T, B, n, K, A, R, tile_mask=None, p=0.0, seed=0, row0=0):
    """the three entry points; returns pi, ctx and the gradients by input name"""
    from imagecaptioning.pytorch_amd._lib import lib, ptr, check, stream_ptr
    N = B * n
    z = lambda *s: torch.full(s, float('nan'), device=DEV)          # noqa: E731
    pi, ctx = z(T, N, K + 1), z(T, N, R)
    for t in range(T):
        td = tile_struct(None if tile_mask is None else tile_mask[t], p, seed, row0 + t * N)
        check(lib.capmi_sentinel_attention_fwd(ptr(d['fre'][t]), 0, 0, None, ptr(d['hoe'][t]), 0, 0, None, None, None, ptr(d['fr'][t]),
                                               ptr(d['ho'][t]), ptr(d['p_att']), ptr(d['att']), ptr(mask), ptr(d['w']), ptr(d['b']),
                                               C.byref(td), ptr(pi[t]), ptr(ctx[t]), B, n, K, A, R, stream_ptr()), 'sentinel fwd')
    td = tile_struct(tile_mask, p, seed, row0)
    d_e, d_hoe, d_fre, d_fr = z(T, N, K + 1), z(T, N, A), z(T, N, A), z(T, N, R)
    check(lib.capmi_sentinel_attention_bwd(ptr(d['d_ctx']), ptr(d['fr']), ptr(d['fre']), ptr(d['hoe']), ptr(pi), ptr(d['p_att']),
                                           ptr(d['att']), ptr(d['w']), C.byref(td), ptr(d_e), ptr(d_hoe), ptr(d_fre), ptr(d_fr), T, B,
                                           n, K, A, R, stream_ptr()), 'sentinel bwd')
    d_att, d_p_att, d_w, d_b = z(B, K, R), z(B, K, A), z(A), z(1)
    part = z(B * (K + 1), A)
    check(lib.capmi_sentinel_attention_bwd_batched(ptr(d['d_ctx']), ptr(d['fre']), ptr(d['hoe']), ptr(pi), ptr(d_e), ptr(d['p_att']),
                                                   ptr(d['w']), C.byref(td), ptr(d_att), ptr(d_p_att), None, ptr(d_b), T, B, n, K, A, R,
                                                   ptr(part), stream_ptr()), 'sentinel bwd batched')
    d_w = part.sum(0)
    return pi, ctx, dict(fre=d_fre, hoe=d_hoe, fr=d_fr, ho=d['d_ctx'], p_att=d_p_att, att=d_att, w=d_w, b=d_b), d_e


# (T, B, n, K, A, R): K = 1; K not a multiple of the 8 waves' stride; n = 1 and n = 5; A = R = 512; one unaligned small size
SHAPES = [(2, 3, 1, 1, 16, 16), (2, 3, 5, 13, 64, 32), (1, 10, 5, 36, 512, 512), (2, 64, 5, 9, 128, 128), (2, 3, 2, 7, 10, 6),
          (1, 70, 8, 5, 32, 32)]


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_sentinel_attention_kernels_vs_fp64(shape, masked):
    T, B, n, K, A, R = shape
    d, mask = sentinel_inputs(T, B, n, K, A, R, masked, seed=sum(shape))
    for tile in (None, (torch.rand(T, B * n, K + 1, A, generator=torch.Generator().manual_seed(3)) < 0.5).float().mul(2).to(DEV)):
        pi, ctx, g, d_e = sentinel_run(d, mask, T, B, n, K, A, R, tile_mask=tile)
        pi_r, ctx_r, g_r = sentinel_ref(d, mask, n, tile)
        assert float((pi.double() - pi_r).abs().max()) < 2e-6
        assert float((ctx.double() - ctx_r).abs().max()) < 2e-5
        # alpha_net's bias gradient is sum(d_e), exactly 0 in exact arithmetic (the softmax is shift invariant): what is left is
        # the fp32 rounding of the terms, bounded by a few ulps (2^-24 relative each) of the sum of their magnitudes
        assert float(g_r['b'].abs().max()) < 1e-9 and float(g['b'].abs().max()) <= 8 * 2.0 ** -24 * float(d_e.abs().sum())
        for k in g:
            if k == 'b':
                continue
            assert rel(g[k], g_r[k]) < 1e-4 or float((g[k].double().cpu() - g_r[k].cpu()).abs().max()) < 1e-6, (k, rel(g[k], g_r[k]))


def test_sentinel_attention_in_kernel_philox_mask():
    """p > 0 without a mask: the kernels draw the keep bits from (seed, row, score row, column).  With one caption row per image
    and one step per launch the two backward kernels expose every bit they use (d_fre != 0: the sentinel's row, d_p_att != 0: a
    region's row).  The keep rate is within binomial bounds, the single-step numbering (row0 = t * N) is the time-batched one,
    and the recovered bits injected as a mask reproduce the Philox forward and backward: all three kernels use the same bits."""
    T, B, n, K, A, R, p = 2, 12, 1, 11, 64, 32, 0.5
    N = B
    d, _ = sentinel_inputs(T, B, n, K, A, R, False, seed=77)
    pi0, ctx0, g0, _ = sentinel_run(d, None, T, B, n, K, A, R, p=p, seed=1234)
    pi1, _, _, _ = sentinel_run(d, None, T, B, n, K, A, R, p=p, seed=1235)
    assert float((pi0 - pi1).abs().max()) > 1e-3, 'the seed does not reach the mask'
    tile = torch.zeros(T, N, K + 1, A, device=DEV)
    for t in range(T):
        dt = {k: (v if k in ('p_att', 'att', 'w', 'b') else v[t:t + 1].contiguous()) for k, v in d.items()}
        pi_t, _, g_t, _ = sentinel_run(dt, None, 1, B, n, K, A, R, p=p, seed=1234, row0=t * N)
        assert torch.equal(pi_t[0], pi0[t]) and torch.equal(g_t['hoe'][0], g0['hoe'][t])
        tile[t, :, 0] = (g_t['fre'][0] != 0).float() * 2
        tile[t, :, 1:] = (g_t['p_att'] != 0).float() * 2
    cnt = tile.numel()
    rate = float((tile != 0).float().mean())
    assert abs(rate - (1 - p)) < 5 * (p * (1 - p) / cnt) ** 0.5, rate            # five binomial sigmas of 18 432 draws
    assert 0.3 < float((tile[0] != 0).float().mean()) < 0.7 and not torch.equal(tile[0], tile[1])
    pi2, ctx2, g2, _ = sentinel_run(d, None, T, B, n, K, A, R, tile_mask=tile.contiguous())
    assert float((pi2 - pi0).abs().max()) < 1e-6 and float((ctx2 - ctx0).abs().max()) < 1e-5
    for k in g0:
        assert rel(g2[k], g0[k]) < 1e-5, k


# ---------------------------------------------------------------------------------------------- a2i2-like size
def full_model(name, seed=0, drop=0.0):
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(seed)
    o = opt_(name, V=9487, input_encoding_size=512, rnn_size=512, att_hid_size=512, fc_feat_size=2048, att_feat_size=2048,
             drop_prob_lm=drop, seq_length=16, max_length=20)
    model = models.setup(o)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    return model.to(DEV)


def full_inputs(B=10, K=36, seed=1):
    g = torch.Generator().manual_seed(seed)
    fc = torch.randn(B, 2048, generator=g).clamp_min(0).to(DEV)
    att = torch.randn(B, K, 2048, generator=g).clamp_min(0).to(DEV)
    am = torch.ones(B, K)
    for b in range(B):
        am[b, 10 + (b * 7) % 27:] = 0
    am[3] = 1                                            # one full row: clip_att keeps K = 36
    return fc, att, am.to(DEV)


def full_drops(B, N, T, K, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    m = lambda *s: ((torch.rand(*s, generator=g) >= p).float() / (1 - p)).to(DEV)          # noqa: E731
    return dict(fc=m(B, 512), att=m(B, K, 512), xt=m(T, N, 512), h=m(T, N, 512), fake=m(T, N, 512), fr=m(T, N, 512), ho=m(T, N, 512),
                tile=m(T, N, K + 1, 512), out=m(T, N, 512))


def params64(model):
    return {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}


@pytest.mark.parametrize('name', VARIANTS)
def test_full_size_xe_vs_restatement(name):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    model = full_model(name, drop=0.5)
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
    T_eff = int((labels.reshape(B * n, -1)[:, 1:T + 1].sum(0) > 0).sum()) + 1
    drops = full_drops(B, B * n, T_eff, 36, seed=21)
    inject(model, drops)
    logp = model(fc, att, labels[..., :-1], am)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    model.zero_grad()
    loss.backward()
    P = params64(model)
    logp_r = ref.xe(P, fc, att, am, labels[..., :-1], drops)
    assert float((logp.detach().double() - logp_r.detach()).abs().max()) < 1e-4
    tgt = labels[..., 1:].reshape(B * n, -1)[:, :logp_r.shape[1]]
    m = masks[..., 1:].reshape(B * n, -1)[:, :logp_r.shape[1]].double()
    loss_r = -(logp_r.gather(2, tgt.unsqueeze(2)).squeeze(2) * m).sum() / m.sum()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, fc, att, am)


@pytest.mark.parametrize('name', VARIANTS)
def test_full_size_scst_sample_and_grads_vs_restatement(name):
    """SCST rollouts at bs 10 x 5, L = 20: sampled rows with injected Gumbel noise in eval numerics (the rollout's tokens are
    the restatement's arg-max), RewardCriterion loss and every gradient."""
    from imagecaptioning.pytorch_amd.captioning.modules.losses import RewardCriterion
    model = full_model(name, seed=3)
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
    seq_r, slp_r = ref.rollout(P, fc, att, am, n, L, gumbel=gum)
    assert torch.equal(seq.cpu(), seq_r.cpu()), 'sampled tokens differ'
    assert float((slp.detach().double() - slp_r.detach()).abs().max()) < 1e-4
    sel = slp_r.gather(2, seq_r.unsqueeze(2)).squeeze(2)
    m = torch.cat([torch.ones(N, 1, dtype=ref.D, device=DEV), (seq_r > 0).double()[:, :-1]], 1)
    loss_r = -(sel * reward.double() * m).sum() / m.sum()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, fc, att, am)


@pytest.mark.parametrize('name', VARIANTS)
def test_full_size_scheduled_sampling_vs_restatement(name):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    model = full_model(name, seed=7, drop=0.5)
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
    drops = full_drops(B, N, T + 1, 36, seed=22)
    inject(model, drops)
    model.ss_prob = 0.25
    model._ss_coin, model._ss_gumbel = coin.to(DEV), gum.to(DEV).contiguous()
    logp = model(fc, att, labels[..., :-1], am)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    model.zero_grad()
    loss.backward()
    P = params64(model)
    logp_r = ref.xe(P, fc, att, am, labels[..., :-1], drops, ss_coin=coin.to(DEV), ss_gumbel=gum.to(DEV))
    assert float((logp.detach().double() - logp_r.detach()).abs().max()) < 1e-4
    tgt = labels[..., 1:].reshape(N, -1)
    loss_r = -logp_r.gather(2, tgt.unsqueeze(2)).squeeze(2).mean()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, fc, att, am)


def test_train_mode_draws_its_own_masks_and_they_move_with_the_seed():
    """the product path: nothing injected, every site (the in-kernel tile included) drawn from the model's seed stream"""
    fx, model, t = golden_model('adaatt', drop_prob_lm=0.5)
    model.train()
    labels = t('labels')
    torch.manual_seed(11)
    a = model(t('fc'), t('att'), labels[..., :-1], t('att_masks'))
    b = model(t('fc'), t('att'), labels[..., :-1], t('att_masks'))
    assert bool(torch.isfinite(a).all()) and float((a - b).detach().abs().max()) > 1e-3
    a.sum().backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())


# ---------------------------------------------------------------------------------------------- stepper, options, edges
@pytest.mark.parametrize('name', VARIANTS)
def test_one_call_greedy_equals_stepper_greedy(name):
    from imagecaptioning.pytorch_amd import decode
    model = full_model(name, seed=11)
    model.eval()
    fc, att, am = full_inputs(seed=12)
    with torch.no_grad():
        seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'sample_n': 2}, mode='sample')
        st = model._stepper(fc, att, am)(2)
        seq_s, slp_s = decode.sample_steps(model, st, 10, model.seq_length, {'sample_method': 'greedy', 'sample_n': 2}, DEV)
    assert torch.equal(seq, seq_s)
    assert float((slp - slp_s).abs().max()) < 1e-4


def test_decode_options_run_through_the_stepper():
    fx, model, t = golden_model('adaattmo')
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
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy', 'output_logsoftmax': 0}, mode='sample')
        ref_seq, ref_slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        assert torch.equal(seq, ref_seq)
        live = ref_slp.abs().sum(2) > 0
        assert float((torch.log_softmax(slp, 2) - ref_slp)[live].abs().max()) < 1e-5


@pytest.mark.parametrize('name', VARIANTS)
def test_get_logprobs_state_matches_the_rollout(name):
    fx, model, t = golden_model(name)
    model.eval()
    with torch.no_grad():
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        fc, att, patt, am = model._prepare_feature(t('fc'), t('att'), t('att_masks'))
        state = model.init_hidden(3)
        it = torch.zeros(3, dtype=torch.long, device=DEV)
        for s in range(3):
            logp, state = model.get_logprobs_state(it, fc, att, patt, am, state)
            assert state[0].shape == (1, 3, 16)
            live = (seq[:, :s] > 0).all(1) if s else torch.ones(3, dtype=torch.bool, device=DEV)
            np.testing.assert_allclose(logp[live].cpu().numpy(), slp[:, s][live].cpu().numpy(), rtol=1e-5, atol=1e-5)
            it = seq[:, s].clone()


@pytest.mark.parametrize('name', VARIANTS)
def test_edge_cases_eos_mixed_lengths_k1_and_full_mask(name):
    fx, model, t = golden_model(name)
    model.eval()
    P = {k: v.detach().cpu() for k, v in model.named_parameters()}
    with torch.no_grad():
        # immediate EOS for every row, and mixed lengths
        model.logit.bias[0] += 50.0
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        assert int(seq.abs().sum()) == 0 and float(slp[:, 1:].abs().max()) == 0.0
        model.logit.bias[0] -= 50.0
        seq, slp = model(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        seq_r, slp_r = ref.rollout(P, fx.t('fc'), fx.t('att'), fx.t('att_masks'), 1, 8)
        assert torch.equal(seq.cpu(), seq_r)
        lens = (seq > 0).sum(1)
        assert int(lens.min()) < int(lens.max())
        np.testing.assert_allclose(slp.cpu().numpy(), slp_r.numpy(), rtol=2e-5, atol=5e-6)
        # K = 1
        att1 = t('att')[:, :1].contiguous()
        seq, slp = model(t('fc'), att1, None, opt={'sample_method': 'greedy'}, mode='sample')
        seq_r, slp_r = ref.rollout(P, fx.t('fc'), att1.cpu(), None, 1, 8)
        assert torch.equal(seq.cpu(), seq_r)
        np.testing.assert_allclose(slp.cpu().numpy(), slp_r.numpy(), rtol=2e-5, atol=5e-6)
        # an all-ones mask equals att_masks=None
        ones = torch.ones(3, 6, device=DEV)
        a = model(t('fc'), t('att'), ones, opt={'sample_method': 'greedy'}, mode='sample')
        b = model(t('fc'), t('att'), None, opt={'sample_method': 'greedy'}, mode='sample')
        assert torch.equal(a[0], b[0])
        assert float((a[1] - b[1]).abs().max()) < 1e-6


# ---------------------------------------------------------------------------------------------- ensemble with an Att2in2 member
def test_ensemble_of_adaatt_and_att2in2_vs_fp64_mixture():
    """greedy: tokens and log-probs of the mean of the members' fp64 probabilities, stepped jointly; beam 3: the returned rows are
    that mixture's log-probs along the returned sequences."""
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    fx, ada, t = golden_model('adaatt')
    z2 = np.load(os.path.join(GOLDEN, 'att2in2_tiny.npz'))
    P2 = {k[2:]: torch.from_numpy(z2[k]) for k in z2.files if k.startswith('P.')}
    a2 = models.setup(opt_('att2in2', att_hid_size=12))
    a2.load_state_dict(P2)
    ens = AttEnsemble([ada, a2.to(DEV)]).to(DEV).eval()
    fc, att, am = fx.t('fc'), fx.t('att'), fx.t('att_masks')
    P1 = ref._p(fx.params())
    P2 = ref._p(P2)
    f1, a1, p1, m1 = ref.prefill(P1, fc, att, am)
    a2f, p2, m2 = ref_a2.prefill(P2, att, am)

    def mixture_along(seq):
        """fp64 mixture log-probs [N, L, V1] teacher-forced along seq (zero after a row has ended, as the decoders store them)"""
        N, L = seq.shape
        h1 = c1 = torch.zeros(N, 16, dtype=ref.D)
        h2 = c2 = torch.zeros(N, 16, dtype=ref.D)
        it = torch.zeros(N, dtype=torch.long)
        out = torch.zeros(N, L, 31, dtype=ref.D)
        alive = torch.ones(N, dtype=torch.bool)
        for s in range(L):
            l1, h1, c1 = ref.step(P1, it, h1, c1, f1, a1, p1, m1, 1)
            l2, h2, c2 = ref_a2.step(P2, it, h2, c2, a2f, p2, m2, 1)
            out[:, s] = torch.log(0.5 * F.softmax(l1, 1) + 0.5 * F.softmax(l2, 1)) * alive.unsqueeze(1)
            it = seq[:, s]
            alive = alive & (it > 0)
        return out

    with torch.no_grad():
        seq, slp = ens(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy'}, mode='sample')
        seq, slp = seq.cpu(), slp.cpu()
        want = mixture_along(seq)
        np.testing.assert_allclose(slp.numpy(), want.numpy(), rtol=2e-5, atol=5e-6)
        # greedy: every stored token is the arg-max of the fp64 mixture (0 once a row has ended)
        alive = torch.ones(3, dtype=torch.bool)
        for s in range(8):
            assert torch.equal(seq[:, s][alive], want[:, s].argmax(1)[alive])
            alive = alive & (seq[:, s] > 0)
        seq, slp = ens(t('fc'), t('att'), t('att_masks'), opt={'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1}, mode='sample')
        seq, slp = seq.cpu(), slp.cpu()
        want = mixture_along(seq)
        live = torch.cat([torch.ones(3, 1, dtype=torch.bool), (seq > 0)[:, :-1]], 1)
        np.testing.assert_allclose(slp[live].numpy(), want[live].numpy(), rtol=2e-5, atol=5e-6)


# ---------------------------------------------------------------------------------------------- command-line tools
@pytest.mark.parametrize('name', VARIANTS)
def test_tools_train_xe_scst_nsc_with_resume_and_eval(name, tmp_path):
    """tools/train.py on synthetic data: XE (scheduled sampling from epoch 0), self-critical after a resume, then
    new_self_critical; losses finite, the XE loss falls over 30 steps; tools/eval.py decodes from the checkpoint with beam search."""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import opts, rewards
    small = ['--caption_model', name, '--rnn_size', '64', '--input_encoding_size', '64', '--att_hid_size', '64',
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
    from imagecaptioning.pytorch_amd.tools import eval as E
    loss, preds = E.main(opts.parse_opt(small + ['--beam_size', '3', '--sample_method', 'beam_search', '--num_images', '8',
                                                 '--start_from', str(tmp_path)]))
    assert len(preds) == 8 and all(isinstance(p['caption'], str) for p in preds)
    assert loss == loss
