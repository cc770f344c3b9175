"""Scheduled sampling for NewFC / AoA / Att2in2 without a GPU: the fp64 restatements (tests/ss_ref64.py over the oracle's single
steps, tests/att2in2_ref64.py) reproduce the real reference's scheduled-sampling fixture tests/golden/ss_tiny.npz, the new struct
field sits where the header puts it, and eval mode never builds an ss_mode."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN
import att2in2_ref64
import ss_ref64 as ref

Z = os.path.join(GOLDEN, 'ss_tiny.npz')
HEADS = 2          # make_ss.family_opt('aoa').num_heads


def load(family):
    z = np.load(Z)
    pre = family + '.'
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    P = {k[2:]: torch.from_numpy(v) for k, v in d.items() if k.startswith('P.')}
    t = {k: torch.from_numpy(d[k]) for k in ('fc', 'att', 'labels', 'masks', 'att_masks', 'fed')}
    return d, P, t


def forward(family, P, t, dtype=ref.D, **how):
    seq = t['labels'][..., :-1]
    if family == 'newfc':
        return ref.newfc_xe(P, t['fc'], seq, dtype=dtype, **how)[0]
    if family == 'aoa':
        return ref.aoa_xe(P, t['att'], t['att_masks'], seq, HEADS, dtype=dtype, **how)[0]
    assert dtype == ref.D and 'fed' not in how
    return att2in2_ref64.xe(P, t['att'], t['att_masks'], seq, **how)


def _close_grads(g, d):
    """the tolerances tests/test_att2in2_host.py applies to its fixture"""
    for k, v in g.items():
        r = d['grad.' + k]
        np.testing.assert_allclose(v.numpy(), r, rtol=1e-4, atol=1e-6 + 1e-5 * np.abs(r).max(), err_msg=k)


@pytest.mark.parametrize('family', ['newfc', 'aoa', 'att2in2'])
def test_restatement_replays_the_reference_scheduled_sampling_fixture(family):
    d, P, t = load(family)
    V1 = P['logit.weight'].shape[0]
    T_eff = t['fed'].shape[0]
    assert T_eff == t['labels'].shape[-1] - 2                       # the all-pad-column break fired
    coin, noise = ref.injection(t['fed'], t['labels'][..., :-1], V1)
    assert int(coin.sum()) * 3 > (T_eff - 1) * coin.shape[1]        # the fixture really samples
    Pg = {k: v.to(ref.D).requires_grad_(True) for k, v in P.items()}
    logp = forward(family, Pg, t, ss_coin=coin, ss_gumbel=noise)
    np.testing.assert_allclose(logp.detach().numpy(), d['logp'], rtol=1e-5, atol=1e-6)
    loss = ref.lm_loss(logp, t['labels'], t['masks'])
    np.testing.assert_allclose(loss.item(), d['loss'], rtol=1e-6)
    loss.backward()
    _close_grads({k: v.grad for k, v in Pg.items()}, d)
    # plain teacher forcing is a different function of the same inputs: the fixture does pin the sampled inputs
    with torch.no_grad():
        plain = forward(family, P, t)
    assert float((plain.numpy() - d['logp'])[:, 1:T_eff].__abs__().max()) > 1e-2


@pytest.mark.parametrize('family', ['newfc', 'aoa'])
def test_fed_token_table_and_injected_coins_are_the_same_run(family):
    d, P, t = load(family)
    coin, noise = ref.injection(t['fed'], t['labels'][..., :-1], P['logit.weight'].shape[0])
    seq = t['labels'][..., :-1]
    args = (P, t['fc'], seq) if family == 'newfc' else (P, t['att'], t['att_masks'], seq, HEADS)
    fn = ref.newfc_xe if family == 'newfc' else ref.aoa_xe
    with torch.no_grad():
        a, fed_a = fn(*args, ss_coin=coin, ss_gumbel=noise)
        b, fed_b = fn(*args, fed=t['fed'])
    assert torch.equal(fed_a, t['fed']) and torch.equal(fed_b, t['fed'])
    assert torch.equal(a, b)


@pytest.mark.parametrize('family', ['newfc', 'aoa'])
def test_fp32_restatement_draws_the_fp64_tokens_under_real_noise(family):
    """With real Gumbel noise the arg-max of fp32 and of fp64 log-probs can differ only at a near-tie of the top two candidates.
    At this size none occurs: the allowance of the full-size GPU test (rows whose top two are within 1e-4, at most 1 % of the coin
    positions) is not needed here."""
    d, P, t = load(family)
    seq = t['labels'][..., :-1]
    N, T = seq.reshape(-1, seq.shape[-1]).shape
    V1 = P['logit.weight'].shape[0]
    g = torch.Generator().manual_seed(5)
    coin = torch.rand(T, N, generator=g) < 0.6
    coin[0] = False
    gum = -torch.log(-torch.log(torch.rand(T, N, V1, generator=g).clamp(1e-10, 1 - 1e-7)))
    args = (P, t['fc'], seq) if family == 'newfc' else (P, t['att'], t['att_masks'], seq, HEADS)
    fn = ref.newfc_xe if family == 'newfc' else ref.aoa_xe
    with torch.no_grad():
        l64, fed64 = fn(*args, ss_coin=coin, ss_gumbel=gum)
        l32, fed32 = fn(*args, ss_coin=coin, ss_gumbel=gum, dtype=torch.float32)
    assert l32.dtype == torch.float32 and l64.dtype == torch.float64
    assert int((fed32 != fed64).sum()) == 0
    assert float((l32.double() - l64).abs().max()) < 1e-4


def test_newfc_rollout_struct_ends_with_ss_mode():
    from imagecaptioning.pytorch_amd import _lib
    assert _lib.NewFCRollout._fields_[-1][0] == 'ss_mode'
    src = open(os.path.join(ROOT, 'include', 'capmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    body = re.search(r'typedef struct capmi_newfc_rollout \{([^{}]*?)\} capmi_newfc_rollout;', src, flags=re.S).group(1)
    names = []
    for stmt in body.split(';'):
        for part in stmt.strip().split(','):
            if part.strip():
                names.append(re.findall(r'(\w+)\s*$', part.strip())[0])
    assert names == [f[0] for f in _lib.NewFCRollout._fields_]
    assert names[-3:] == ['partial', 'partial_capacity', 'ss_mode']


def _tiny_opt(family):
    V = 30
    o = argparse.Namespace(caption_model=family, vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1, drop_prob_lm=0.0,
                           seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=12, use_bn=0, logit_layers=1,
                           vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    if family == 'aoa':
        o.refine, o.refine_aoa, o.use_ff, o.decoder_type, o.use_multi_head = 1, 1, 0, 'AoA', 2
        o.num_heads, o.multi_head_scale, o.mean_feats, o.ctx_drop, o.dropout_aoa, o.num_layers = 2, 1, 1, 1, 0.0, 2
    return o


@pytest.mark.parametrize('family', ['newfc', 'aoa'])
def test_forward_builds_ss_mode_in_train_mode_only(family):
    """_forward hands _run its rollout configuration: eval mode ignores ss_prob (AttModel.py:145), train mode with ss_prob > 0 adds
    ss_mode [T_eff,N] (1 = draw, 2 = label) from the injected coins, a seed and the injected noise.  _run is replaced: no device."""
    from imagecaptioning.pytorch_amd.captioning import models
    model = models.setup(_tiny_opt(family))
    seen = []

    def spy(cfg, *a, **kw):
        seen.append(dict(cfg))
        raise StopIteration
    model._run = spy
    B, n, T = 2, 2, 6
    labels = torch.randint(1, 31, (B, n, T))
    labels[..., 0] = 0
    labels[..., T - 1] = 0                       # T_eff = T - 1
    fc, att = torch.zeros(B, 20), torch.zeros(B, 3, 20)

    def call():
        with pytest.raises(StopIteration):
            model._forward(fc, att, labels)
        return seen.pop()
    model.ss_prob = 0.5
    model.eval()
    assert 'ss_mode' not in call() and model._rng_calls == 0
    model.train()
    model.ss_prob = 0.0
    assert 'ss_mode' not in call() and model._rng_calls == 0
    model.ss_prob = 0.5
    coin = torch.zeros(T - 1, B * n, dtype=torch.bool)
    coin[2, 1] = coin[3] = True
    model._ss_coin, model._ss_gumbel = coin, torch.zeros(T - 1, B * n, 31)
    cfg = call()
    assert cfg['teacher'] and cfg['T'] == T - 1 and cfg['L'] == T
    assert cfg['ss_mode'].dtype == torch.uint8 and torch.equal(cfg['ss_mode'], torch.where(coin, 1, 2).to(torch.uint8))
    assert cfg['gumbel'] is model._ss_gumbel and cfg['seed'] != 0 and model._rng_calls == 1
    model._ss_coin = model._ss_gumbel = None
    torch.manual_seed(3)
    cfg = call()
    assert tuple(cfg['ss_mode'].shape) == (T - 1, B * n) and 'gumbel' not in cfg
    assert set(cfg['ss_mode'].unique().tolist()) == {1, 2}
