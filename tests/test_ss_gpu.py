"""Scheduled sampling (AttModel._forward with ss_prob > 0, reference AttModel.py:144-162) of NewFC, AoA and Att2in2 on a real MI355X.

* against the real reference's fixture tests/golden/ss_tiny.npz: the coins / noise that reproduce its fed tokens are injected
  (ss_ref64.injection), then fed tokens, log-probs, loss and every gradient are compared;
* NewFC and AoA at the sizes bench.py builds for newfc_xe / aoa_nsc (bs 10 x 5, T 16, ss_prob 0.25, their dropout ON with the engine's
  own masks handed to the restatement) against tests/ss_ref64.py in fp64;
* AoA's routes (activation planes / plain, folded / separate embedding, > 64 rows), the Philox route without hooks, the
  launch-for-launch identity at ss_prob 0 and in eval mode, argument contracts, and tools/train.py through its schedule.
"""
import contextlib
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import ss_ref64 as ref
from test_ss_host import load, _tiny_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PKG = ROOT + '/imagecaptioning/pytorch_amd'


# ------------------------------------------------------------------------------------------------ helpers
@contextlib.contextmanager
def engines():
    """the engine objects (newfc_engine.Rollout / att2in2_engine.Rollout / aoa_engine.AoAGraph) of the rollouts run inside"""
    from imagecaptioning.pytorch_amd import newfc_engine, att2in2_engine, aoa_engine
    got, saved = [], []
    for cls, name in ((newfc_engine.Rollout, 'run'), (att2in2_engine.Rollout, 'run'), (aoa_engine.AoAGraph, 'rollout')):
        orig = getattr(cls, name)

        def wrapped(self, *a, _orig=orig, **kw):
            got.append(self)
            return _orig(self, *a, **kw)
        saved.append((cls, name, orig))
        setattr(cls, name, wrapped)
    try:
        yield got
    finally:
        for cls, name, orig in saved:
            setattr(cls, name, orig)


def no_hardcoded_dropout(monkeypatch):
    """AoAGraph's attention-probability and sublayer dropouts are fixed at 0.1 in train mode (AoAModel.py:18,119); the fixture was
    recorded with every dropout probability 0"""
    from imagecaptioning.pytorch_amd import aoa_engine
    real = aoa_engine.Dropper
    monkeypatch.setattr(aoa_engine, 'Dropper', lambda p, seed, dev, training: real(0.0, seed, dev, training))


def tiny_model(family, flatten=False):
    from imagecaptioning.pytorch_amd.captioning import models
    d, P, t = load(family)
    model = models.setup(_tiny_opt(family))
    model.load_state_dict(P)
    model = model.to(DEV)
    if flatten:
        model.flatten_parameters_()
    return d, P, {k: v.to(DEV) for k, v in t.items()}, model


def forward_args(family, t, B=None):
    sl = slice(None) if B is None else slice(0, B)
    return (t['fc'][sl], t['att'][sl], t['labels'][sl][..., :-1], t['att_masks'][sl])


def inject(model, coin, noise):
    model._ss_coin, model._ss_gumbel = coin.to(DEV), noise.to(DEV).contiguous()


def check_grads(model, d, rtol=5e-4):
    """the tolerances tests/test_att2in2_gpu.py applies to its fixture"""
    for k, p in model.named_parameters():
        r = d['grad.' + k]
        np.testing.assert_allclose(p.grad.cpu().numpy(), r, rtol=rtol, atol=1e-6 + 2e-5 * np.abs(r).max(), err_msg=k)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def check_draws(it_all, logp, coin, gum, seq, cap=0.005):
    """every token fed at a coin position (t >= 1) is the arg-max of the HIP log-probs of step t-1 plus the injected noise; a row
    may differ only when its top two candidates are within 1e-4 of each other, and at most `cap` of the coin positions may.
    The cap: ss_ref64 in fp32 against itself in fp64 on the inputs of the two full-size tests below (no dropout) moves no arg-max
    at all (0 of 210 and 0 of 185 coin positions, log-probs within 1.7e-6), so the 1 % the allowance was designed with is halved:
    at about 200 coin positions that is ONE position, for a near-tie that a log-prob error inside the 1e-4 bound may still flip."""
    T_eff, N = it_all.shape
    it_all, coin, seq = it_all.cpu(), coin.cpu()[:T_eff], seq.reshape(N, -1).cpu()
    assert torch.equal(it_all[0], seq[:, 0])
    forced = ~coin
    forced[0] = True
    assert torch.equal(it_all[forced], seq[:, :T_eff].t()[forced]), 'a teacher-forced position did not feed its label'
    score = logp.detach().double().cpu()[:, :T_eff - 1].transpose(0, 1) + gum.double().cpu()[:T_eff - 1]       # [T_eff-1, N, V1]
    top2 = score.topk(2, dim=2)
    fed = it_all[1:]
    c = coin[1:]
    wrong = (top2.indices[..., 0] != fed) & c
    near = (top2.values[..., 0] - top2.values[..., 1]) < 1e-4
    second = top2.indices[..., 1] == fed
    bad = wrong & ~(near & second)
    n_coin, n_allow = int(c.sum()), int((wrong & near & second).sum())
    assert n_coin > 0
    assert not bool(bad.any()), '%d of %d coin positions fed a token that is not the arg-max' % (int(bad.sum()), n_coin)
    assert n_allow <= cap * n_coin, '%d of %d coin positions used the near-tie allowance (cap %g)' % (n_allow, n_coin, cap)
    return n_coin, n_allow


# ------------------------------------------------------------------------------------------------ 3. the reference's fixture
@pytest.mark.parametrize('flatten', [False, True])
@pytest.mark.parametrize('family', ['newfc', 'aoa', 'att2in2'])
def test_fixture_fed_tokens_logp_loss_and_grads(family, flatten, monkeypatch):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    no_hardcoded_dropout(monkeypatch)
    d, P, t, model = tiny_model(family, flatten)
    model.train()
    model.ss_prob = float(d['ss_prob'])
    coin, noise = ref.injection(t['fed'].cpu(), t['labels'].cpu()[..., :-1], P['logit.weight'].shape[0])
    inject(model, coin, noise)
    with engines() as eng:
        logp = model(*forward_args(family, t))
    assert len(eng) == 1
    T_eff = t['fed'].shape[0]
    assert torch.equal(eng[0].it_all[:T_eff].cpu(), t['fed'].cpu()), 'fed tokens differ from the reference run'
    np.testing.assert_allclose(logp.detach().cpu().numpy(), d['logp'], rtol=2e-5, atol=5e-6)
    loss = LanguageModelCriterion()(logp, t['labels'][..., 1:], t['masks'][..., 1:])
    np.testing.assert_allclose(loss.item(), d['loss'], rtol=1e-5)
    model.zero_grad()
    loss.backward()
    check_grads(model, d)


# ------------------------------------------------------------------------------------------------ 4. full size vs the fp64 restatement
def full_labels(B, n, T, V1, seed):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(1, V1, (B, n, T + 2), generator=g)
    labels[..., 0] = 0
    labels[..., T + 1:] = 0
    coin = torch.rand(T + 1, B * n, generator=g) < 0.25
    coin[0] = False
    gum = -torch.log(-torch.log(torch.rand(T + 1, B * n, V1, generator=g).clamp(1e-10, 1 - 1e-7)))
    return labels.to(DEV), torch.ones(B, n, T + 2, device=DEV), coin, gum


def params64(model):
    return {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}


def full_model(name, seed):
    """the model bench.py builds for --config newfc_xe / aoa_nsc (its dropout rates included)"""
    sys.path.insert(0, ROOT)
    import bench
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(seed)
    model = models.setup(bench._opt(name))
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.02 * torch.randn_like(p))
    return model.to(DEV).train()


def second_seed(model):
    """the seed of the second _next_seed() call after _rng_calls = 0: the first is the scheduled-sampling draw's"""
    keep = model._rng_calls
    model._rng_calls = 1
    s = model._next_seed()
    model._rng_calls = keep
    return s


def test_full_size_newfc_vs_restatement():
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    model = full_model('newfc', seed=7)
    B, n, T, V1 = 10, 5, 16, model.vocab_size + 1
    N = B * n
    assert (model.rnn_size, model.input_encoding_size, V1) == (512, 512, 9488) and model.drop_prob_lm == 0.5
    fc = torch.randn(B, 2048, generator=torch.Generator().manual_seed(8)).clamp_min(0).to(DEV)
    labels, masks, coin, gum = full_labels(B, n, T, V1, seed=9)
    model.ss_prob = 0.25
    inject(model, coin, gum)
    model._rng_calls = 0
    with engines() as eng:
        logp = model(fc, None, labels[..., :-1], None)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    model.zero_grad()
    loss.backward()
    it_all = eng[0].it_all
    assert it_all.shape[0] == T + 1
    n_coin, n_allow = check_draws(it_all, logp, coin, gum, labels[..., :-1])
    print('newfc: %d coin positions, %d near-tie allowances' % (n_coin, n_allow))
    drop_out = ops.dropout_mask((T + 1, N, model.rnn_size), 0.5, second_seed(model), 0, torch.device(DEV))
    assert torch.equal(drop_out, eng[0].drop_out)
    P = params64(model)
    logp_r, fed_r = ref.newfc_xe(P, fc, labels[..., :-1], fed=it_all, drop_out=drop_out)
    assert torch.equal(fed_r, it_all)
    assert float((logp.detach().double() - logp_r.detach()).abs().max()) < 1e-4
    loss_r = -logp_r.gather(2, labels[..., 1:].reshape(N, -1).unsqueeze(2)).squeeze(2).mean()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    for k, p in model.named_parameters():
        assert rel(p.grad, P[k].grad) < 1e-3, k


def test_full_size_aoa_vs_restatement():
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    from test_aoa_train_mode_gpu import realisation
    model = full_model('aoa_nsc', seed=11)
    B, n, T, K, V1 = 10, 5, 16, 36, model.vocab_size + 1
    N = B * n
    assert (model.rnn_size, model.input_encoding_size, model.num_heads, V1) == (1024, 1024, 8, 9488)
    assert model.drop_prob_lm == 0.5 and model.dropout_aoa == 0.3
    att = (torch.randn(B, K, 2048, generator=torch.Generator().manual_seed(12)) * 0.5).clamp_min(0).to(DEV)
    am = torch.ones(B, K)
    for b in range(B):
        am[b, 10 + (b * 7) % 27:] = 0
    am[3, :K - 2] = 1                                   # the longest row: the clip moves K to 34
    am = am.to(DEV)
    Kc = int(am.sum(1).max())
    labels, masks, coin, gum = full_labels(B, n, T, V1, seed=13)
    model.ss_prob = 0.25
    inject(model, coin, gum)
    model._rng_calls = 0
    with engines() as eng:
        logp = model(None, att, labels[..., :-1], am)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    model.zero_grad()
    loss.backward()
    it_all = eng[0].it_all
    assert it_all.shape[0] == T + 1
    n_coin, n_allow = check_draws(it_all, logp, coin, gum, labels[..., :-1])
    print('aoa: %d coin positions, %d near-tie allowances' % (n_coin, n_allow))
    # the engine's own dropout realisation, handed to the restatement through the oracle's hooks
    named = {k: v.to(DEV) for k, v in realisation(model, second_seed(model), B, Kc, N, T + 1).items()}
    used = set()

    def drop(name, x):
        used.add(name)
        assert named[name].shape == x.shape, (name, named[name].shape, x.shape)
        return x * named[name].to(x)
    P = params64(model)
    logp_r, fed_r = ref.aoa_xe(P, att, am, labels[..., :-1], model.num_heads, fed=it_all, drop=drop)
    assert used == set(named), set(named) ^ used
    assert torch.equal(fed_r, it_all)
    assert float((logp.detach().double() - logp_r.detach()).abs().max()) < 1e-4
    loss_r = -logp_r.gather(2, labels[..., 1:].reshape(N, -1).unsqueeze(2)).squeeze(2).mean()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    # att_embed units whose pre-activation is within 1e-4 of zero for some live (image, region): the fp32 and fp64 ReLU gates may
    # differ there (the exclusion of test_att2in2_gpu.check_rel)
    P64 = {k: v.detach() for k, v in P.items()}
    pre = att.double()[:, :Kc] @ P64['att_embed.0.weight'].t() + P64['att_embed.0.bias']
    edge = (pre.abs() < 1e-4)[am[:, :Kc].bool()].any(0)
    assert int(edge.sum()) <= pre.shape[-1] // 20, int(edge.sum())
    for k, p in model.named_parameters():
        a, b = p.grad, P[k].grad
        if k.endswith('self_attn.linears.1.bias'):       # attention key bias: the softmax cancels it, gradient mathematically zero
            continue
        if k.startswith('att_embed.'):
            a, b = a[~edge], b[~edge]
        assert rel(a, b) < 1e-3, k


# ------------------------------------------------------------------------------------------------ 5. AoA routes
def _aoa_injected(monkeypatch, planes, slabs, B_rep=1):
    """the fixture's AoA run (B_rep > 1: its images repeated, so 6 * B_rep rows) on one route; -> (it_all, logp)"""
    from imagecaptioning.pytorch_amd import aoa_engine
    no_hardcoded_dropout(monkeypatch)
    if planes is None:
        monkeypatch.delenv('CAPMI_AOA_PLANES', raising=False)
    else:
        monkeypatch.setenv('CAPMI_AOA_PLANES', planes)
    monkeypatch.setattr(aoa_engine, 'SLAB_CONSUMERS', slabs)
    d, P, t, model = tiny_model('aoa')
    model.train()
    model.ss_prob = float(d['ss_prob'])
    coin, noise = ref.injection(t['fed'].cpu(), t['labels'].cpu()[..., :-1], P['logit.weight'].shape[0])
    rep = lambda x, dim: torch.cat([x] * B_rep, dim)                 # noqa: E731
    inject(model, rep(coin, 1), rep(noise, 1))
    with engines() as eng:
        logp = model(None, rep(t['att'], 0), rep(t['labels'], 0)[..., :-1], rep(t['att_masks'], 0))
    return d, t, eng[0].it_all.cpu(), logp.detach().cpu()


@pytest.mark.parametrize('planes,slabs', [(None, True), ('0', True), (None, False)])
def test_aoa_routes_feed_the_same_tokens(planes, slabs, monkeypatch):
    """planes + folded embedding (default), no planes, planes with the separate embedding launch: each passes the fixture's bounds"""
    d, t, it_all, logp = _aoa_injected(monkeypatch, planes, slabs)
    assert torch.equal(it_all[:t['fed'].shape[0]], t['fed'].cpu())
    np.testing.assert_allclose(logp.numpy(), d['logp'], rtol=2e-5, atol=5e-6)


def test_aoa_more_than_64_rows(monkeypatch):
    """72 rows (the fixture's 6 rows twelve times): no activation planes, the embedding launch reads the select's token"""
    d, t, it_all, logp = _aoa_injected(monkeypatch, None, True, B_rep=12)
    T_eff = t['fed'].shape[0]
    assert it_all.shape[1] == 72
    assert torch.equal(it_all[:T_eff], torch.cat([t['fed'].cpu()] * 12, 1))
    np.testing.assert_allclose(logp.numpy(), np.concatenate([d['logp']] * 12, 0), rtol=2e-5, atol=5e-6)


# ------------------------------------------------------------------------------------------------ 6. Philox route, identities
def _many_rows(family, B=512, n=4, T=5, seed=21):
    d, P, t, model = tiny_model(family)
    g = torch.Generator().manual_seed(seed)
    fc = torch.randn(B, 20, generator=g).clamp_min(0).to(DEV)
    att = torch.randn(B, 6, 20, generator=g).clamp_min(0).to(DEV)
    labels = torch.randint(1, 31, (B, n, T + 1), generator=g)
    labels[..., 0] = 0
    return model, fc, att, labels.to(DEV)


@pytest.mark.parametrize('family', ['newfc', 'aoa'])
def test_philox_draws_follow_the_previous_steps_distribution(family):
    """no hooks, ss_prob 1: every input after position 0 is a draw, so the tokens fed at step 1 are distributed as exp(logp[:, 0]);
    per token, |count - sum of probabilities| within 5 standard deviations of the Poisson-binomial"""
    model, fc, att, labels = _many_rows(family)
    model.train()
    model.ss_prob = 1.0
    torch.manual_seed(5)
    with engines() as eng:
        logp = model(fc, att, labels, None)
    it1 = eng[0].it_all[1].cpu()
    p = logp.detach()[:, 0].double().exp().cpu()                       # [N, V1]
    N, V1 = p.shape
    assert N == 2048 and abs(float(p.sum()) - N) < 1e-3 * N
    count = torch.bincount(it1, minlength=V1).double()
    mean, std = p.sum(0), (p * (1 - p)).sum(0).sqrt()
    assert bool(((count - mean).abs() <= 5 * std + 1e-9).all()), ((count - mean) / std).abs().max()
    assert int((it1 != labels.reshape(N, -1)[:, 1].cpu()).sum()) > N // 2       # draws, not labels
    # later steps draw too (and differ between rows of one image: per-row streams)
    assert int((eng[0].it_all[2].cpu() != labels.reshape(N, -1)[:, 2].cpu()).sum()) > N // 2


@pytest.mark.parametrize('family', ['newfc', 'aoa'])
def test_ss_prob_zero_and_eval_mode_run_the_plain_rollout(family, monkeypatch):
    no_hardcoded_dropout(monkeypatch)
    d, P, t, model = tiny_model(family)
    args = forward_args(family, t)
    seen = []
    run = model._run

    def spy(cfg, *a, **kw):
        seen.append('ss_mode' in cfg)
        return run(cfg, *a, **kw)
    model._run = spy
    model.train()
    model.ss_prob = 0.0
    plain = model(*args).detach().clone()
    assert seen == [False]
    # all coins tails: the scheduled-sampling launches with every row on its label -- the same bits
    model.ss_prob = 0.5
    T_eff, N = t['fed'].shape
    inject(model, torch.zeros(T_eff, N, dtype=torch.bool), torch.zeros(T_eff, N, P['logit.weight'].shape[0]))
    with engines() as eng:
        forced = model(*args).detach().clone()
    assert seen == [False, True]
    assert torch.equal(eng[0].it_all[:T_eff].cpu(), t['labels'].cpu()[..., :-1].reshape(N, -1)[:, :T_eff].t())
    assert torch.equal(plain, forced)
    # eval mode ignores ss_prob
    model.eval()
    with torch.no_grad():
        a = model(*args).clone()
        model.ss_prob = 0.0
        b = model(*args).clone()
    assert seen == [False, True, False, False]
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. contracts
def test_newfc_ss_mode_without_teacher_is_einval():
    from imagecaptioning.pytorch_amd import _lib, newfc_engine
    d, P, t, model = tiny_model('newfc')
    Pd = {k: v.detach() for k, v in model.named_parameters()}
    ro = newfc_engine.Rollout(Pd, t['fc'], n=2, T=4, L=4, mode='greedy')
    ss = torch.full((4, 6), 2, dtype=torch.uint8, device=DEV)
    ro.r.ss_mode = ss.data_ptr()
    rc = _lib.lib.capmi_newfc_rollout_fwd(C.byref(ro.w), C.byref(ro.r), _lib.stream_ptr())
    assert rc == _lib.EINVAL
    with pytest.raises(AssertionError):
        newfc_engine.Rollout(Pd, t['fc'], n=2, T=4, L=4, mode='greedy', ss_mode=ss)


def test_logsoftmax_select_refuses_a_malformed_ss_mode():
    from imagecaptioning.pytorch_amd import _lib, ops
    N, V1, L = 6, 32, 4
    logits = torch.randn(N, V1, device=DEV)
    forced = torch.randint(1, V1, (N, L), device=DEV)
    seq = torch.zeros(N, L, dtype=torch.long, device=DEV)
    it, unf = torch.zeros(N, dtype=torch.long, device=DEV), torch.ones(N, dtype=torch.uint8, device=DEV)
    slp, sel, live = torch.zeros(N, L, V1, device=DEV), torch.zeros(N, L, device=DEV), torch.zeros(N, L, dtype=torch.uint8, device=DEV)

    def call(ss, f=forced):
        ops.logsoftmax_select(logits, 0, L, 2, 1.0, None, 1, None if f is None else f[:, 1:], 1, seq, it, unf, slp, sel, live, ss_mode=ss)
    for bad in (torch.full((N,), 2, dtype=torch.int32, device=DEV), torch.full((N + 1,), 2, dtype=torch.uint8, device=DEV),
                torch.full((1, N), 2, dtype=torch.uint8, device=DEV), torch.full((N,), 2, dtype=torch.uint8), [2] * N):
        with pytest.raises(_lib.CapmiError):
            call(bad)
    with pytest.raises(_lib.CapmiError):
        call(torch.full((N,), 2, dtype=torch.uint8, device=DEV), f=None)
    # a well-formed one: rows on mode 2 take forced[:, 1], rows on mode 1 the arg-max of logits + noise
    ss = torch.tensor([2, 1, 2, 1, 1, 2], dtype=torch.uint8, device=DEV)
    noise = torch.zeros(N, V1, device=DEV)
    noise[:, 7] = 1e4
    ops.logsoftmax_select(logits, 0, L, 2, 1.0, noise, 1, forced[:, 1:], 1, seq, it, unf, slp, sel, live, ss_mode=ss)
    want = torch.where(ss == 1, torch.full_like(forced[:, 1], 7), forced[:, 1])
    assert torch.equal(it, want)
    assert float((slp[:, 0] - torch.log_softmax(logits, 1)).abs().max()) < 1e-5
    assert torch.equal(unf, torch.ones_like(unf))


# ------------------------------------------------------------------------------------------------ 8. tools/train.py
@pytest.mark.parametrize('model_args', [['--caption_model', 'newfc'], ['--caption_model', 'aoa', '--num_heads', '4', '--num_layers', '2']])
def test_train_runs_through_the_scheduled_sampling_epochs(model_args, tmp_path):
    """the schedule of test_entrypoints_gpu.test_train_with_scheduled_sampling: ss_prob rises with the epoch, reaches the model and
    the XE iterations run with sampled inputs -- launch by launch, never as a replayed graph"""
    import pickle
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import train as T
    from imagecaptioning.pytorch_amd import graph_step
    small = model_args + ['--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--fc_feat_size', '24',
                          '--att_feat_size', '24', '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6', '--max_length', '6',
                          '--batch_size', '4', '--seq_per_img', '2', '--synthetic_images', '8', '--checkpoint_path', str(tmp_path),
                          '--scheduled_sampling_start', '0', '--scheduled_sampling_increase_every', '1',
                          '--scheduled_sampling_increase_prob', '0.2', '--scheduled_sampling_max_prob', '0.5',
                          '--losses_log_every', '1', '--save_checkpoint_every', '10']
    opt = opts.parse_opt(small + ['--max_iters', '10'])          # 2 iterations per epoch -> epochs 0..4
    calls = []
    orig = graph_step.TrainStep.__call__

    def spy(self, *a, **kw):
        before = self.replays
        r = orig(self, *a, **kw)
        calls.append((float(getattr(self.model, 'ss_prob', 0.0)), self.replays - before))
        return r
    graph_step.TrainStep.__call__ = spy
    try:
        loss = T.train(opt)
    finally:
        graph_step.TrainStep.__call__ = orig
    assert loss == loss and abs(loss) != float('inf')
    assert opt.ss_prob == pytest.approx(0.5)             # min(0.2 * 4, 0.5) at epoch 4
    assert len(calls) == 10
    sampled = [c for c in calls if c[0] > 0]
    assert len(sampled) == 8 and all(r == 0 for _, r in sampled), calls
    infos = pickle.load(open(tmp_path / 'infos_capmi.pkl', 'rb'))
    hist = [infos['histories']['ss_prob_history'][i] for i in range(10)]
    assert hist == sorted(hist) and hist[0] == 0.0 and hist[-1] == pytest.approx(0.5) and len(set(hist)) >= 4, hist
