"""use_bn (BatchNorm1d around att_embed, AttModel.py:80-85) on a real MI355X.

* the kernels of region_norm.hip alone against float64 on the same inputs.  Bound per quantity: 4 x the error of torch's own CPU
  float32 F.batch_norm against float64 on these inputs (the summation order differs, nothing ties ours to ATen's), floor 1e-6
  relative to the largest element (the floor of test_optim_gpu.py);
* the reference's fixture (tests/golden/use_bn_tiny_*.npz, truth = its float64 arrays): three train-mode XE steps, eval XE, greedy,
  beam 3, a train-mode step with the recorded dropout masks -- plain and flatten_parameters_(), both families, use_bn 1 and 2.
  Bounds of test_att2in2_gpu.py (log-probs rtol 2e-5 / atol 5e-6, loss 1e-5, gradients rtol 5e-4 / atol 1e-6 + 2e-5 max|ref|); where
  the reference's own float32-vs-float64 difference stored in the fixture exceeds a bound, 4 x that difference takes its place
  (check(): per element the larger of the two.  Needed by the log-probs of every pass -- the reference's own float32 run is up to 6.7e-5
  from its float64 run there (updown use_bn 1, dropout step), 13 x the atol -- and by small elements of gradients in every pass; the losses
  and the running buffers keep the stated bounds);
* the SCST ordering of the fused rollout; eval-mode prefills (_prepare_feature, the host-stepped greedy decode on the family's stepper
  == the one-call greedy, an ensemble);
* XE and SCST with injected Gumbel noise at a mid size (D = 2053) against the float64 restatement; a tools/train.py round trip.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import use_bn_ref64 as ref
from test_use_bn_host import CONFIGS, fixture, opt_, state_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS, MOM = 1e-5, 0.1


# ---------------------------------------------------------------------------------------------- the kernels alone
def kernel_inputs(M_kind, D, seed=0):
    """(x [B,K,D], mask [B,K]): clamp_min(0) of a normal plus three hand-made columns -- constant 0, constant 7, mean 100 with
    std 0.01 (the one a one-pass variance gets wrong)"""
    g = torch.Generator().manual_seed(seed)
    if M_kind == 'ragged':
        B, K = 20, 50
        lens = [int(v) for v in torch.randint(20, 51, (B,), generator=g)]         # about 700 valid rows
        lens[3] = K
    else:
        B, K, lens = 1, M_kind, [M_kind]
    x = torch.randn(B, K, D, generator=g).clamp_min(0)
    x[:, :, 1] = 0.0
    x[:, :, 2] = 7.0
    x[:, :, 4] = 100.0 + 0.01 * torch.randn(B, K, generator=g)
    mask = torch.zeros(B, K)
    for b, ln in enumerate(lens):
        mask[b, :ln] = 1
    x = x * (0.5 + mask.unsqueeze(-1))            # padded rows hold other values: they must not count
    return x, mask


def truth_and_bound(x, mask, gamma, beta, steps=3):
    """float64 statistics / running buffers over `steps` calls / output, and per quantity 4 x the error of ATen's CPU float32
    batch_norm against them (floor 1e-6 of the largest element)"""
    xv = x[mask.bool()]
    x64 = xv.double()
    M = x64.shape[0]
    mean, var = x64.mean(0), ((x64 - x64.mean(0)) ** 2).mean(0)
    rstd = 1 / torch.sqrt(var + EPS)
    y = (x64 - mean) * rstd * gamma.double() + beta.double()
    rm, rv = torch.zeros_like(mean), torch.ones_like(mean)
    rm32, rv32 = torch.zeros(x.shape[-1]), torch.ones(x.shape[-1])
    for _ in range(steps):
        rm = (1 - MOM) * rm + MOM * mean
        rv = (1 - MOM) * rv + MOM * var * M / (M - 1)
        y32 = F.batch_norm(xv, rm32, rv32, gamma, beta, True, MOM, EPS)
    mean32, var32 = xv.mean(0), xv.var(0, unbiased=False)
    t = dict(mean=mean, var=var, rstd=rstd, y=y, running_mean=rm, running_var=rv)
    a = dict(mean=mean32, var=var32, rstd=1 / torch.sqrt(var32 + EPS), y=y32, running_mean=rm32, running_var=rv32)
    bound = {k: max(4 * float((a[k].double() - t[k]).abs().max()), 1e-6 * float(t[k].abs().max())) for k in t}
    return t, bound


@pytest.mark.parametrize('D', [20, 37, 2048, 2053])
@pytest.mark.parametrize('M_kind', [2, 3, 65, 'ragged'])
def test_kernels_against_float64(M_kind, D):
    from imagecaptioning.pytorch_amd import ops
    x, mask = kernel_inputs(M_kind, D)
    g = torch.Generator().manual_seed(5)
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    t, bound = truth_and_bound(x, mask, gamma, beta)
    B, K = mask.shape
    xd, md = x.view(B * K, D).to(DEV), mask.view(-1).to(DEV)
    rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    for _ in range(3):
        mean, rstd, count, shift = ops.bn_stats(xd, md, True, rm, rv, nbt)
    y = ops.bn_apply(xd, md, shift, rstd, gamma.to(DEV), beta.to(DEV))
    assert int(nbt) == 3 and float(count) == float(mask.sum())
    var = 1 / rstd.double() ** 2 - EPS
    got = dict(mean=mean, var=var, rstd=rstd, y=y[md.bool()], running_mean=rm, running_var=rv)
    worst = {}                                      # (the biased variance as the consumers see it: 1 / rstd^2 - eps)
    for k in ('mean', 'var', 'rstd', 'y', 'running_mean', 'running_var'):
        worst[k] = float((got[k].double().cpu() - t[k]).abs().max())
        print('bn kernel M=%s D=%d %-12s err %.3e bound %.3e' % (M_kind, D, k, worst[k], bound[k]))
    for k in worst:
        assert worst[k] <= bound[k], (k, worst[k], bound[k])
    assert float(y[~md.bool()].abs().max() if (~md.bool()).any() else 0.0) == 0.0          # padded rows are zero
    # bit-equal on a second call
    mean2, rstd2 = ops.bn_stats(xd, md, True)[:2]
    mean3, rstd3 = ops.bn_stats(xd, md, True)[:2]
    assert torch.equal(mean2, mean3) and torch.equal(rstd2, rstd3) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    # eval: the running statistics, nothing updated
    before = (rm.clone(), rv.clone(), int(nbt))
    mean_e, rstd_e = ops.bn_stats(xd, md, False, rm, rv, nbt)[:2]
    assert torch.equal(mean_e, rm) and torch.equal(rm, before[0]) and torch.equal(rv, before[1]) and int(nbt) == before[2]
    assert float((rstd_e.double() - 1 / torch.sqrt(rv.double() + EPS)).abs().max() / rstd_e.abs().max()) < 1e-6


def test_fewer_than_two_rows_leave_the_buffers_alone():
    from imagecaptioning.pytorch_amd import ops
    x = torch.rand(4, 37, device=DEV)
    for valid in (0, 1):
        mask = torch.zeros(4, device=DEV)
        mask[:valid] = 1
        rm, rv = torch.full((37,), 0.25, device=DEV), torch.full((37,), 2.0, device=DEV)
        nbt = torch.zeros((), dtype=torch.long, device=DEV)
        mean, rstd, count, _ = ops.bn_stats(x, mask, True, rm, rv, nbt)
        assert int(nbt) == 0 and float(count) == valid
        assert torch.equal(rm, torch.full_like(rm, 0.25)) and torch.equal(rv, torch.full_like(rv, 2.0))
        assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
        assert torch.equal(mean, x[0] if valid else torch.zeros_like(mean))


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('D', [37, 2048])
def test_backward_kernels_against_float64_autograd(D, train):
    """bn_backward (the full Jacobian over the valid rows) and bn_linear_bwd (BatchNorm in front of a Linear, from the weight
    gradient on the raw rows) against autograd in float64; 1e-5 of the largest element of each gradient (fp32 sums of <= 700 terms
    of either sign, no cancellation built in: inputs are a plain normal here)"""
    from imagecaptioning.pytorch_amd import ops
    g = torch.Generator().manual_seed(11)
    B, K, R = 6, 9, 24
    x = torch.randn(B, K, D, generator=g).clamp_min(0)
    mask = torch.ones(B, K)
    mask[1, 5:] = 0
    mask[4, 2:] = 0
    rows = mask.view(-1).bool()
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    W, dpre = torch.randn(R, D, generator=g) / D ** 0.5, torch.randn(B * K, R, generator=g) * mask.view(-1, 1)
    rm, rv = 0.3 * torch.rand(D, generator=g), 0.5 + torch.rand(D, generator=g)
    # float64
    x64, ga, be, W64 = x.view(-1, D).double(), gamma.double().requires_grad_(), beta.double().requires_grad_(), W.double().requires_grad_()
    xin = x64.clone().requires_grad_()
    if train:
        mu, var = xin[rows].mean(0), ((xin[rows] - xin[rows].mean(0)) ** 2).mean(0)
    else:
        mu, var = rm.double(), rv.double()
    yy = (xin - mu) / torch.sqrt(var + EPS) * ga + be
    (yy @ W64.t() * dpre.double()).sum().backward()
    dy = (dpre.double() @ W64.detach())
    # device
    d = lambda t: t.contiguous().float().to(DEV)        # noqa: E731
    xd, md = d(x.view(-1, D)), d(mask.view(-1))
    mean, rstd, count, _ = ops.bn_stats(xd, md, train, d(rm), d(rv))
    dg, db = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    dx = ops.bn_backward(d(dy), xd, md, mean, rstd, d(gamma), count, train, dg, db)
    rel = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())          # noqa: E731
    assert rel(dg, ga.grad) < 1e-5 and rel(db, be.grad) < 1e-5
    assert rel(dx, xin.grad * mask.view(-1, 1).double()) < 1e-5
    G = d(dpre.t().double() @ x64)                      # the weight gradient on the RAW rows
    bias_g = d(dpre.double().sum(0))
    dg2, db2 = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    ops.bn_linear_bwd(G, bias_g, d(W), mean, rstd, d(gamma), d(beta), dg2, db2)
    assert rel(G, W64.grad) < 1e-5 and rel(dg2, ga.grad) < 1e-5 and rel(db2, be.grad) < 1e-5


# ---------------------------------------------------------------------------------------------- the reference's fixture
def golden_model(family, use_bn, flatten=False, **kw):
    from imagecaptioning.pytorch_amd.captioning import models
    z = fixture(family, use_bn)
    model = models.setup(opt_(family, use_bn, **kw))
    model.load_state_dict(state_of(z), strict=True)
    model = model.to(DEV)
    if flatten:
        model.flatten_parameters_()
    return z, model, (lambda k: torch.from_numpy(z[k]).to(DEV))


def bound_for(z, key, bound):
    """the stated bound, or 4 x the reference's own float32-vs-float64 difference where that is larger"""
    return max(bound, 4 * float(z[key + '@d']))


def check(z, key, got, rtol, atol):
    r = z[key + '@64']
    got = got.detach().double().cpu().numpy()
    tol = bound_for(z, key, 0.0)
    err = np.abs(got - r)
    lim = np.maximum(atol + rtol * np.abs(r), tol)
    assert (err <= lim).all(), (key, float(err.max()), float(lim.min()))


def xe_pass(z, model, t, tag, att, att_masks):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    labels, masks = t('labels'), t('masks')
    logp = model(t('fc').float(), att.float(), labels[..., :-1], att_masks.float())
    check(z, tag + '_logp', logp, 2e-5, 5e-6)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:].float())
    check(z, tag + '_loss', loss, 1e-5, 0.0)
    model.zero_grad()
    loss.backward()
    for k, p in model.named_parameters():
        r = z[tag + '_grad.' + k + '@64']
        check(z, tag + '_grad.' + k, p.grad, 5e-4, 1e-6 + 2e-5 * float(np.abs(r).max()))


def check_buffers(z, model, tag):
    for k, v in model.state_dict().items():
        if 'running_' in k:
            r = z['%s_buf.%s@64' % (tag, k)]
            check(z, '%s_buf.%s' % (tag, k), v, 5e-4, 1e-6 + 2e-5 * float(np.abs(r).max()))
        elif 'num_batches' in k:
            assert int(v) == int(z['%s_buf.%s' % (tag, k)]), k


@pytest.mark.parametrize('flatten', [False, True])
@pytest.mark.parametrize('family,use_bn', CONFIGS)
def test_golden_train_steps_eval_xe_greedy_and_beam3(family, use_bn, flatten):
    z, model, t = golden_model(family, use_bn, flatten)
    model.train()                  # drop_prob_lm 0: dropout is the identity
    for s in range(3):
        xe_pass(z, model, t, 'train%d' % s, t('att%d' % s), t('att_masks'))
        check_buffers(z, model, 'train%d' % s)
    model.eval()
    xe_pass(z, model, t, 'eval', t('att0'), t('att_masks'))
    with torch.no_grad():
        fc, att, am = t('fc').float(), t('att0').float(), t('att_masks').float()
        seq, slp = model(fc, att, am, opt={'sample_method': 'greedy'}, mode='sample')
        assert np.array_equal(seq.cpu().numpy(), z['greedy_seq'])
        check(z, 'greedy_logp', slp, 2e-5, 5e-6)
        seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1}, mode='sample')
        assert np.array_equal(seq.cpu().numpy(), z['beam3_seq'])
        check(z, 'beam3_logp', slp, 2e-5, 5e-6)
    check_buffers(z, model, 'train2')          # the eval passes updated nothing


@pytest.mark.parametrize('flatten', [False, True])
@pytest.mark.parametrize('family,use_bn', CONFIGS)
def test_golden_train_step_with_recorded_dropout_masks(family, use_bn, flatten):
    z, model, t = golden_model(family, use_bn, flatten, drop_prob_lm=0.5)
    # the running buffers the reference had before this step: those behind its three train steps
    model.load_state_dict({k: torch.from_numpy(z['train2_buf.' + k + ('' if 'num_batches' in k else '@64')]).float()
                           if 'running_' in k else (torch.from_numpy(z['train2_buf.' + k]) if 'num_batches' in k else v)
                           for k, v in model.state_dict().items()}, strict=True)
    keep = lambda k: (torch.from_numpy(z[k].astype(np.float32)) / 0.5).to(DEV).contiguous()      # noqa: E731
    masks = dict(drop_att=keep('drop.att'), drop_xt=keep('drop.xt'), drop_out=keep('drop.out'))
    if family == 'updown':
        masks['drop_fc'] = keep('drop.fc')
        model._dropout_masks = lambda *a, **k: dict(masks)
    else:
        model._drop_masks = masks
    model.train()
    xe_pass(z, model, t, 'drop', t('att1'), t('att_masks'))
    check_buffers(z, model, 'drop')


# ---------------------------------------------------------------------------------------------- SCST ordering, eval prefills
def far_model(use_bn, seed=3):
    """a model whose running buffers are far from the statistics of its batch"""
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(seed)
    model = models.setup(opt_('updown', use_bn))
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.3 * torch.randn_like(p))
        for m in model.att_embed:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.fill_(2.0)
                m.running_var.fill_(9.0)
    g = torch.Generator().manual_seed(seed + 1)
    B, K = 4, 7
    fc, att = torch.randn(B, 20, generator=g).clamp_min(0), torch.randn(B, K, 20, generator=g).clamp_min(0)
    am = torch.ones(B, K)
    am[0, 4:] = 0
    am[2, 6:] = 0
    return model.to(DEV), fc.to(DEV), att.to(DEV), am.to(DEV)


@pytest.mark.parametrize('use_bn', [1, 2])
def test_scst_rollouts_greedy_half_reads_the_old_running_statistics(use_bn):
    model, fc, att, am = far_model(use_bn)
    model.eval()
    with torch.no_grad():
        greedy_before, _ = model(fc, att, am, opt={'sample_method': 'greedy'}, mode='sample')
    state = {k: v.clone() for k, v in model.state_dict().items()}
    # one train-mode update in float64
    P = ref.p64(state)
    new = {}
    ref.att_embed(P, att, am, train=True, new_bufs=new)
    model.train()
    greedy_res, gen, logp = model.scst_rollouts(fc, att, am, sample_n=3)
    assert torch.equal(greedy_res, greedy_before)
    after = model.state_dict()
    for k, v in new.items():
        if 'num_batches' in k:
            assert int(after[k]) == int(state[k]) + 1
        else:
            assert float((after[k].double().cpu() - v.cpu()).abs().max()) <= 1e-6 * float(v.abs().max()) + 1e-7, k
    # and the sampled half saw BATCH statistics: a second call with other running buffers gives the same sampled log-probs
    model2, _, _, _ = far_model(use_bn)
    model2.train()
    g = torch.Generator(device='cpu').manual_seed(9)
    gum = -torch.log(-torch.log(torch.rand(8, 4 * 3 + 4, 31, generator=g))).to(DEV)
    with torch.no_grad():
        for m in model2.att_embed:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.fill_(-1.0)
                m.running_var.fill_(0.25)
    model3, _, _, _ = far_model(use_bn)
    model3.train()
    _, gen2, lp2 = model2.scst_rollouts(fc, att, am, sample_n=3, _gumbel=gum)
    _, gen3, lp3 = model3.scst_rollouts(fc, att, am, sample_n=3, _gumbel=gum)
    assert torch.equal(gen2, gen3) and torch.equal(lp2.detach(), lp3.detach())


@pytest.mark.parametrize('family,use_bn', CONFIGS)
def test_eval_prefills_update_nothing_and_agree(family, use_bn):
    """_prepare_feature, the stepper's greedy decode against the one-call greedy, an AttEnsemble of two use_bn members"""
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    z, model, t = golden_model(family, use_bn)
    z2, model2, _ = golden_model(family, use_bn)
    fc, att, am = t('fc').float(), t('att0').float(), t('att_masks').float()
    model.train()                                   # even in train mode these are eval-mode prefills
    before = {k: v.clone() for k, v in model.state_dict().items()}
    P = ref.p64(state_of(z))
    a64, p64_, _ = ref.att_embed({k: v.to(DEV) for k, v in P.items()}, att, am, train=False)
    _, a, p_att, _ = model._prepare_feature(fc, att, am)
    assert float((a.double() - a64).abs().max()) < 1e-5 * float(a64.abs().max())
    assert float((p_att.double() - p64_).abs().max()) < 1e-5 * float(p64_.abs().max())
    model.eval()
    with torch.no_grad():
        seq, slp = model(fc, att, am, opt={'sample_method': 'greedy'}, mode='sample')
        # the host-stepped decoder on the family's stepper (what decode options, beam search and ensembles run), plain greedy
        from imagecaptioning.pytorch_amd import decode
        model.train()                               # the stepper's prefill is an eval-mode one whatever the module's mode
        make = model._stepper(*model._feeds(fc, att, am))
        model.eval()
        seq_s, slp_s = decode.sample_steps(model, make(1), fc.shape[0], model.seq_length, {'sample_method': 'greedy'}, fc.device)
        ens = AttEnsemble([model, model2], weights=None)
        ens.eval()
        seq_e, _ = ens(fc, att, am, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')
    assert torch.equal(seq_s, seq)
    np.testing.assert_allclose(slp_s.cpu().numpy(), slp.cpu().numpy(), rtol=2e-5, atol=5e-6)
    assert torch.equal(seq_e, seq)                  # two equal members decode like one
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k


# ---------------------------------------------------------------------------------------------- mid size against the restatement
MID = dict(V=200, input_encoding_size=64, rnn_size=64, att_hid_size=64, fc_feat_size=48, att_feat_size=2053, seq_length=12,
           max_length=12)
MID_SEED = {'updown': 0, 'att2in2': 0}      # seeds whose float64 pre-activations leave <= 64 // 20 units within 1e-4 of a ReLU edge


def mid_setup(family, dev):
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(MID_SEED[family])
    o = opt_(family, 2)
    for k, v in MID.items():
        setattr(o, 'vocab_size' if k == 'V' else k, v)
    o.vocab = {str(i): 'w%d' % i for i in range(1, MID['V'] + 1)}
    model = models.setup(o)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    g = torch.Generator().manual_seed(MID_SEED[family] + 1)
    B, K, n, T = 10, 36, 5, 12
    att = torch.randn(B, K, 2053, generator=g).clamp_min(0)
    am = torch.ones(B, K)
    for b in range(B):
        am[b, 10 + (b * 7) % 27:] = 0
    am[3] = 1
    fc = torch.randn(B, 48, generator=g).clamp_min(0)
    labels = torch.zeros(B, n, T + 2, dtype=torch.long)
    for b in range(B):
        for j in range(n):
            ln = int(torch.randint(4, T, (1,), generator=g))
            labels[b, j, 1:1 + ln] = torch.randint(1, MID['V'] + 1, (ln,), generator=g)
    masks = (labels > 0).float()
    masks[..., :2] = 1
    return model.to(dev), fc.to(dev), att.to(dev), am.to(dev), labels.to(dev), masks.to(dev)


def edge_units(P, att, am):
    """att_embed units whose float64 pre-activation lies within 1e-4 of zero for some valid region: there the float32 and the
    float64 ReLU gates may differ (check_rel of test_att2in2_gpu.py)"""
    B, K, C = att.shape
    valid = am.reshape(-1) > 0
    x = ref.batch_norm(att.double().reshape(B * K, C), valid, P, 'att_embed.0', True, None)
    pre = x @ P['att_embed.1.weight'].t() + P['att_embed.1.bias']
    return (pre.detach().abs() < 1e-4)[valid].any(0)


def rel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


def check_rel(model, P, att, am):
    """every gradient within 1e-3 of the float64 restatement's, relative to its largest element (check_rel of test_att2in2_gpu.py).
    Units of att_embed's Linear (and of the BatchNorm behind it) with a pre-activation within 1e-4 of zero are left out of those
    layers' comparison, at most 1/20 of the units: asserted here for the seed in use."""
    edge = edge_units(P, att, am)
    assert int(edge.sum()) <= 64 // 20, int(edge.sum())
    keep = ~edge
    for k, p in model.named_parameters():
        a, b = p.grad, P[k].grad
        if k == 'core.attention.alpha_net.bias':     # exactly 0 (the softmax is shift invariant): compare absolutely
            assert float(a.abs().max()) < 1e-6 and float(b.abs().max()) < 1e-9, k
            continue
        if k.startswith('att_embed.1.') or k.startswith('att_embed.4.'):
            a, b = a[keep], b[keep]
        assert rel(a, b) < 1e-3, (k, rel(a, b))


def check_new_buffers(model, new):
    """the running buffers after ONE train-mode update against the restatement's"""
    after = model.state_dict()
    for k, v in new.items():
        if 'num_batches' in k:
            assert int(after[k]) == 1, k
        else:
            assert rel(after[k], v) < 1e-5, k


@pytest.mark.parametrize('family', ['updown', 'att2in2'])
def test_mid_size_scst_with_injected_gumbel_vs_restatement(family):
    """The same size, SCST: the sampled rows with injected Gumbel noise in train mode (batch statistics, one update of the running
    buffers; drop_prob_lm 0) -- UpDown through the fused scst_rollouts, whose greedy half must equal an eval-mode greedy decode on the
    OLD running statistics; Att2in2 through _sample.  Tokens equal the restatement's arg-max, log-probs within 1e-4, RewardCriterion
    loss and every gradient by check_rel."""
    from imagecaptioning.pytorch_amd.captioning.modules.losses import RewardCriterion
    model, fc, att, am, _, _ = mid_setup(family, DEV)
    with torch.no_grad():              # running statistics far from the batch's: the two halves must not be confused
        for m in model.att_embed:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.fill_(0.5)
                m.running_var.fill_(4.0)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    B, n, L, V1 = 10, 5, 12, MID['V'] + 1
    N = B * n
    gum = -torch.log(-torch.log(torch.rand(L, N + B, V1, generator=torch.Generator().manual_seed(5)).clamp(1e-10, 1 - 1e-7)))
    gum = gum.to(DEV)
    reward = torch.randn(N, 1, generator=torch.Generator().manual_seed(6)).repeat(1, L).to(DEV)
    if family == 'updown':
        model.eval()
        with torch.no_grad():
            greedy_before, _ = model(fc, att, am, opt={'sample_method': 'greedy'}, mode='sample')
        model.train()
        greedy_res, seq, slp = model.scst_rollouts(fc, att, am, sample_n=n, _gumbel=gum)
        assert torch.equal(greedy_res, greedy_before)
        g_ref = gum[:, :N]
    else:
        model.train()
        g_ref = gum[:, :N].contiguous()
        seq, slp = model(fc, att, am, opt={'sample_method': 'sample', 'sample_n': n, '_gumbel': g_ref}, mode='sample')
    loss = RewardCriterion()(slp, seq, reward)
    model.zero_grad()
    loss.backward()
    P = ref.p64(state, grad=True)
    new = {}
    seq_r, slp_r = ref.greedy(family, P, fc, att, am, L, n=n, gumbel=g_ref, train=True, new_bufs=new)
    assert torch.equal(seq, seq_r), 'sampled tokens differ'
    assert float((slp.detach().double() - slp_r.detach()).abs().max()) < 1e-4
    sel = slp_r.gather(2, seq_r.unsqueeze(2)).squeeze(2)
    m = torch.cat([torch.ones(N, 1, dtype=ref.D, device=DEV), (seq_r > 0).double()[:, :-1]], 1)
    loss_r = -(sel * reward.double() * m).sum() / m.sum()
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, att, am)
    check_new_buffers(model, new)
    if family == 'updown':             # and the greedy half is the restatement's eval-mode decode on the old buffers
        seq_g, _ = ref.greedy(family, ref.p64(state), fc, att, am, L)
        assert torch.equal(greedy_res, seq_g)


@pytest.mark.parametrize('family', ['updown', 'att2in2'])
def test_mid_size_xe_vs_restatement(family):
    """R = E = A = 64, D = 2053, K = 36 ragged, B = 10, n = 5, V = 200, use_bn 2, train mode: log-probs, loss, every gradient within
    1e-3 of the float64 restatement's, relative to its largest element; the running buffers after the step"""
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    model, fc, att, am, labels, masks = mid_setup(family, DEV)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    logp = model(fc, att, labels[..., :-1], am)
    loss = LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    model.zero_grad()
    loss.backward()
    P = ref.p64(state, grad=True)
    new = {}
    logp_r = ref.xe(family, P, fc, att, am, labels[..., :-1], train=True, new_bufs=new)
    loss_r = ref.lm_loss(logp_r, labels, masks)
    loss_r.backward()
    assert float((logp.detach().double() - logp_r.detach()).abs().max()) < 1e-4
    assert abs(loss.item() - loss_r.item()) < 1e-4
    check_rel(model, P, att, am)
    check_new_buffers(model, new)


def test_tools_train_xe_then_resume_into_self_critical(tmp_path):
    """tools/train.py on synthetic data with use_bn 2: XE, then --start_from resume into self-critical.  The running buffers
    travel through model.pth and survive the resume (num_batches_tracked goes on counting), losses finite, the XE loss falls."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd'))
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import opts, rewards
    small = ['--caption_model', 'updown', '--use_bn', '2', '--rnn_size', '64', '--input_encoding_size', '64', '--att_hid_size', '32',
             '--fc_feat_size', '48', '--att_feat_size', '48', '--vocab_size', '60', '--synthetic_regions', '7', '--seq_length', '8',
             '--max_length', '8', '--batch_size', '4', '--seq_per_img', '3', '--synthetic_images', '16', '--losses_log_every', '2',
             '--checkpoint_path', str(tmp_path)]
    l0 = T.train(opts.parse_opt(small + ['--max_iters', '1']))
    l1 = T.train(opts.parse_opt(small + ['--max_iters', '30', '--save_checkpoint_every', '30', '--learning_rate', '0.01',
                                         '--reduce_on_plateau', '0']))
    assert np.isfinite(l0) and np.isfinite(l1)
    assert l1 < l0, 'XE loss should fall on a 16-image synthetic set (%.3f -> %.3f)' % (l0, l1)
    sd = torch.load(os.path.join(str(tmp_path), 'model.pth'), map_location='cpu')
    assert int(sd['att_embed.0.num_batches_tracked']) == 30 and int(sd['att_embed.4.num_batches_tracked']) == 30
    assert float(sd['att_embed.0.running_mean'].abs().max()) > 0 and torch.isfinite(sd['att_embed.4.running_var']).all()
    rewards.reset_scorer()
    l2 = T.train(opts.parse_opt(small + ['--max_iters', '33', '--self_critical_after', '0', '--train_sample_n', '3',
                                         '--save_checkpoint_every', '33', '--start_from', str(tmp_path)]))
    assert np.isfinite(l2)
    sd2 = torch.load(os.path.join(str(tmp_path), 'model.pth'), map_location='cpu')
    assert int(sd2['att_embed.0.num_batches_tracked']) == 33          # resumed at 30, one update per self-critical step
    assert not torch.equal(sd2['att_embed.0.running_mean'], sd['att_embed.0.running_mean'])
