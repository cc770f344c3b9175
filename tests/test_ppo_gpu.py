"""The PPO structure loss on the MI355X: capmi_ppo_loss_fwd / _bwd against the fp64 restatement (tests/ppo_ref64.py), the fused
route of PPOLoss against its generic route through a real rollout backward, the repo's old models against the reference's recorded
PPOLoss (tests/golden/make_ppo.py), the identity invariant (old model == live model), TrainStep and tools/train.py with use_ppo."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from ppo_ref64 import ppo64
from test_model_api_gpu import tiny_opt, DEV

pytestmark = pytest.mark.gpu
Z = os.path.join(GOLDEN, 'ppo_tiny.npz')
KW = {'updown': {}, 'transformer': dict(caption_model='transformer', N_enc=2, N_dec=2, d_model=16, d_ff=32, num_att_heads=2,
                                         dropout=0.0)}


# ---------------------------------------------------------------------------------------------------------------- the kernels
def _inputs(N, L, V1, n, seed):
    """fp32 device inputs: old rows, new rows near them, ragged tokens (an all-zero row, a row with no end token), scores with an
    image whose samples all score the same (advantage 0)"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.log_softmax(2 * torch.randn(N, L, V1, generator=g), 2)
    ln = torch.log_softmax(lo + 0.3 * torch.randn(N, L, V1, generator=g), 2)
    seq = torch.randint(1, V1 + 1, (N, L), generator=g) % V1 if V1 > 1 else torch.zeros(N, L, dtype=torch.long)
    lens = torch.randint(0, L + 1, (N,), generator=g)
    lens[0], lens[-1] = 0, L
    for i in range(N):
        seq[i, int(lens[i]):] = 0
    scores = torch.rand(N, generator=g)
    scores[:n] = 0.5
    return ln.to(DEV), lo.to(DEV), seq.to(DEV), scores.to(DEV)


def _near_clip(r, eps):
    return ((r - (1 - eps)).abs() < 1e-4) | ((r - (1 + eps)).abs() < 1e-4)


def upstream(N, per_row):
    """the upstream gradient the kernel tests feed the backward: [N] for per_row, else the scalar 0.7"""
    return torch.linspace(0.5, 1.5, N, device=DEV) if per_row else torch.tensor([0.7], device=DEV)


def _check_kernel(ln, lo, seq, scores, n, eps, klc, per_row):
    from imagecaptioning.pytorch_amd import ops
    u = upstream(ln.shape[0], per_row)
    out, loss_rows, rs, msum = ops.ppo_loss_fwd(ln, lo, seq, scores, n, eps, klc, per_row)
    grad = ops.ppo_loss_bwd(lo, seq, rs, msum, u, n, eps, klc, per_row)
    check_against_ppo64(out, loss_rows, rs, grad, ln, lo, seq, scores, n, eps, klc, per_row, u)
    return out, rs, grad


def check_against_ppo64(out, loss_rows, rs, grad, ln, lo, seq, scores, n, eps, klc, per_row, u):
    """what a forward and a backward launch returned (out [4], loss_rows [N] or None, row_stats [4, N, L], grad [N, L, V1], any
    strides) against the fp64 restatement on the same inputs; u as upstream() gives it"""
    torch.cuda.synchronize()
    ref = ppo64(ln, lo, seq, scores, n, eps, klc, per_row, u=(u if per_row else 0.7))
    m = ref['mask'] > 0
    kl, r, pg, gpg = (rs[k].double() for k in range(4))
    far = m & ~_near_clip(ref['r'], eps) & torch.isfinite(ref['r'].float())
    assert bool(((kl - ref['kl']).abs() <= 2e-5 * ref['kl_bound'] + 1e-6)[m].all()), 'kl'
    assert torch.equal(kl[~m], torch.zeros_like(kl[~m])) and torch.equal(gpg[~m], torch.zeros_like(gpg[~m]))
    assert bool(((r - ref['r']).abs() <= 1e-5 * ref['r'].abs())[far].all()), 'r'
    A = ref['pg'].abs().max() + 1e-6
    assert bool(((pg - ref['pg']).abs() <= 1e-5 * ref['pg'].abs() + 1e-6 * A)[far].all()), 'pg'
    assert bool(((gpg - ref['g_pg']).abs() <= 1e-5 * ref['g_pg'].abs() + 1e-6 * A)[far].all()), 'g_pg'
    M = float(m.sum())
    near = float((_near_clip(ref['r'], eps) & m).sum())
    scale = float(ref['kl_bound'][m].mean()) + float(ref['pg'][m].abs().mean()) + 1e-6
    assert abs(float(out[0]) - float(ref['pg_loss'])) <= 1e-5 * scale
    assert abs(float(out[1]) - float(ref['kl_loss'])) <= 2e-5 * scale
    assert abs(float(out[2]) - float(ref['clipfrac'])) <= near / M + 1e-6
    if per_row:
        assert float((loss_rows.double() - ref['loss']).abs().max()) <= 2e-5 * (scale + float(ref['loss'].abs().max()))
    else:
        assert abs(float(out[3]) - float(ref['loss'])) <= 2e-5 * scale
    rowok = far.unsqueeze(2) | ~m.unsqueeze(2)
    gref = ref['grad']
    err = (grad.double() - gref).abs()
    assert bool((err <= 2e-5 * gref.abs() + 1e-6 * float(gref.abs().max()) + 1e-30)[rowok.expand_as(err)].all()), 'grad'
    assert torch.equal(grad[~m], torch.zeros_like(grad[~m]))


@pytest.mark.parametrize('per_row', (False, True))
@pytest.mark.parametrize('N,L,V1', [(6, 1, 1), (6, 2, 3), (50, 22, 5), (6, 1, 11), (9, 4, 11), (640, 21, 11), (12, 5, 4097), (50, 20, 9488)])
def test_kernel_against_fp64(N, L, V1, per_row):
    for eps, klc in ((0.2, 0.02), (0.05, 0.5)):
        ln, lo, seq, scores = _inputs(N, L, V1, 3 if N % 3 == 0 else 2, seed=N * 31 + V1)
        _check_kernel(ln, lo, seq, scores, 3 if N % 3 == 0 else 2, eps, klc, per_row)


@pytest.mark.parametrize('V1', (11, 9488))
def test_kernel_at_the_largest_row_count(V1):
    N, L = 640, 21
    ln, lo, seq, scores = _inputs(N, L, V1, 5, seed=7)
    out, rs, _ = _check_kernel(ln, lo, seq, scores, 5, 0.2, 0.02, False)
    r = rs[1][ref_mask(seq)]
    assert (r < 0.8).any() and (r > 1.2).any()          # clipped on both sides and unclipped rows


def ref_mask(seq):
    from ppo_ref64 import shifted_mask
    return shifted_mask(seq) > 0


def test_kernel_edge_cases():
    """an overflowing ratio with A > 0 (finite loss, zero gradient for its token), with A < 0 (infinite loss); non-finite values
    in masked rows are not read; invalid arguments are refused"""
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import CapmiError
    N, L, V1, n = 4, 3, 37, 2
    ln, lo, seq, _ = _inputs(N, L, V1, n, seed=3)
    seq[:, :] = torch.tensor([[5, 6, 0], [7, 0, 0], [4, 9, 2], [3, 3, 3]], device=DEV)
    scores = torch.tensor([1.0, 0.0, 0.3, 0.6], device=DEV)             # A = +1, -1, -0.3, +0.3
    ln[0, 1, 6] = lo[0, 1, 6] + 100.0                                    # r = exp(100) = inf in fp32, A > 0
    ln[1, 2, :] = float('nan')                                           # masked row (row 1 ended at step 1)
    lo[1, 2, :] = -float('inf')
    out, loss_rows, rs, msum = ops.ppo_loss_fwd(ln, lo, seq, scores, n, 0.2, 0.02, False)
    grad = ops.ppo_loss_bwd(lo, seq, rs, msum, torch.ones(1, device=DEV), n, 0.2, 0.02, False)
    torch.cuda.synchronize()
    assert float(rs[1, 0, 1]) == float('inf') and float(rs[2, 0, 1]) == pytest.approx(-1.2)
    assert float(rs[3, 0, 1]) == 0.0
    assert torch.isfinite(out).all(), out
    assert torch.isfinite(grad).all()
    g = grad[0, 1]
    assert float(g[6]) == pytest.approx(-0.02 / float(msum[0]) * float(lo[0, 1, 6].exp()), rel=1e-5)
    assert torch.equal(grad[1, 2], torch.zeros(V1, device=DEV))
    # A < 0 with the same overflow: the unclipped side -A r = +inf wins
    scores2 = torch.tensor([0.0, 1.0, 0.3, 0.6], device=DEV)
    out2, _, _, _ = ops.ppo_loss_fwd(ln, lo, seq, scores2, n, 0.2, 0.02, False)
    assert float(out2[0]) == float('inf')
    for bad in (dict(n=1), dict(n=3)):
        with pytest.raises(CapmiError):
            ops.ppo_loss_fwd(ln, lo, seq, scores, bad['n'], 0.2, 0.02, False)
    with pytest.raises(CapmiError):
        ops.ppo_loss_fwd(ln, lo, seq, scores, n, -0.1, 0.02, False)
    with pytest.raises(CapmiError):
        ops.ppo_loss_fwd(ln.double(), lo, seq, scores, n, 0.2, 0.02, False)
    with pytest.raises(CapmiError):
        ops.ppo_loss_fwd(ln.transpose(0, 1).contiguous().transpose(0, 1), lo, seq, scores, n, 0.2, 0.02, False)
    with pytest.raises(CapmiError):
        ops.ppo_loss_fwd(ln.cpu(), lo, seq, scores, n, 0.2, 0.02, False)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- models
def family_model(fam, perturb=0.0, seed=0):
    from imagecaptioning.pytorch_amd.captioning import models
    z = np.load(os.path.join(GOLDEN, fam + '_tiny.npz'))
    model = models.setup(tiny_opt(**KW[fam]))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('P.')}
    if perturb:
        g = torch.Generator().manual_seed(seed)
        sd = {k: v + perturb * torch.randn(v.shape, generator=g) * (v.std() if v.numel() > 1 else 0.0) for k, v in sd.items()}
    model.load_state_dict(sd)
    return model.to(DEV)


def _ppo(fam, path, **kw):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    opt = tiny_opt(**KW[fam], use_ppo=1, ppo_old_model_path=path, train_sample_n=3, **kw)
    return losses.PPOLoss(opt, family_model(fam))


def _feats():
    u = np.load(os.path.join(GOLDEN, 'updown_tiny.npz'))
    return tuple(torch.from_numpy(u[k]).to(DEV) for k in ('fc', 'att', 'att_masks'))


@pytest.mark.parametrize('red', ('mean', 'none'))
@pytest.mark.parametrize('fam', ('updown', 'transformer'))
def test_repo_old_model_matches_reference_fixture(fam, red, tmp_path, monkeypatch):
    """the repo's UpDown / Transformer as the old model (the fixture's weights through a checkpoint), the fused route: the reference
    PPOLoss's outputs and input gradient to fp32-grade tolerance"""
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    z = np.load(Z)
    path = str(tmp_path / 'old.pth')
    torch.save(family_model(fam).state_dict(), path)
    seq = torch.from_numpy(z[fam + '_seq']).to(DEV)
    scores = torch.from_numpy(z[fam + '_scores']).float().to(DEV)
    monkeypatch.setattr(losses, 'get_scores', lambda gts, s, opt, as_tensor=False: scores)
    fc, att, am = _feats()
    for tag, eps, klc in (('e2k2', 0.2, 0.02), ('e05k50', 0.05, 0.5)):
        crit = _ppo(fam, path, ppo_cliprange=eps, ppo_kl_coef=klc)
        lo = crit.old_logprobs(fc, att, seq, am)
        m = ref_mask(seq.cpu()).numpy()                  # (rows past the end may differ between the families' early stops)
        np.testing.assert_allclose(lo.cpu().numpy()[m], z[fam + '_old_logp'][m], atol=5e-5, rtol=0)
        x = torch.from_numpy(z[fam + '_input']).float().to(DEV).requires_grad_(True)
        o = crit(x, seq, [None] * 3, fc, att, am, reduction=red)
        u = torch.from_numpy(z[fam + '_u']).float().to(DEV)
        (o['loss'] if red == 'mean' else (o['loss'] * u).sum()).backward()
        key = '%s_%s_%s_' % (fam, tag, red)
        for k in ('loss', 'pg_loss', 'kl_loss', 'clipfrac', 'reward'):
            np.testing.assert_allclose(o[k].detach().cpu().numpy(), z[key + k], atol=2e-5, rtol=1e-4, err_msg=key + k)
        np.testing.assert_allclose(x.grad.cpu().numpy(), z[key + 'grad'], atol=5e-6, rtol=1e-4, err_msg=key + 'grad')


def _rollout(model, fc, att, am, seed):
    torch.manual_seed(seed)
    model._rng_calls = 3
    return model(fc, att, am, opt={'sample_method': 'sample', 'beam_size': 1, 'output_logsoftmax': 1, 'sample_n': 3}, mode='sample')


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('red', ('mean', 'none'))
@pytest.mark.parametrize('fam', ('updown', 'transformer'))
def test_fused_route_equals_generic_route(fam, red, tmp_path):
    """same rollout, same old log-probs: the fused route (capmi_ppo_loss_*) and the generic ATen route give the same loss, the same
    d input and, after the rollout backward, the same parameter gradients"""
    path = str(tmp_path / 'old.pth')
    torch.save(family_model(fam, perturb=1.0, seed=1).state_dict(), path)
    crit = _ppo(fam, path, ppo_cliprange=0.02)        # (the tiny models' distributions are flat: ratios stay near 1)
    model = family_model(fam).train()
    fc, att, am = _feats()
    scores = torch.tensor([0.1, 0.9, 0.4, 0.5, 0.5, 0.5, 1.3, 0.2, 0.0], device=DEV)
    res = {}
    for route in ('fused', 'generic'):
        model.zero_grad(set_to_none=True)
        seq, logp = _rollout(model, fc, att, am, seed=11)
        lo = crit.old_logprobs(fc, att, seq, am)
        o = (crit.loss if route == 'fused' else crit.generic)(logp, seq, scores, lo, red)
        assert (type(o['loss'].grad_fn).__name__ == '_FusedPPOBackward') == (route == 'fused')
        loss = o['loss'] if red == 'mean' else o['loss'].sum()
        (dx,) = torch.autograd.grad(loss, logp, retain_graph=True)
        loss.backward()
        res[route] = (seq, o, dx, _grads(model))
    (sa, oa, da, ga), (sb, ob, db, gb) = res['fused'], res['generic']
    assert torch.equal(sa, sb)
    for k in ('loss', 'pg_loss', 'kl_loss', 'clipfrac'):
        assert torch.allclose(oa[k], ob[k], atol=1e-5, rtol=1e-4), (k, oa[k], ob[k])
    assert float((da - db).abs().max()) <= 1e-5 * float(db.abs().max()) + 1e-8
    assert float(oa['clipfrac']) > 0, (oa['kl_loss'], oa['clipfrac'])
    floor = 1e-6 * max(float(v.abs().max()) for v in gb.values())
    assert set(ga) == set(gb)
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 2e-4 * float(gb[k].abs().max()) + floor, k


@pytest.mark.parametrize('fam', ('updown', 'transformer'))
def test_identity_old_model_gives_new_self_critical(fam, tmp_path, monkeypatch):
    """old model == live model (dropout 0): r == 1, kl == 0, clipfrac == 0, and the parameter gradients of the PPO step equal those of
    structure_loss_type new_self_critical without PPO on the same samples"""
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    model = family_model(fam, perturb=0.1, seed=4).train()
    path = str(tmp_path / 'same.pth')
    torch.save(model.state_dict(), path)
    scores = torch.tensor([0.1, 0.9, 0.4, 0.5, 0.5, 0.5, 1.3, 0.2, 0.0], device=DEV)
    monkeypatch.setattr(losses, 'get_scores', lambda gts, s, opt, as_tensor=False: scores)
    fc, att, am = _feats()
    res = {}
    for use_ppo in (1, 0):
        opt = tiny_opt(**KW[fam], use_ppo=use_ppo, ppo_old_model_path=path, train_sample_n=3,
                       structure_loss_type='new_self_critical', structure_loss_weight=1.0)
        lw = LossWrapper(model, opt)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(21)
        model._rng_calls = 0
        out = lw(fc, att, None, None, am, [None] * 3, torch.arange(3), False, True, False)
        out['loss'].backward()
        res[use_ppo] = (out, _grads(model))
        if use_ppo:                  # the per-token ratio and KL of the same samples
            from imagecaptioning.pytorch_amd import ops
            seq, logp = _rollout(model, fc, att, am, seed=21)
            lo = lw.ppo_crit.old_logprobs(fc, att, seq, am)
            _, _, rs, _ = ops.ppo_loss_fwd(logp.detach().contiguous(), lo.contiguous(), seq, scores, 3)
            m = ref_mask(seq)
            assert float((rs[1][m] - 1).abs().max()) < 2e-5
            assert float(rs[0][m].abs().max()) < 1e-5
    (oa, ga), (ob, gb) = res[1], res[0]
    assert float(oa['clipfrac']) == 0.0 and abs(float(oa['kl_loss'])) < 1e-6
    # (the losses differ -- mean(-A r) against mean(-A log p) -- but at r == 1 their gradients are the same)
    floor = 1e-6 * max(float(v.abs().max()) for v in gb.values())
    for k in gb:
        assert float((ga[k] - gb[k]).abs().max()) <= 1e-3 * float(gb[k].abs().max()) + floor, k


def test_train_step_runs_ppo_launch_by_launch(tmp_path):
    """TrainStep with use_ppo: no capture (the old model's forward sizes itself on the host), the same numbers as a direct
    LossWrapper call under the same step record"""
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd.graph_step import TrainStep
    from test_graph_step_gpu import _setup, _batches
    _, model0, _, _, _ = _setup('aoa')
    path = str(tmp_path / 'old.pth')
    torch.save(model0.state_dict(), path)
    runs = []
    for direct in (False, True):
        opt, model, flat, lw, dims = _setup('aoa')
        opt.use_ppo, opt.ppo_old_model_path = 1, path
        from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
        lw = LossWrapper(model, opt)
        batch = _batches('aoa', dims, nb=1)[0]
        if not direct:
            ts = TrainStep(lw, flat, opt, DEV, graph=True)
            for _ in range(2):
                loss, out = ts(batch, False, True, lr=0.0)
            assert ts.captures == 0 and ts.replays == 0 and ts.stepped == 2 and ts.failed is None
            runs.append((float(loss), {k: float(out[k]) for k in ('pg_loss', 'kl_loss', 'clipfrac')}))
        else:
            st = ops.StepState(torch.device(DEV))
            for _ in range(2):
                st.advance(opt.optim_alpha, opt.optim_beta)
                model._rng_calls = 0
                with st.bound():
                    out = lw(batch['fc_feats'], batch['att_feats'], None, None, None, batch['gts'], torch.arange(3), False, True, False)
            runs.append((float(out['loss'].detach()), {k: float(out[k]) for k in ('pg_loss', 'kl_loss', 'clipfrac')}))
    assert all(np.isfinite(v) for v in [runs[0][0]] + list(runs[0][1].values()))
    assert runs[0][0] == pytest.approx(runs[1][0], rel=1e-5, abs=1e-6), runs
    for k in runs[0][1]:
        assert runs[0][1][k] == pytest.approx(runs[1][1][k], rel=1e-5, abs=1e-6), (k, runs)


@pytest.mark.parametrize('fam', ('updown', 'transformer'))
def test_train_py_xe_then_ppo(fam, tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd'))
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import opts, rewards
    small = ['--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--fc_feat_size', '24', '--att_feat_size', '24',
             '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6', '--max_length', '6', '--batch_size', '4',
             '--seq_per_img', '2', '--synthetic_images', '8', '--losses_log_every', '1']
    if fam == 'transformer':
        small += ['--caption_model', 'transformer', '--d_model', '32', '--d_ff', '64', '--N_enc', '1', '--N_dec', '1',
                  '--num_att_heads', '4']
    a, b = tmp_path / 'xe', tmp_path / 'ppo'
    T.train(opts.parse_opt(small + ['--max_iters', '3', '--save_checkpoint_every', '3', '--checkpoint_path', str(a)]))
    old = torch.load(a / 'model.pth')
    rewards.reset_scorer()
    capsys.readouterr()
    loss = T.train(opts.parse_opt(small + ['--max_iters', '3', '--structure_after', '0', '--use_ppo', '1', '--ppo_old_model_path',
                                           str(a / 'model.pth'), '--structure_loss_type', 'new_self_critical', '--train_sample_n', '3',
                                           '--save_checkpoint_every', '3', '--checkpoint_path', str(b)]))
    rewards.reset_scorer()
    text = capsys.readouterr().out
    assert np.isfinite(loss)
    lines = [ln for ln in text.splitlines() if 'pg_loss =' in ln]
    assert len(lines) == 3, text
    for ln in lines:
        vals = [float(x.split('=')[1]) for x in ln.split(', ')[1:]]
        assert len(vals) == 3 and all(np.isfinite(vals)), ln
    after = torch.load(a / 'model.pth')
    assert set(after) == set(old) and all(torch.equal(after[k], old[k]) for k in old)
    trained = torch.load(b / 'model.pth')
    assert set(trained) == set(old)                                      # no old-model weights in the checkpoint
    assert any(not torch.equal(trained[k], old[k]) for k in old)
