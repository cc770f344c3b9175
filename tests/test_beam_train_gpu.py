"""Beam search as a training rollout on a real MI355X (train_sample_method greedy, train_beam_size > 1; reference
ADVANCED.md "SCST in Topdown Bottomup paper"): search with training numerics, capmi_beam_finalize, forced replay with gradient.

Golden parity is against the REAL reference's train-mode beam search (tests/golden/beam_train_tiny.npz, masks injected through
opt['_beam_masks']); the gradient tolerance is the one tests/test_updown_gpu.py already uses for RewardCriterion gradients of
these kernels (rtol 5e-4, atol 1e-6 + 2e-5 * max|ref|), the log-prob tolerance the one it uses for rollout log-probs.
"""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import beam_train_ref64 as ref
from test_beam_train_host import load, inputs, random_tables, RUNS, BEAM, L, FAMILIES, _tiny_model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
LOGP_TOL = dict(rtol=2e-5, atol=5e-6)


def tiny_opt(family, drop):
    """tests/golden/make_golden.tiny_opt: the sizes of the fixture"""
    V = 30
    return argparse.Namespace(caption_model=family, vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1, drop_prob_lm=drop,
                              seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=12, use_bn=0, logit_layers=1,
                              vocab={str(i): 'w%d' % i for i in range(1, V + 1)}, rnn_type='lstm')


def golden_model(family, drop=0.0):
    from imagecaptioning.pytorch_amd.captioning import models
    zz, P = load(family)
    model = models.setup(tiny_opt(family, drop))
    model.load_state_dict(P)
    return zz, P, model.to(DEV)


def d(x):
    return None if x is None else x.to(DEV)


def masks_to_dev(masks):
    return None if masks is None else {k: v.to(DEV).contiguous() for k, v in masks.items()}


# ------------------------------------------------------------------------------------------------------------ finalize
def _check_finalize(parent, token, score, ended, pen, sample_n):
    """capmi_beam_finalize against assemble_done_beams on the same device tables."""
    from imagecaptioning.pytorch_amd import beam

    class M:
        pass
    Lx, B, bd = parent.shape
    V1 = 5
    logp_rows = torch.zeros(Lx, B * bd, V1, device=DEV)
    logp_rows[:, :, 0] = torch.arange(Lx * B * bd, device=DEV, dtype=torch.float32).view(Lx, B * bd)     # row id in column 0
    m = M()
    seq_h, slp_h = beam.assemble_done_beams(m, parent, token, score, ended, logp_rows, B, bd, Lx, V1, sample_n, bd, {'length_penalty': pen})
    seq, lineage, length, p = beam.finalize(parent, token, score, ended, sample_n, pen)
    torch.cuda.synchronize()
    assert seq.dtype == torch.long and torch.equal(seq, seq_h)
    len_h = torch.tensor([m.done_beams[b][i]['seq'].shape[0] for b in range(B) for i in range(sample_n)], dtype=torch.int32)
    p_h = torch.tensor([m.done_beams[b][i]['p'] for b in range(B) for i in range(sample_n)], dtype=torch.float64).float()
    assert torch.equal(length.cpu(), len_h)
    assert torch.equal(p.cpu(), p_h), (p.cpu() - p_h).abs().max()
    lin = lineage.cpu().long()
    for row in range(B * sample_n):
        n = int(len_h[row])
        want = slp_h[row, :n, 0].cpu().long()                     # flat row ids t * N + search row, as the host gathered them
        got = torch.arange(n) * (B * bd) + lin[:n, row]
        assert torch.equal(got, want), (row, got, want)
        assert bool((lin[n:, row] == -1).all())


@pytest.mark.parametrize('pen', ['', 'wu_0.7', 'avg_0'])
@pytest.mark.parametrize('repeats', [False, True])
def test_finalize_kernel_equals_the_host_assembly_on_random_tables(pen, repeats):
    rng = np.random.RandomState(5 + repeats)
    for B, bd, Lx in ((4, 3, 6), (2, 5, 9), (3, 1, 4), (10, 5, 20), (1, 16, 64)):
        tabs = [torch.from_numpy(a).to(DEV) for a in random_tables(rng, B, bd, Lx, repeats)]
        for sample_n in sorted({1, bd}):
            _check_finalize(*tabs, pen, sample_n)


def _config_model(family='updown', drop=0.0, seed=3):
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    torch.manual_seed(seed)
    model = models.setup(synthetic.updown_opt(caption_model=family, drop_prob_lm=drop)).to(DEV)
    with torch.no_grad():
        model.logit.bias[0] += 1.5           # beams of several lengths
    return model


def test_finalize_kernel_on_the_tables_of_a_real_search_at_config_size():
    from imagecaptioning.pytorch_amd import synthetic
    model = _config_model()
    fc, att = synthetic.batch(10, device=DEV)
    model.train()
    seq, slp = model(fc, att, None, opt=dict(sample_method='greedy', beam_size=5, sample_n=5), mode='sample')
    t = model._last_beam
    for pen in ('', 'wu_0.5'):
        for sample_n in (1, 5):
            _check_finalize(t['parent'], t['token'], t['score'], t['ended'], pen, sample_n)
    assert len(set(t['length'].cpu().tolist())) > 1


# ------------------------------------------------------------------------------------------------------- golden parity
@pytest.mark.parametrize('tag', RUNS)
@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_golden_parity_with_the_reference_train_mode_beam_search(family, tag):
    """seq exact; seqLogprobs and every parameter gradient of the RewardCriterion loss.  Fails without the feature: the log-probs of
    a beam search come back without a graph."""
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    zz, _ = load(family)
    drop, sample_n = float(zz[tag + '.opt'][0]), int(zz[tag + '.opt'][1])
    pen = str(zz[tag + '.length_penalty'])
    zz, P, model = golden_model(family, drop)
    fc, att, am = inputs(zz)
    masks = ref.recorded_masks(zz, tag, family, fc.shape[0], BEAM, L, am) if drop > 0 else None
    model.train()
    model.zero_grad(set_to_none=True)
    o = dict(sample_method='greedy', beam_size=BEAM, sample_n=sample_n, length_penalty=pen)
    if masks is not None:
        o['_beam_masks'] = masks_to_dev(masks)
    seq, slp = model(d(fc), d(att), d(am), opt=o, mode='sample')
    assert slp.requires_grad
    assert model.done_beams is None
    assert np.array_equal(seq.cpu().numpy(), zz[tag + '.seq'])
    np.testing.assert_allclose(slp.detach().cpu().numpy(), zz[tag + '.logp'], **LOGP_TOL)
    loss = losses.RewardCriterion()(slp, seq.data, torch.from_numpy(zz[tag + '.reward']).to(DEV))
    np.testing.assert_allclose(loss.item(), zz[tag + '.loss'], rtol=1e-5)
    loss.backward()
    for k, p in model.named_parameters():
        g = zz['%s.grad.%s' % (tag, k)]
        assert p.grad is not None, k
        print('%s %s %-32s max|ref| %.3e  max err %.3e' % (family, tag, k, np.abs(g).max(), np.abs(p.grad.cpu().numpy() - g).max()))
        np.testing.assert_allclose(p.grad.cpu().numpy(), g, rtol=5e-4, atol=1e-6 + 2e-5 * np.abs(g).max(), err_msg=k)


# ------------------------------------------------------------------------------- consistency with the eval-mode search
def _train_vs_eval(model, fc, att, am, bd, sample_n):
    model.train()
    seq, slp = model(fc, att, am, opt=dict(sample_method='greedy', beam_size=bd, sample_n=sample_n), mode='sample')
    assert slp.requires_grad
    model.eval()
    with torch.no_grad():
        seq_e, slp_e = model(fc, att, am, opt=dict(sample_method='greedy', beam_size=bd, sample_n=sample_n), mode='sample')
    assert torch.equal(seq, seq_e)
    np.testing.assert_allclose(slp.detach().cpu().numpy(), slp_e.cpu().numpy(), **LOGP_TOL)
    return seq


@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_without_dropout_the_new_path_equals_the_eval_mode_beam_search_tiny(family):
    zz, P, model = golden_model(family, 0.0)
    fc, att, am = inputs(zz)
    for sample_n in (1, BEAM):
        _train_vs_eval(model, d(fc), d(att), d(am), BEAM, sample_n)
        _train_vs_eval(model, d(fc), d(att), None, BEAM, sample_n)


@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_without_dropout_the_new_path_equals_the_eval_mode_beam_search_config_size(family):
    from imagecaptioning.pytorch_amd import synthetic
    model = _config_model(family)
    fc, att = synthetic.batch(10, device=DEV)
    am = torch.ones(10, 36, device=DEV)
    for b in range(10):
        am[b, 36 - 2 * b:] = 0
    seq = _train_vs_eval(model, fc, att, None, 5, 5)
    assert len(set((seq > 0).sum(1).tolist())) > 1
    _train_vs_eval(model, fc, att, am, 5, 1)


# ------------------------------------------------------------------------------------------------------- Philox masks
def philox_search_and_replay_agree(model, fc, att, am, bd, tol):
    """Two calls at the same _rng_calls position agree bit for bit, and the replayed log-prob of every beam token equals the
    search's own score difference along the beam's lineage (within `tol`): search and replay saw the same masks.  Inputs on the
    device; shared with the config-size test (tests/test_beam_train_full_gpu.py)."""
    model.train()
    outs = []
    for _ in range(2):
        torch.manual_seed(9)
        model._rng_calls = 0
        seq, slp = model(fc, att, am, opt=dict(sample_method='greedy', beam_size=bd, sample_n=bd), mode='sample')
        outs.append((seq.clone(), slp.detach().clone(), {k: v.clone() for k, v in model._last_beam.items()}))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    seq, slp, t = outs[0]
    sel = slp.gather(2, seq.unsqueeze(2)).squeeze(2).cpu().double()                 # [rows, L]
    seq = seq.cpu()
    score, lineage, length = t['score'].cpu().double(), t['lineage'].cpu().long(), t['length'].cpu()
    B = fc.shape[0]
    checked = 0
    # the beam's own slot after the selection of step t: the row its successor came from (lineage[t + 1] - b * bd); the last
    # step's slot is found by the token / parent match below
    parent, token = t['parent'].cpu(), t['token'].cpu()
    for row in range(B * bd):
        b, n = row // bd, int(length[row])
        prev = 0.0
        for s in range(n):
            if s + 1 < n:
                slot = int(lineage[s + 1, row]) - b * bd
            else:
                src = 0 if s == 0 else int(lineage[s, row]) - b * bd
                cand = [j for j in range(bd) if int(token[s, b, j]) == int(seq[row, s]) and int(parent[s, b, j]) == src]
                assert len(cand) == 1
                slot = cand[0]
            sc = float(score[s, b, slot])
            np.testing.assert_allclose(float(sel[row, s]), sc - prev, **tol)
            prev = sc
            checked += 1
    assert checked > B * bd
    # a different stream position gives different masks
    seq2, slp2 = model(fc, att, am, opt=dict(sample_method='greedy', beam_size=bd, sample_n=bd), mode='sample')
    assert not torch.equal(slp2.detach(), slp)


@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_philox_masks_are_shared_by_search_and_replay(family):
    """Two calls at the same _rng_calls position agree bit for bit, and the replayed log-prob of every beam token equals the
    search's own score difference along the beam's lineage: search and replay saw the same masks."""
    zz, P, model = golden_model(family, 0.5)
    fc, att, am = inputs(zz)
    philox_search_and_replay_agree(model, d(fc), d(att), d(am), BEAM, dict(rtol=2e-5, atol=2e-5))


# ------------------------------------------------------------------------------------------------- LossWrapper / train
def _refs(rng, V1, Lx, n=5):
    rows = np.zeros((n, Lx), dtype=np.uint32)
    for r in range(n):
        ln = int(rng.integers(2, Lx + 1))
        rows[r, :ln] = rng.integers(1, min(V1, 12), ln)
    return rows


@pytest.mark.parametrize('family', ['updown', 'newfc'])
@pytest.mark.parametrize('branch', ['sc', 'struc'])
def test_loss_wrapper_end_to_end(family, branch):
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    from imagecaptioning.pytorch_amd.captioning.utils import rewards
    V1, Lx, F, B, K = 61, 6, 40, 3, 5
    kw = dict(caption_model=family, seq_length=Lx, max_length=Lx, vocab_size=V1 - 1, fc_feat_size=F, att_feat_size=F,
              vocab={str(i): 'w%d' % i for i in range(1, V1)}, input_encoding_size=32, rnn_size=32, att_hid_size=16, drop_prob_lm=0.5,
              train_sample_method='greedy', train_beam_size=5, train_sample_n=5)
    if branch == 'struc':
        kw.update(structure_loss_type='new_self_critical', structure_loss_weight=1.0)
    opt = synthetic.updown_opt(**kw)
    torch.manual_seed(2)
    model = models.setup(opt).to(DEV)
    lw = LossWrapper(model, opt)
    rewards.reset_scorer()
    rng = np.random.default_rng(3)
    df, ref_len = synthetic.document_frequency([_refs(rng, V1, Lx) for _ in range(50)])
    rewards.init_scorer((df, ref_len), device=torch.device(DEV))
    g = torch.Generator().manual_seed(5)
    fc = torch.randn(B, F, generator=g).clamp_min(0).to(DEV)
    att = torch.randn(B, K, F, generator=g).clamp_min(0).to(DEV)
    gts = rewards.pack_gts([_refs(rng, V1, Lx) for _ in range(B)])
    model.train()
    out = lw(fc, att, None, None, None, gts, torch.arange(B), branch == 'sc', branch == 'struc', False)
    assert torch.isfinite(out['loss']) and 'reward' in out
    out['loss'].backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert sum(float(p.grad.abs().sum()) for p in model.parameters()) > 0
    rewards.reset_scorer()


@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_tools_train_runs_a_beam_search_scst(family, tmp_path):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    from captioning.utils import opts, rewards
    small = ['--caption_model', family, '--rnn_size', '64', '--input_encoding_size', '64', '--att_hid_size', '32', '--fc_feat_size', '48',
             '--att_feat_size', '48', '--vocab_size', '60', '--synthetic_regions', '7', '--seq_length', '8', '--max_length', '8',
             '--batch_size', '4', '--seq_per_img', '3', '--synthetic_images', '16', '--losses_log_every', '2', '--checkpoint_path', str(tmp_path),
             '--train_sample_method', 'greedy', '--train_beam_size', '5', '--train_sample_n', '5']
    rewards.reset_scorer()
    l0 = T.train(opts.parse_opt(small + ['--max_iters', '4', '--self_critical_after', '0', '--save_checkpoint_every', '4']))
    assert np.isfinite(l0)
    first = {k: v.clone() for k, v in torch.load(os.path.join(str(tmp_path), 'model.pth'), map_location='cpu').items()}
    rewards.reset_scorer()
    l1 = T.train(opts.parse_opt(small + ['--max_iters', '8', '--structure_after', '0', '--structure_loss_type', 'new_self_critical',
                                         '--save_checkpoint_every', '8', '--start_from', str(tmp_path)]))
    assert np.isfinite(l1)
    second = torch.load(os.path.join(str(tmp_path), 'model.pth'), map_location='cpu')
    assert any(not torch.equal(first[k], second[k]) for k in first)
    rewards.reset_scorer()


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('family,extra', FAMILIES)
def test_other_families_refuse_on_device_tensors(family, extra):
    model = _tiny_model(family, extra).to(DEV)
    model.train()
    fc, att = torch.zeros(2, 12, device=DEV), torch.zeros(2, 3, 12, device=DEV)
    with pytest.raises(NotImplementedError, match='train_beam_size'):
        model(fc, att, None, opt=dict(beam_size=2, sample_n=2), mode='sample')
    model.eval()
    with torch.no_grad():                                           # their eval-mode search is untouched
        seq, _ = model(fc, att, None, opt=dict(beam_size=2, sample_n=2), mode='sample')
    assert seq.shape == (4, 5)


@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_unsupported_options_are_named_on_device_tensors(family):
    model = _tiny_model(family, {}).to(DEV)
    model.train()
    fc, att = torch.zeros(2, 12, device=DEV), torch.zeros(2, 3, 12, device=DEV)
    for name, o in (('group_size', dict(group_size=2, beam_size=4)), ('decoding_constraint', dict(decoding_constraint=1)),
                    ('remove_bad_endings', dict(remove_bad_endings=1)), ('temperature', dict(temperature=0.5)),
                    ('output_logsoftmax', dict(output_logsoftmax=0)), ('use_ppo', dict(use_ppo=1))):
        with pytest.raises(NotImplementedError, match=name):
            model(fc, att, None, opt=dict(dict(beam_size=2, sample_n=2), **o), mode='sample')
    with torch.no_grad():                                           # no gradient wanted: the search that exists, host-assembled beams
        seq, slp = model(fc, att, None, opt=dict(beam_size=2, sample_n=2), mode='sample')
    assert not slp.requires_grad and model.done_beams is not None
