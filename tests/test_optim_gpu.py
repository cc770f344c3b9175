"""The fused flat-buffer optimizer rules other than Adam (capmi_optim_step / capmi_optim_step_dyn: rmsprop, adagrad, sgdm, sgdmom,
adamw) on a real MI355X: kernel against the float64 replay (tests/optim_ref64.py), captured form against stepped form,
flat.FlatParams, graph_step.TrainStep and tools/train.py end to end.

Tolerance of the kernel tests: the one test_kernels_gpu.test_adam_matches_torch holds capmi_adam_step to, max |a - b| / max |b|
< 1e-6."""
import os
import sys

import pytest
import torch

import optim_ref64 as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
TOL = 1e-6
# (alpha, beta, eps) as misc.build_optimizer hands them to each rule at the command line's defaults
HP = {'rmsprop': (0.9, 0.999, 1e-8), 'adagrad': (0.9, 0.999, 1e-10), 'sgdm': (0.9, 0.999, 1e-8), 'sgdmom': (0.9, 0.999, 1e-8),
      'adamw': (0.9, 0.999, 1e-8)}
# (n, element offset of the range inside its allocation): offset 1 = 4 bytes off a 16-byte boundary, the start of a shard or bucket
# of the flat buffer -- scalar head and tail around the quads
SIZES = [(1, 0), (3, 0), (4, 0), (5, 0), (1023, 0), (4096 + 7, 0), (1023, 1), (4096 + 7, 1), (6, 1)]
SETTINGS = [(clip, scale, wd) for clip in (0.0, 0.1) for scale in (1.0, 0.2) for wd in (0.0, 0.01)]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _buffers(n, off, k):
    """k zero fp32 ranges of n elements that start `off` elements into their own 16-byte aligned allocation"""
    return [torch.zeros(n + off, device=DEV)[off:] for _ in range(k)]


@pytest.mark.parametrize('rule', R.RULES)
def test_kernel_matches_the_float64_replay(rule):
    """4 consecutive steps (the first-step momentum rule and the state carry both show) at every size, alignment and setting, the rate
    moving between the steps.  Gradients ~ N(0, 0.3^2): with clip 0.1 some but not all of them are clipped at either scale."""
    from imagecaptioning.pytorch_amd import ops
    alpha, beta, eps = HP[rule]
    keys = R.STATE_KEYS[rule]
    worst = 0.0
    for n, off in SIZES:
        for clip, scale, wd in SETTINGS:
            g = torch.Generator().manual_seed(1000 * n + off)
            p0 = torch.randn(n, generator=g)
            grads = [torch.randn(n, generator=g) * 0.3 for _ in range(4)]
            if clip > 0 and n > 100:
                hit = (grads[0] * scale).abs() > clip
                assert 0 < int(hit.sum()) < n
            bufs = _buffers(n, off, 2 + len(keys))
            p, gd, state = bufs[0], bufs[1], bufs[2:]
            assert p.data_ptr() % 16 == 4 * off
            p.copy_(p0)
            p64, st64 = p0.double(), R.new_state(rule, p0)
            for t in range(1, 5):
                lr = 1e-2 / t
                gd.copy_(grads[t - 1])
                ops.optim_step(rule, p, gd, state[0], state[1] if len(state) > 1 else None, lr, alpha, beta, eps, wd, clip, scale, t)
                R.step(rule, p64, grads[t - 1], st64, R.f32(lr), t, alpha=R.f32(alpha), beta=R.f32(beta), eps=R.f32(eps),
                       weight_decay=R.f32(wd), clip=R.f32(clip), grad_scale=R.f32(scale))
            assert torch.equal(gd.cpu(), grads[3])                       # the gradient is read, never written
            errs = [rel_err(p, p64)] + [rel_err(s, st64[k]) for s, k in zip(state, keys)]
            worst = max(worst, *errs)
            assert max(errs) < TOL, (rule, n, off, clip, scale, wd, errs)
    print('%s: worst relative error against the float64 replay %.3g' % (rule, worst))


@pytest.mark.parametrize('rule', R.RULES)
def test_range_neighbours_are_not_touched(rule):
    """a range inside a larger buffer, starting off a 16-byte boundary: the elements in front of and behind it keep their values in
    every buffer (the scalar head and tail end where the range ends)"""
    from imagecaptioning.pytorch_amd import ops
    alpha, beta, eps = HP[rule]
    k = 2 + len(R.STATE_KEYS[rule])
    for lo, n in ((1, 1023), (3, 9), (2, 2), (5, 4096 + 7)):
        g = torch.Generator(device=DEV).manual_seed(lo)
        whole = [torch.randn(lo + n + 6, device=DEV, generator=g).abs() for _ in range(k)]
        before = [w.clone() for w in whole]
        r = [w[lo:lo + n] for w in whole]
        ops.optim_step(rule, r[0], r[1], r[2], r[3] if k > 3 else None, 1e-2, alpha, beta, eps, 0.01, 0.1, 1.0, 2)
        for w, b in zip(whole, before):
            assert torch.equal(w[:lo], b[:lo]) and torch.equal(w[lo + n:], b[lo + n:])
        assert not torch.equal(whole[0][lo:lo + n], before[0][lo:lo + n])
        assert torch.equal(whole[1], before[1])


@pytest.mark.parametrize('rule', R.RULES)
def test_dyn_form_is_the_stepped_form_bit_for_bit(rule):
    """capmi_optim_step_dyn with the rate written by capmi_step_set_lr and the step number (and AdamW's bias corrections) by
    capmi_step_advance == capmi_optim_step with the same values, to the bit -- aligned and as a shard"""
    from imagecaptioning.pytorch_amd import ops
    alpha, beta, eps = HP[rule]
    nk = len(R.STATE_KEYS[rule])
    for n, off in ((64 * 100, 0), (4096 + 7, 1)):
        g = torch.Generator().manual_seed(3 + off)
        p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.3
        a, b = _buffers(n, off, 2 + nk), _buffers(n, off, 2 + nk)
        for bufs in (a, b):
            bufs[0].copy_(p0)
            bufs[1].copy_(gr)
        st = ops.StepState(torch.device(DEV), lr=0.0)
        for step in range(1, 5):
            lr = 1e-3 / step
            ops.optim_step(rule, a[0], a[1], a[2], a[3] if nk > 1 else None, lr, alpha, beta, eps, 0.01, 0.1, 0.5, step)
            st.set_lr(lr)
            st.advance(alpha, beta)
            ops.optim_step_dyn(rule, b[0], b[1], b[2], b[3] if nk > 1 else None, st, alpha, beta, eps, 0.01, 0.1, 0.5)
        assert st.read().adam_step == 4
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert not torch.equal(a[0].cpu(), p0)


# ---------------------------------------------------------------------------------------------- FlatParams
def _tiny_updown(rule, seed=5):
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    V1 = 41
    opt = synthetic.updown_opt(vocab_size=V1 - 1, input_encoding_size=24, rnn_size=24, att_hid_size=12, fc_feat_size=20, att_feat_size=20,
                               seq_length=6, max_length=6, vocab={str(i): 'w%d' % i for i in range(1, V1)}, optim=rule)
    torch.manual_seed(seed)
    model = models.setup(opt).to(DEV)
    return opt, model, model.flatten_parameters_(rule)


@pytest.fixture(scope='module')
def one_rank_group(tmp_path_factory):
    """finish_overlap_and_step waits for the collectives of its buckets: a one-rank gloo group serves them in this process"""
    import torch.distributed as dist
    store = tmp_path_factory.mktemp('pg') / 'store'
    dist.init_process_group('gloo', init_method='file://%s' % store, rank=0, world_size=1)
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize('rule', R.RULES)
def test_flat_params_steps_by_bucket_and_round_trips_its_state(rule, one_rank_group):
    """3 steps through finish_overlap_and_step (two announced buckets + the leftovers: the update runs range by range, some ranges
    starting off the buffer's front) on a tiny UpDown's parameters against the float64 replay on the same gradients; state_dict ->
    load_state_dict is bit-equal; a state saved under another rule is refused by a message naming both."""
    from imagecaptioning.pytorch_amd.captioning.utils import misc
    opt, model, flat = _tiny_updown(rule)
    hp = misc.build_optimizer(opt)
    keys = R.STATE_KEYS[rule]
    assert flat.rule == rule and flat.state_keys == keys
    if len(keys) == 1:
        assert not hasattr(flat, 'exp_avg') and not hasattr(flat, 'exp_avg_sq')      # Adam's second buffer is never allocated
    flat.begin_overlap()
    p64, st64 = flat.flat.double().cpu(), R.new_state(rule, flat.flat.cpu())
    g = torch.Generator().manual_seed(9)
    for t in range(1, 4):
        lr = 5e-3 / t
        flat.zero_grad()
        for n, p in zip(flat.names, flat.params):
            flat.grad_views[n].copy_(torch.randn(p.shape, generator=g) * 0.3)
        flat.end_backward()
        flat._bucket_ready(flat.names[-2:])                                 # two buckets a native backward would announce; the rest are leftovers
        flat._bucket_ready(flat.names[2:4])
        grad = flat.grad.clone().cpu()
        flat.finish_overlap_and_step(lr, hp['betas'], hp['eps'], 0.01, clip_value=0.1)
        assert flat.last_collectives >= 3 and flat.step_count == t
        R.step(rule, p64, grad, st64, R.f32(lr), t, alpha=R.f32(hp['betas'][0]), beta=R.f32(hp['betas'][1]), eps=R.f32(hp['eps']),
               weight_decay=R.f32(0.01), clip=R.f32(0.1), grad_scale=1.0)
    used = flat.used                                                        # (the padding behind `used` carries no gradient)
    assert rel_err(flat.flat[:used], p64[:used]) < TOL
    for k in keys:
        assert rel_err(getattr(flat, k)[:used], st64[k][:used]) < TOL, k
    for p, o in zip(flat.params, flat.offsets):                             # the parameters still ARE the flat buffer
        assert p.data_ptr() == flat.flat.data_ptr() + 4 * o
    sd = flat.state_dict()
    assert sd['rule'] == rule and sd['step_count'] == 3 and set(keys) <= set(sd)
    _, _, back = _tiny_updown(rule)
    back.load_state_dict(sd)
    assert back.step_count == 3
    for k in keys:
        assert torch.equal(getattr(back, k), getattr(flat, k))
    other = 'sgdmom' if rule != 'sgdmom' else 'rmsprop'
    _, _, wrong = _tiny_updown(other)
    with pytest.raises(ValueError, match='%r.*%r' % (rule, other)):
        wrong.load_state_dict(sd)


# ---------------------------------------------------------------------------------------------- captured step
@pytest.mark.parametrize('rule', ['rmsprop', 'sgdmom'])
def test_captured_step_is_the_stepped_step_bit_for_bit(rule):
    """graph_step.TrainStep with graph=True against stepped, 3 iterations of a tiny XE step: the captured graph ends in
    capmi_optim_step_dyn and replays with the rate moving underneath it.  Model, batches and loop are those of
    test_graph_step_gpu.test_captured_training_step_is_the_stepped_step_bit_for_bit -- its Transformer: an UpDown XE step cannot be
    captured into a hipGraph under any optimizer (its forward makes a call the capturing stream refuses,
    hipErrorStreamCaptureUnsupported; the trainer steps that family launch by launch, graph_step.py), so there is no captured
    UpDown step to compare.  The parameters move into a flat buffer of the rule under test before the first step."""
    from test_graph_step_gpu import _batches, _setup
    from imagecaptioning.pytorch_amd.graph_step import TrainStep
    runs = {}
    for mode in ('stepped', 'graph'):
        opt, model, _, lw, dims = _setup('transformer')
        opt.optim, opt.weight_decay = rule, 0.01
        flat = model.flatten_parameters_(rule)
        batches = _batches('transformer', dims)
        ts = TrainStep(lw, flat, opt, DEV, graph=(mode == 'graph'))
        losses = []
        for it in range(3):
            lr = 1e-2 if it < 2 else 5e-3                                  # the schedule moves the rate under the replayed graph
            loss, _ = ts(batches[0], False, False, lr=lr)
            losses.append(loss.clone())
        torch.cuda.synchronize()
        st = ts.state.read()
        assert st.adam_step == 3 and flat.step_count == 3
        if mode == 'graph':
            assert ts.failed is None, ts.failed
            assert ts.captures == 1 and ts.replays == 2 and ts.stepped == 1, (ts.captures, ts.replays, ts.stepped)
        else:
            assert ts.captures == 0 and ts.stepped == 3
        assert all(p.data_ptr() == flat.flat.data_ptr() + 4 * o for p, o in zip(flat.params, flat.offsets))
        runs[mode] = (torch.stack(losses).cpu(), flat.flat.clone().cpu(), getattr(flat, flat.state_keys[0]).clone().cpu())
    a, b = runs['stepped'], runs['graph']
    assert torch.isfinite(a[0]).all() and len(set(a[0].tolist())) == 3
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert float(a[2].abs().max()) > 0


# ---------------------------------------------------------------------------------------------- tools/train.py
def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


@pytest.mark.parametrize('rule', R.RULES)
def test_trainer_runs_checkpoints_and_resumes_under_every_rule(tmp_path, rule):
    """tools/train.py --optim <rule> at test_entrypoints_gpu's small sizes: 2 iterations, checkpoint, resume, 1 more == 3 iterations
    straight, parameters and optimizer state to the bit (warm-up on: the rate differs at every iteration).  Resuming the checkpoint
    under another --optim fails with a message that names both."""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    small = ['--caption_model', 'updown', '--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--fc_feat_size', '24',
             '--att_feat_size', '24', '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6', '--max_length', '6',
             '--batch_size', '4', '--seq_per_img', '2', '--synthetic_images', '12', '--use_warmup', '1', '--noamopt_warmup', '6',
             '--learning_rate', '0.01', '--drop_prob_lm', '0.5', '--weight_decay', '0.01', '--optim', rule]
    a, b = tmp_path / 'a', tmp_path / 'b'
    T.train(_opts(small + ['--max_iters', '3', '--save_checkpoint_every', '3', '--checkpoint_path', str(a)]))
    T.train(_opts(small + ['--max_iters', '2', '--save_checkpoint_every', '2', '--checkpoint_path', str(b)]))
    osd = torch.load(b / 'optimizer.pth', weights_only=False)['flat']
    keys = R.STATE_KEYS[rule]
    assert osd['rule'] == rule and osd['step_count'] == 2 and all(float(osd[k].abs().max()) > 0 for k in keys)
    if len(keys) == 1:
        assert 'exp_avg' not in osd and 'exp_avg_sq' not in osd
    other = 'adam' if rule != 'adamw' else 'rmsprop'
    with pytest.raises(ValueError, match='%r.*%r' % (rule, other)):
        T.train(_opts(small[:-1] + [other, '--max_iters', '3', '--checkpoint_path', str(tmp_path / 'c'), '--start_from', str(b)]))
    T.train(_opts(small + ['--max_iters', '3', '--save_checkpoint_every', '3', '--checkpoint_path', str(b), '--start_from', str(b)]))
    pa, pb = torch.load(a / 'model.pth'), torch.load(b / 'model.pth')
    p0 = torch.load(tmp_path / 'c' / 'model.pth') if (tmp_path / 'c' / 'model.pth').exists() else None
    assert p0 is None                                                      # the refused resume wrote nothing
    assert set(pa) == set(pb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), (k, float((pa[k] - pb[k]).abs().max()))
    sa, sb = (torch.load(d / 'optimizer.pth', weights_only=False)['flat'] for d in (a, b))
    assert sa['step_count'] == sb['step_count'] == 3
    for k in keys:
        assert torch.equal(sa[k], sb[k]), k
