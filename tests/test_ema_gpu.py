"""The exponential moving average of the parameters (capmi_ema_step / capmi_ema_step_dyn, --ema_decay) on a real MI355X: the kernel
against the float64 replay (tests/ema_ref64.py), the record-reading form against the by-value form, the argument checks, and
tools/train.py end to end.

Tolerance (ema_ref64's docstring): two float32 roundings per step of values bounded by m = max(|ema|, |p|), so after S steps
|kernel - replay| <= 2 * S * 2^-24 * m, rtol 0, m taken from the inputs of each case."""
import os
import sys

import pytest
import torch

import ema_ref64 as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
STEPS = 20
WRAP = 2048 * 256 * 8 + 5            # one quad more than 2048 workgroups x 256 threads x 2 quads cover in one trip: the grid-stride loop wraps
COUNTS = [1, 3, 4, 5, 7, 8, 9, 1027, WRAP]
GUARD = 4                            # floats in front of (plus the offset) and behind every range: must keep their bits


def _bits(t):
    return t.view(torch.int32)


def _padded(n, off, fill):
    """a range of n floats that starts `off` floats off a 16-byte boundary, inside a guard-padded allocation filled with `fill`"""
    whole = torch.full((GUARD + 3 + n + GUARD,), fill, device=DEV)
    r = whole[GUARD + off:GUARD + off + n]
    assert r.data_ptr() % 16 == 4 * off
    return whole, r


# ---------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize('n', COUNTS)
def test_kernel_matches_the_float64_replay(n):
    """20 steps, p redrawn at every step, every start offset of ema and of p (head, tail and the differently-misaligned scalar route),
    warm-up off and on, decay 0 / 0.9 / 0.9999.  The replay of a (warm-up, decay) pair is computed once, in float64 on the device,
    and shared by the 16 offset pairs, which all see the same numbers."""
    from imagecaptioning.pytorch_amd import ops
    g = torch.Generator(device=DEV).manual_seed(n)
    ema0 = torch.randn(n, device=DEV, generator=g)
    ps = [torch.randn(n, device=DEV, generator=g) * (1.0 + 0.1 * t) for t in range(STEPS)]
    tol = R.atol(STEPS, ema0, *ps)
    worst = 0.0
    for warmup in (0, 1):
        for decay in (0.0, 0.9, 0.9999):
            ref = R.replay(ema0, ps, decay, warmup)
            for oe in range(4):
                for op in range(4):
                    we, e = _padded(n, oe, -7.0)
                    wp, p = _padded(n, op, 5.0)
                    e.copy_(ema0)
                    for t in range(STEPS):
                        p.copy_(ps[t])
                        ops.ema_step(e, p, decay, warmup, t + 1)
                    err = float((e.double() - ref).abs().max())
                    worst = max(worst, err)
                    assert err <= tol, (n, warmup, decay, oe, op, err, tol)
                    assert torch.equal(_bits(p), _bits(ps[-1]))                          # p is read, never written
                    for whole, off, fill in ((we, oe, -7.0), (wp, op, 5.0)):             # the guards keep their bits
                        front, back = whole[:GUARD + off], whole[GUARD + off + n:]
                        assert torch.equal(_bits(front), _bits(torch.full_like(front, fill))), (n, oe, op)
                        assert torch.equal(_bits(back), _bits(torch.full_like(back, fill))), (n, oe, op)
            if decay == 0.0 and not warmup:
                assert torch.equal(e, ps[-1])                                            # d = 0: the average IS the parameters
    print('n = %d: worst |kernel - float64 replay| %.3g, bound %.3g' % (n, worst, tol))


@pytest.mark.parametrize('n,oe,op', [(64 * 100, 0, 0), (4096 + 7, 1, 1), (1027, 2, 3)])
def test_dyn_form_is_the_by_value_form_bit_for_bit(n, oe, op):
    """capmi_ema_step_dyn with the step number written by capmi_step_advance == capmi_ema_step with the same number, to the bit, over
    steps 6..10 with decay 0.5 and warm-up on: (1 + step) / (10 + step) crosses 0.5 at step 8, so both sides of the fminf run."""
    from imagecaptioning.pytorch_amd import ops
    g = torch.Generator(device=DEV).manual_seed(17 + n)
    ema0 = torch.randn(n, device=DEV, generator=g)
    ps = [torch.randn(n, device=DEV, generator=g) for _ in range(5)]
    (_, a), (_, b), (_, c) = _padded(n, oe, 0.0), _padded(n, oe, 0.0), _padded(n, oe, 0.0)
    _, p = _padded(n, op, 0.0)
    for x in (a, b, c):
        x.copy_(ema0)
    st = ops.StepState(torch.device(DEV), adam_step=5)
    for i, step in enumerate(range(6, 11)):
        p.copy_(ps[i])
        ops.ema_step(a, p, 0.5, 1, step)
        st.advance(0.9, 0.999)
        ops.ema_step_dyn(b, p, st, 0.5, 1)
        ops.ema_step(c, p, 0.5, 0, step)
        assert torch.equal(_bits(a), _bits(b)), step
    assert st.read().adam_step == 10
    assert not torch.equal(a, c)                                                         # the warm-up side of the crossover was in effect
    ref = R.replay(ema0, ps, 0.5, 1, first_step=6)
    assert float((a.double() - ref).abs().max()) <= R.atol(5, ema0, *ps)


def test_invalid_arguments_are_einval_and_write_nothing():
    """every refusal of capmi.h, each before anything is launched: the sentinel buffers keep their bits"""
    from imagecaptioning.pytorch_amd import _lib, ops
    lib = _lib.lib
    ema = torch.full((16,), 3.25, device=DEV)
    p = torch.full((16,), -1.5, device=DEV)
    keep_e, keep_p = ema.clone(), p.clone()
    st = ops.StepState(torch.device(DEV), adam_step=3)
    keep_s = st.buf.clone()
    e, q, s = ema.data_ptr(), p.data_ptr(), st.buf.data_ptr()
    stream = _lib.stream_ptr()
    assert lib.capmi_ema_step(e, q, 16, 0.9, 1, 1, stream) == 0                          # the valid call these are variations of
    assert lib.capmi_ema_step_dyn(e, q, 16, s, 0.9, 1, stream) == 0
    torch.cuda.synchronize()
    assert not torch.equal(ema, keep_e)
    ema.copy_(keep_e)
    nan = float('nan')
    by_value = [(None, q, 16, 0.9, 1, 1), (e, None, 16, 0.9, 1, 1), (e, q, 0, 0.9, 1, 1), (e, q, -4, 0.9, 1, 1), (e, q, 16, 0.9, 1, 0),
                (e, q, 16, 0.9, 1, -3), (e, q, 16, -0.1, 1, 1), (e, q, 16, 1.0, 1, 1), (e, q, 16, 1.5, 1, 1), (e, q, 16, nan, 1, 1),
                (e + 2, q, 8, 0.9, 1, 1), (e, q + 2, 8, 0.9, 1, 1), (e, e, 16, 0.9, 1, 1)]
    for args in by_value:
        assert lib.capmi_ema_step(*args, stream) == _lib.EINVAL, args
    dyn = [(None, q, 16, s, 0.9, 1), (e, None, 16, s, 0.9, 1), (e, q, 16, None, 0.9, 1), (e, q, 0, s, 0.9, 1), (e, q, -4, s, 0.9, 1),
           (e, q, 16, s, -0.1, 1), (e, q, 16, s, 1.0, 1), (e, q, 16, s, 1.5, 1), (e, q, 16, s, nan, 1), (e + 2, q, 8, s, 0.9, 1),
           (e, q + 2, 8, s, 0.9, 1), (e, e, 16, s, 0.9, 1)]
    for args in dyn:
        assert lib.capmi_ema_step_dyn(*args, stream) == _lib.EINVAL, args
    with pytest.raises(_lib.CapmiError, match='capmi_ema_step failed: invalid argument'):
        ops.ema_step(ema, p, 1.0, 1, 1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ema), _bits(keep_e)) and torch.equal(_bits(p), _bits(keep_p)) and torch.equal(st.buf, keep_s)


# ---------------------------------------------------------------------------------------------- tools/train.py
# the tiny synthetic UpDown setting of test_entrypoints_gpu.test_resume_restores_optimizer_schedule_counters_and_loader
SMALL = ['--caption_model', 'updown', '--rnn_size', '32', '--input_encoding_size', '32', '--att_hid_size', '16', '--fc_feat_size', '24',
         '--att_feat_size', '24', '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6', '--max_length', '6',
         '--batch_size', '4', '--seq_per_img', '2', '--synthetic_images', '12', '--use_warmup', '1', '--noamopt_warmup', '6',
         '--learning_rate', '0.01', '--drop_prob_lm', '0.5']


def _opts(argv):
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    return opts.parse_opt(argv)


def _train(argv):
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    opt = _opts(argv)
    T.train(opt)
    return opt


def _six(path, extra=()):
    return _train(SMALL + ['--max_iters', '6', '--save_checkpoint_every', '6', '--checkpoint_path', str(path)] + list(extra))


@pytest.fixture(scope='module')
def six_iterations(tmp_path_factory):
    """6 iterations with --ema_decay 0.9, run once: the options, the directory, and what a hook on FlatParams.ema_update_dyn saw at
    every step -- the average before the first update and the parameters the optimizer had just written."""
    from imagecaptioning.pytorch_amd import flat as F
    path = tmp_path_factory.mktemp('ema') / 'a'
    seen = {'ps': [], 'steps': []}
    orig = F.FlatParams.ema_update_dyn

    def spy(self, state):
        if not seen['ps']:
            seen['ema0'], seen['flat'] = self.ema.clone(), self
        seen['ps'].append(self.flat.clone())
        orig(self, state)
        seen['steps'].append(int(state.read().adam_step))

    F.FlatParams.ema_update_dyn = spy
    try:
        opt = _six(path, ['--ema_decay', '0.9'])
    finally:
        F.FlatParams.ema_update_dyn = orig
    return opt, path, seen


def test_trainer_writes_an_average_that_loads_and_equals_the_float64_replay(six_iterations):
    sys.path.insert(0, PKG)
    from captioning import models
    opt, path, seen = six_iterations
    assert seen['steps'] == [1, 2, 3, 4, 5, 6]                                            # once per iteration, behind the optimizer
    raw, avg = torch.load(path / 'model.pth'), torch.load(path / 'model_ema.pth')
    assert list(raw) == list(avg)
    models.setup(opt).load_state_dict(avg)                                               # strict
    assert any(not torch.equal(raw[k], avg[k]) for k in raw)
    flat = seen['flat']
    assert not torch.equal(seen['ema0'], seen['ps'][0])                                  # it started as the initial parameters' copy
    ref =R.replay(seen['ema0'], seen['ps'], 0.9, 1)
    tol = R.atol(6, seen['ema0'], *seen['ps'])
    worst = 0.0
    for n, p, o in zip(flat.names, flat.params, flat.offsets):
        err = float((avg[n].to(DEV).double().reshape(-1) - ref[o:o + p.numel()]).abs().max())
        worst = max(worst, err)
        assert err <= tol, (n, err, tol)
        assert torch.equal(raw[n].to(DEV).reshape(-1), seen['ps'][-1][o:o + p.numel()])
    print('model_ema.pth: worst |trainer - float64 replay| %.3g, bound %.3g' % (worst, tol))
    osd = torch.load(path / 'optimizer.pth', weights_only=False)['flat']
    assert osd['ema_decay'] == 0.9 and osd['ema_warmup'] is True and osd['step_count'] == 6
    for n, p, o in zip(flat.names, flat.params, flat.offsets):
        assert torch.equal(osd['ema'][o:o + p.numel()], avg[n].reshape(-1))
    # tools/eval.py --model reads the file by path: the averaged weights decode, and score another loss than the raw ones
    from imagecaptioning.pytorch_amd.tools import eval as E
    small = SMALL[:SMALL.index('--use_warmup')]                                          # the model and data options, not the schedule's
    loss_avg, preds = E.main(_opts(small + ['--num_images', '4', '--model', str(path / 'model_ema.pth')]))
    loss_raw, _ = E.main(_opts(small + ['--num_images', '4', '--start_from', str(path)]))
    assert len(preds) == 4 and loss_avg == loss_avg and loss_avg != loss_raw


def test_resumed_average_is_the_uninterrupted_average_bit_for_bit(six_iterations, tmp_path):
    """3 iterations, checkpoint, --start_from, 3 more == 6 straight: optimizer.pth carries the average and the step count its
    warm-up reads"""
    _, a, _ = six_iterations
    b = tmp_path / 'b'
    common = SMALL + ['--ema_decay', '0.9', '--checkpoint_path', str(b)]
    _train(common + ['--max_iters', '3', '--save_checkpoint_every', '3'])
    half = torch.load(b / 'optimizer.pth', weights_only=False)['flat']
    assert half['step_count'] == 3 and 'ema' in half
    _train(common + ['--max_iters', '6', '--save_checkpoint_every', '6', '--start_from', str(b)])
    ea, eb = torch.load(a / 'model_ema.pth'), torch.load(b / 'model_ema.pth')
    assert list(ea) == list(eb)
    for k in ea:
        assert torch.equal(_bits(ea[k]), _bits(eb[k])), (k, float((ea[k] - eb[k]).abs().max()))
    sa, sb = (torch.load(d / 'optimizer.pth', weights_only=False)['flat'] for d in (a, b))
    assert sa['step_count'] == sb['step_count'] == 6 and torch.equal(_bits(sa['ema']), _bits(sb['ema']))
    assert not torch.equal(half['ema'], sb['ema'])


def test_captured_step_and_stepped_step_give_the_same_average(tmp_path, monkeypatch):
    """The same 6 iterations through the captured step (hipGraph replays that end in capmi_ema_step_dyn) and launch by launch
    (CAPMI_GRAPH_STEP=0): bit-equal averages.  On the tiny Transformer of test_entrypoints_gpu's captured-trainer test: the trainer
    captures the Transformer and AoA families only -- an UpDown step cannot be captured (Optimizers), so under UpDown both
    runs would be the stepped path."""
    from imagecaptioning.pytorch_amd import graph_step as G
    tiny = ['--caption_model', 'transformer', '--d_model', '32', '--d_ff', '64', '--N_enc', '1', '--N_dec', '1', '--num_att_heads', '4',
            '--input_encoding_size', '32', '--rnn_size', '32', '--noamopt', '1', '--noamopt_warmup', '5', '--noamopt_factor', '1.0',
            '--fc_feat_size', '24', '--att_feat_size', '24', '--vocab_size', '40', '--synthetic_regions', '5', '--seq_length', '6',
            '--max_length', '6', '--batch_size', '4', '--seq_per_img', '2', '--synthetic_images', '8', '--max_iters', '6',
            '--save_checkpoint_every', '6', '--ema_decay', '0.9']
    made = []
    orig = G.TrainStep.__init__

    def spy(self, *a, **kw):
        orig(self, *a, **kw)
        made.append(self)

    monkeypatch.setattr(G.TrainStep, '__init__', spy)
    out = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('CAPMI_GRAPH_STEP', mode)
        d = tmp_path / ('g' + mode)
        _train(tiny + ['--checkpoint_path', str(d)])
        out[mode] = (torch.load(d / 'model_ema.pth'), torch.load(d / 'model.pth'))
    captured, stepped = made
    assert captured.failed is None and captured.captures >= 1 and captured.replays >= 1 and captured.replays + captured.stepped == 6
    assert stepped.captures == 0 and stepped.stepped == 6
    for k in out['1'][0]:
        assert torch.equal(_bits(out['1'][0][k]), _bits(out['0'][0][k])), k
        assert torch.equal(_bits(out['1'][1][k]), _bits(out['0'][1][k])), k
    assert any(not torch.equal(out['1'][0][k], out['1'][1][k]) for k in out['1'][0])


def test_decay_zero_is_the_run_without_the_option(tmp_path):
    """--ema_decay 0: no model_ema.pth, no 'ema' in optimizer.pth, and the parameters of the run with the option left out, to the bit"""
    a, b = tmp_path / 'off', tmp_path / 'none'
    _six(a, ['--ema_decay', '0'])
    _six(b)
    for d in (a, b):
        assert not (d / 'model_ema.pth').exists() and sorted(os.listdir(d)) == ['infos_capmi.pkl', 'model.pth', 'optimizer.pth']
        osd = torch.load(d / 'optimizer.pth', weights_only=False)['flat']
        assert not {'ema', 'ema_decay', 'ema_warmup'} & set(osd)
    pa, pb = torch.load(a / 'model.pth'), torch.load(b / 'model.pth')
    assert list(pa) == list(pb)
    for k in pa:
        assert torch.equal(_bits(pa[k]), _bits(pb[k])), k


def test_average_does_not_disturb_the_raw_weights_and_ema_eval_validates_on_it(six_iterations, tmp_path, monkeypatch):
    """the raw parameters of a run with the average are those of a run without it, to the bit; so are those of a run whose periodic
    validation swaps the average in and out (--ema_eval 1) and of one that validates on the raw weights (--ema_eval 0), while the
    validation losses of the two differ: with --ema_eval 1 the model holds the average while it is validated"""
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import train as T
    _, with_ema, _ = six_iterations
    plain = tmp_path / 'plain'
    _six(plain)
    pa, pb = torch.load(with_ema / 'model.pth'), torch.load(plain / 'model.pth')
    for k in pa:
        assert torch.equal(_bits(pa[k]), _bits(pb[k])), k
    orig = T.validation_loss
    seen = []

    def spy(lw_model, *a, **kw):
        flat = lw_model.model._flat
        before = (flat.flat.clone(), flat.ema.clone())
        tot, n = orig(lw_model, *a, **kw)
        assert torch.equal(flat.flat, before[0]) and torch.equal(flat.ema, before[1])        # validation writes neither
        seen.append((tot, n, before))
        return tot, n

    monkeypatch.setattr(T, 'validation_loss', spy)
    runs = {}
    for ev in ('1', '0'):
        d = tmp_path / ('ev' + ev)
        del seen[:]
        _six(d, ['--ema_decay', '0.9', '--ema_eval', ev, '--val_every', '3', '--val_images', '4'])
        assert len(seen) == 2 and all(n > 0 for _, n, _ in seen)
        runs[ev] = (list(seen), torch.load(d / 'model.pth'), torch.load(d / 'model_ema.pth'))
    for k in runs['1'][1]:
        assert torch.equal(_bits(runs['1'][1][k]), _bits(runs['0'][1][k])), k
        assert torch.equal(_bits(runs['1'][2][k]), _bits(runs['0'][2][k])), k
    for (t1, n1, (held1, other1)), (t0, n0, (held0, other0)) in zip(runs['1'][0], runs['0'][0]):
        assert n1 == n0 and t1 != t0
        assert torch.equal(held1, other0) and torch.equal(other1, held0)                     # --ema_eval 1 validated on the other run's average
