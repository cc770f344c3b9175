"""The exponential moving average of the parameters (--ema_decay), host side: the two entry points against the header, the three
command-line switches, and the bookkeeping of flat.FlatParams (enable_ema, state_dict / load_state_dict, ema_state_dict, swap_ema)
on CPU tensors.  What needs the device kernel (ema_update, ema_update_dyn) is in test_ema_gpu.py."""
import argparse
import os
import re
import sys

import pytest
import torch

import ema_ref64 as R
from conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'capmi.h')
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')


def _declared():
    """[(name, argument count)] of the header's prototypes in the order they are declared (the parsing of test_abi.declared)"""
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = []
    for m in re.finditer(r'\b(?:int|int64_t|const char \*)\s*(capmi_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        args = m.group(2).strip()
        out.append((m.group(1), 0 if args in ('', 'void') else len(args.split(',')), args))
    return out


def test_entry_points_follow_the_optimizers_in_header_and_binding():
    from imagecaptioning.pytorch_amd import _lib
    d = _declared()
    names = [n for n, _, _ in d]
    i = names.index('capmi_optim_step_dyn')
    assert names[i + 1:i + 3] == ['capmi_ema_step', 'capmi_ema_step_dyn']
    bound = list(_lib.SIGNATURES)
    j = bound.index('capmi_optim_step_dyn')
    assert bound[j + 1:j + 3] == ['capmi_ema_step', 'capmi_ema_step_dyn']            # the same order in the ctypes table
    by_name = {n: (k, a) for n, k, a in d}
    assert by_name['capmi_ema_step'][0] == 7 and by_name['capmi_ema_step_dyn'][0] == 7
    for n in ('capmi_ema_step', 'capmi_ema_step_dyn'):
        assert len(_lib.SIGNATURES[n]) == by_name[n][0]
    words = lambda a: [re.findall(r'(\w+)$', part.strip())[0] for part in a.split(',')]      # noqa: E731
    assert words(by_name['capmi_ema_step'][1]) == ['ema', 'p', 'count', 'decay', 'warmup', 'step', 'stream']
    assert words(by_name['capmi_ema_step_dyn'][1]) == ['ema', 'p', 'count', 'state', 'decay', 'warmup', 'stream']
    # the record the _dyn form reads its step number from: layout unchanged
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct (?:capmi_step_state )?\{([^{}]*?)\} capmi_step_state;', src, flags=re.S).group(1)
    fields = []
    for stmt in body.split(';'):
        for part in (stmt.strip().split(',') if stmt.strip() else []):
            fields.append(re.findall(r'(\w+)\s*(?:\[\w+\])?$', part.strip())[0])
    assert fields == [f[0] for f in _lib.StepState._fields_] and fields[1] == 'adam_step'


def test_the_three_switches_default_to_off_on_on():
    sys.path.insert(0, PKG)
    from captioning.utils import opts
    assert (opts.DEFAULTS['ema_decay'], opts.DEFAULTS['ema_warmup'], opts.DEFAULTS['ema_eval']) == (0.0, 1, 1)
    o = opts.parse_opt([])
    assert o.ema_decay == 0.0 and o.ema_warmup == 1 and o.ema_eval == 1
    o = opts.parse_opt(['--ema_decay', '0.999', '--ema_warmup', '0', '--ema_eval', '0'])
    assert o.ema_decay == 0.999 and o.ema_warmup == 0 and o.ema_eval == 0
    import json
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'opts_defaults.json')))
    assert not {'ema_decay', 'ema_warmup', 'ema_eval'} & set(ref)                      # not flags of the reference: nothing to agree with


def _net():
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))


def test_enable_ema_and_state_dict_round_trip():
    from imagecaptioning.pytorch_amd.flat import FlatParams
    torch.manual_seed(0)
    a = FlatParams(_net())
    assert a.ema is None and 'ema' not in a.state_dict()                              # off: no buffer, no key
    with pytest.raises(RuntimeError, match='enable_ema'):
        a.swap_ema()
    for bad in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            a.enable_ema(bad)
    a.enable_ema(0.99, warmup=False)
    assert a.ema.shape == a.flat.shape and a.ema.dtype == torch.float32 and a.ema.data_ptr() != a.flat.data_ptr()
    assert torch.equal(a.ema, a.flat) and a.ema_decay == 0.99 and a.ema_warmup is False
    a.ema.copy_(torch.arange(a.total, dtype=torch.float32))
    a.exp_avg.fill_(2.0)
    a.step_count = 4
    sd = a.state_dict()
    assert sd['ema_decay'] == 0.99 and sd['ema_warmup'] is False and sd['ema'].shape == (a.total,)
    assert sd['ema'].data_ptr() != a.ema.data_ptr()
    b = FlatParams(_net())
    b.enable_ema(0.5)
    b.load_state_dict(sd)
    assert torch.equal(b.ema, a.ema) and torch.equal(b.exp_avg, a.exp_avg) and b.step_count == 4
    assert b.ema_decay == 0.5 and b.ema_warmup is True                                # the object keeps what enable_ema() was given


def test_cross_loading(capsys):
    from imagecaptioning.pytorch_amd.flat import FlatParams
    torch.manual_seed(1)
    plain = FlatParams(_net())
    plain.exp_avg.fill_(3.0)
    plain.step_count = 2
    sd_plain = plain.state_dict()
    # a file without an average into an object with one: the average starts from the (loaded) parameters, said once
    torch.manual_seed(2)
    e = FlatParams(_net())
    e.enable_ema(0.9)
    e.ema.zero_()
    capsys.readouterr()
    e.load_state_dict(sd_plain)
    e.load_state_dict(sd_plain)
    out = capsys.readouterr().out
    assert out.count('moving average') == 1 and 'starts from the loaded parameters' in out
    assert torch.equal(e.ema, e.flat) and float(e.ema.abs().max()) > 0 and e.step_count == 2
    assert torch.equal(e.exp_avg, plain.exp_avg)
    # a file with an average into an object without one: the key is ignored
    e.ema.fill_(7.0)
    sd_ema = e.state_dict()
    assert 'ema' in sd_ema
    q = FlatParams(_net())
    q.load_state_dict(sd_ema)
    assert q.ema is None and 'ema' not in q.state_dict() and torch.equal(q.exp_avg, e.exp_avg)


def test_the_average_moves_by_name_when_the_layout_differs():
    """a state saved in another segment order (the 'offsets' table of the file): the average follows its parameters like the moments"""
    from imagecaptioning.pytorch_amd.flat import FlatParams
    torch.manual_seed(3)
    a = FlatParams(_net())
    a.enable_ema(0.9)
    a.ema.copy_(torch.arange(a.total, dtype=torch.float32))
    sd = a.state_dict()
    order = list(reversed(a.names))                                                    # the same segments, laid out back to front
    theirs, off = {}, 0
    for n in order:
        theirs[n] = off
        off += (a.params[a.names.index(n)].numel() + 3) // 4 * 4
    moved = {k: torch.zeros(a.total) for k in ('ema', 'exp_avg', 'exp_avg_sq')}
    for n, p, o in zip(a.names, a.params, a.offsets):
        for k in moved:
            moved[k][theirs[n]:theirs[n] + p.numel()] = sd[k][o:o + p.numel()]
    sd2 = dict(sd, offsets=theirs, **moved)
    b = FlatParams(_net())
    b.enable_ema(0.9)
    b.load_state_dict(sd2)
    for p, o in zip(a.params, a.offsets):
        assert torch.equal(b.ema[o:o + p.numel()], a.ema[o:o + p.numel()])


def test_ema_state_dict_has_the_modules_keys_and_passes_buffers_through():
    """a tiny use_bn = 1 UpDown: parameters come from the average, BatchNorm's running statistics are copied as they are"""
    from imagecaptioning.pytorch_amd.captioning import models
    V = 30
    opt = argparse.Namespace(caption_model='updown', vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1, drop_prob_lm=0.0,
                             seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=12, use_bn=1, logit_layers=1,
                             vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    torch.manual_seed(4)
    model = models.setup(opt)
    flat = model.flatten_parameters_('adam')
    flat.enable_ema(0.9)
    flat.ema.copy_(torch.arange(flat.total, dtype=torch.float32) + 0.5)
    own = model.state_dict()
    pnames = {n for n, _ in model.named_parameters()}
    buffers = [k for k in own if k not in pnames]
    assert any('running_mean' in k for k in buffers) and any('num_batches_tracked' in k for k in buffers)
    for k in buffers:
        if own[k].is_floating_point():
            own[k].copy_(torch.rand_like(own[k]) + 1.0)                               # state_dict() aliases the module's buffers
    esd = flat.ema_state_dict(model)
    assert list(esd) == list(model.state_dict())                                      # the module's keys, in the module's order
    for n, p, o in zip(flat.names, flat.params, flat.offsets):
        assert esd[n].shape == p.shape and torch.equal(esd[n].reshape(-1), flat.ema[o:o + p.numel()])
        assert not torch.equal(esd[n], p.detach())
        assert esd[n].data_ptr() != flat.ema.data_ptr() + 4 * o                        # a copy, not a view of the live average
    for k in buffers:
        assert torch.equal(esd[k], model.state_dict()[k]) and esd[k].data_ptr() != model.state_dict()[k].data_ptr()
    fresh = models.setup(opt)
    fresh.load_state_dict(esd)                                                        # strict: loads wherever model.pth does


def test_swap_ema_twice_is_the_identity():
    from imagecaptioning.pytorch_amd.flat import FlatParams
    torch.manual_seed(5)
    net = _net()
    f = FlatParams(net)
    f.enable_ema(0.9)
    f.ema.copy_(torch.randn(f.total))
    p0, e0 = f.flat.clone(), f.ema.clone()
    ptrs = (f.flat.data_ptr(), f.ema.data_ptr())
    f.swap_ema()
    assert torch.equal(f.flat, e0) and torch.equal(f.ema, p0)
    o = f.offsets[0]
    assert torch.equal(net[0].weight.detach().reshape(-1), e0[o:o + 35])              # the module sees the swap: its storage IS the buffer
    f.swap_ema()
    assert torch.equal(f.flat.view(torch.int32), p0.view(torch.int32)) and torch.equal(f.ema.view(torch.int32), e0.view(torch.int32))
    assert (f.flat.data_ptr(), f.ema.data_ptr()) == ptrs                              # in place: recorded pointers stay valid


def test_ref64_decay_schedule():
    """the replay's decay: the warm-up quotient below the cap, the cap above it; decay 0.5 crosses at step 8 ((1 + 8) / (10 + 8))"""
    assert R.decay_at(0.9, 0, 1) == float(torch.tensor(0.9, dtype=torch.float32))
    assert R.decay_at(0.9, 1, 1) == float(torch.tensor(2.0, dtype=torch.float32) / torch.tensor(11.0, dtype=torch.float32))
    assert [R.decay_at(0.5, 1, s) < 0.5 for s in (6, 7, 8, 9, 10)] == [True, True, False, False, False]
    assert R.decay_at(0.5, 1, 8) == 0.5 and R.decay_at(0.5, 1, 9) == 0.5
    e = R.replay(torch.zeros(3), [torch.ones(3)] * 2, 0.5, 0)
    assert torch.equal(e, torch.full((3,), 0.75, dtype=torch.float64))
    assert R.atol(20, torch.tensor([2.0]), torch.tensor([-4.0])) == 2 * 20 * 2.0 ** -24 * 4.0
