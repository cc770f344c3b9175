"""The optimizer rules of the fused flat-buffer step, host side: the float64 replay the GPU tests hold the kernels to is pinned to the
torch.optim classes as the reference's misc.build_optimizer constructs them; the trainer's option mapping; the new ABI struct."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch

import optim_ref64 as R
from conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'capmi.h')


def _opt(name, wd):
    # values that differ from every torch default, so that a number handed to the wrong constructor argument shows
    return argparse.Namespace(optim=name, learning_rate=3e-3, optim_alpha=0.8, optim_beta=0.95, optim_epsilon=1e-6, weight_decay=wd)


def _reference_optimizer(params, opt):
    """the constructor calls of the reference's captioning/utils/misc.py build_optimizer, argument for argument"""
    optim = torch.optim
    if opt.optim == 'rmsprop':
        return optim.RMSprop(params, opt.learning_rate, opt.optim_alpha, opt.optim_epsilon, weight_decay=opt.weight_decay)
    if opt.optim == 'adagrad':
        return optim.Adagrad(params, opt.learning_rate, weight_decay=opt.weight_decay)
    if opt.optim == 'sgdm':
        return optim.SGD(params, opt.learning_rate, opt.optim_alpha, weight_decay=opt.weight_decay)
    if opt.optim == 'sgdmom':
        return optim.SGD(params, opt.learning_rate, opt.optim_alpha, weight_decay=opt.weight_decay, nesterov=True)
    if opt.optim == 'adam':
        return optim.Adam(params, opt.learning_rate, (opt.optim_alpha, opt.optim_beta), opt.optim_epsilon, weight_decay=opt.weight_decay)
    if opt.optim == 'adamw':
        return optim.AdamW(params, opt.learning_rate, (opt.optim_alpha, opt.optim_beta), opt.optim_epsilon, weight_decay=opt.weight_decay)
    raise AssertionError(opt.optim)


def _misc():
    from imagecaptioning.pytorch_amd.captioning.utils import misc
    return misc


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('rule', R.RULES + ('adam',))
def test_ref64_is_torch_optim_as_the_reference_builds_it(rule, wd):
    """5 steps in float64 on the CPU: optim_ref64, fed with what the trainer's mapping makes of the options, against the torch
    optimizer the reference would have built from the same options.  The rate moves between the steps; the replay's clip and scale
    are applied to the gradient torch receives."""
    opt = _opt(rule, wd)
    hp = _misc().build_optimizer(opt)
    assert hp['rule'] == rule
    g = torch.Generator().manual_seed(11)
    n = 257
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    p_t = p0.clone().requires_grad_(True)
    tor = _reference_optimizer([p_t], opt)
    p, state = p0.clone(), R.new_state(rule, p0)
    clip, scale = 0.1, 0.6
    for t in range(1, 6):
        gr = torch.randn(n, generator=g, dtype=torch.float64) * 0.3
        lr = opt.learning_rate / t
        for grp in tor.param_groups:
            grp['lr'] = lr
        p_t.grad = (gr * scale).clamp(-clip, clip)
        tor.step()
        R.step(rule, p, gr, state, lr, t, alpha=hp['betas'][0], beta=hp['betas'][1], eps=hp['eps'], weight_decay=hp['weight_decay'],
               clip=clip, grad_scale=scale)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())      # noqa: E731
    assert rel(p, p_t.detach()) < 1e-12
    ts = tor.state[p_t]
    assert set(R.STATE_KEYS[rule]) <= set(ts)                           # the state buffers carry torch's key names
    for k in R.STATE_KEYS[rule]:
        assert rel(state[k], ts[k]) < 1e-12, k


def test_option_mapping_of_the_trainer():
    """tools/train.py builds its rule with misc.build_optimizer: every name of the reference's build_optimizer but plain sgd maps to
    a rule and the numbers the reference hands that rule's constructor"""
    misc = _misc()
    src = open(os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd', 'tools', 'train.py')).read()
    assert 'misc.build_optimizer(opt)' in src and "flatten_parameters_(optim['rule'])" in src
    want_eps = {'rmsprop': 1e-6, 'adagrad': 1e-10, 'sgdm': 1e-6, 'sgdmom': 1e-6, 'adam': 1e-6, 'adamw': 1e-6}
    for name, eps in want_eps.items():
        hp = misc.build_optimizer(_opt(name, 0.02))
        assert hp == {'rule': name, 'betas': (0.8, 0.95), 'eps': eps, 'weight_decay': 0.02}, (name, hp)
    with pytest.raises(NotImplementedError, match='sgd'):
        misc.build_optimizer(_opt('sgd', 0.0))
    with pytest.raises(Exception, match='bad option opt.optim: lion'):
        misc.build_optimizer(_opt('lion', 0.0))
    from imagecaptioning.pytorch_amd import flat, ops
    assert set(flat.STATE_KEYS) == set(want_eps) and flat.STATE_KEYS == R.STATE_KEYS
    assert set(ops.OPTIM_RULES) == set(R.RULES)


def test_flat_params_state_follows_the_rule():
    """one state buffer for the one-state rules, named like torch's state key; a state saved under one rule does not load under
    another, and the message names both"""
    from imagecaptioning.pytorch_amd.flat import FlatParams
    net = lambda: torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))      # noqa: E731
    a = FlatParams(net(), 'rmsprop')
    assert a.rule == 'rmsprop' and a.square_avg.shape == a.flat.shape
    assert not hasattr(a, 'exp_avg') and not hasattr(a, 'exp_avg_sq')
    a.square_avg.copy_(torch.arange(a.total, dtype=torch.float32))
    a.step_count = 3
    sd = a.state_dict()
    assert sd['rule'] == 'rmsprop' and 'exp_avg' not in sd
    b = FlatParams(net(), 'rmsprop')
    b.load_state_dict(sd)
    assert torch.equal(b.square_avg, a.square_avg) and b.step_count == 3
    with pytest.raises(ValueError, match="'rmsprop'.*'sgdmom'"):
        FlatParams(net(), 'sgdmom').load_state_dict(sd)
    adam = FlatParams(net())
    assert adam.rule == 'adam' and adam.state_dict()['rule'] == 'adam'
    legacy = {k: v for k, v in adam.state_dict().items() if k != 'rule'}                  # written before the rule was recorded
    adam.load_state_dict(legacy)
    with pytest.raises(ValueError, match="'adam'.*'adagrad'"):
        FlatParams(net(), 'adagrad').load_state_dict(legacy)
    with pytest.raises(ValueError):
        FlatParams(net(), 'sgd')


def test_optim_hp_layout_matches_header():
    """capmi_optim_hp: field order, types and the rule numbers of the ctypes side against include/capmi.h (parsed like test_abi.py)"""
    from imagecaptioning.pytorch_amd import _lib
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    body = re.search(r'typedef struct (?:capmi_optim_hp )?\{([^{}]*?)\} capmi_optim_hp;', src, flags=re.S).group(1)
    ctype = {'int32_t': C.c_int32, 'float': C.c_float}
    fields = []
    for stmt in body.split(';'):
        stmt = stmt.strip()
        if not stmt:
            continue
        ty, names = stmt.split(None, 1)
        fields += [(nm.strip(), ctype[ty]) for nm in names.split(',')]
    assert fields == [(f[0], f[1]) for f in _lib.OptimHp._fields_]
    assert C.sizeof(_lib.OptimHp) == 4 * len(fields)
    for i, (nm, _) in enumerate(fields):
        assert getattr(_lib.OptimHp, nm).offset == 4 * i
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define CAPMI_OPTIM_(\w+) (\d+)', src)}
    from imagecaptioning.pytorch_amd import ops
    assert enum == {k.upper(): v for k, v in ops.OPTIM_RULES.items()}
    assert enum == {'RMSPROP': _lib.OPTIM_RMSPROP, 'ADAGRAD': _lib.OPTIM_ADAGRAD, 'SGDM': _lib.OPTIM_SGDM, 'SGDMOM': _lib.OPTIM_SGDMOM,
                    'ADAMW': _lib.OPTIM_ADAMW}
    d = {m.group(1): len(m.group(2).split(',')) for m in
         re.finditer(r'\bint\s*(capmi_optim_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S)}
    assert d == {'capmi_optim_step': 9, 'capmi_optim_step_dyn': 8}
    for name, n in d.items():
        assert len(_lib.SIGNATURES[name]) == n


def test_invalid_arguments_are_einval():
    """null pointers, n <= 0, an unknown rule, a missing second buffer for AdamW: CAPMI_EINVAL before anything is launched (no device
    is touched: the checks come first)"""
    from imagecaptioning.pytorch_amd import _lib
    lib = _lib.lib
    hp = _lib.OptimHp(rule=_lib.OPTIM_RMSPROP, alpha=0.9, beta=0.999, eps=1e-8, weight_decay=0.0, clip=0.0, grad_scale=1.0)
    buf = (C.c_float * 8)()
    a = C.addressof(buf)
    ok = (C.byref(hp), a, a, a, None, 8, 1e-3, 1, None)
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (5, 0), (5, -4), (7, 0)):
        args = list(ok)
        args[i] = bad
        assert lib.capmi_optim_step(*args) == _lib.EINVAL, i
    assert lib.capmi_optim_step_dyn(C.byref(hp), a, a, a, None, 8, None, None) == _lib.EINVAL
    for rule in (0, 6, -1):
        hp.rule = rule
        assert lib.capmi_optim_step(*ok) == _lib.EINVAL, rule
        assert lib.capmi_optim_step_dyn(C.byref(hp), a, a, a, None, 8, a, None) == _lib.EINVAL, rule
    hp.rule = _lib.OPTIM_ADAMW
    assert lib.capmi_optim_step(*ok) == _lib.EINVAL                       # AdamW needs its second buffer
    hp.rule = _lib.OPTIM_SGDM
    assert lib.capmi_optim_step(C.byref(hp), a + 2, a, a, None, 4, 1e-3, 1, None) == _lib.EINVAL      # a pointer off 4 bytes
