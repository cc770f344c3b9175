"""AdaAtt (caption_model adaatt / adaattmo) without a GPU: the fp64 restatement reproduces the reference's fixture (both variants),
the models' parameter trees are the reference's, the constructor refuses what the kernels do not cover, and the new C structs
match their ctypes mirrors."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN
import adaatt_ref64 as ref

Z = os.path.join(GOLDEN, 'adaatt_tiny.npz')
VARIANTS = ('adaatt', 'adaattmo')


def tiny_opt(name='adaatt', **kw):
    V = 30
    o = argparse.Namespace(caption_model=name, vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1,
                           drop_prob_lm=0.0, seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=16,
                           use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Fixture:
    """the arrays of one variant"""

    def __init__(self, name):
        self.z, self.pre = np.load(Z), name + '.'
        self.files = [k[len(self.pre):] for k in self.z.files if k.startswith(self.pre)]

    def __getitem__(self, k):
        return self.z[self.pre + k]

    def t(self, k):
        return torch.from_numpy(self[k])

    def params(self):
        return {k[2:]: self.t(k) for k in self.files if k.startswith('P.')}


def ss_draws(fx):
    """the reference's scheduled-sampling inputs without its RNG (as tests/test_ss_host.py): coin = the fed token differs from the
    label, noise = a large constant at the fed token"""
    fed = fx.t('ss_fed')
    T_eff, N = fed.shape
    seq = fx.t('labels')[..., :-1].reshape(N, -1)
    coin = fed != seq[:, :T_eff].t()
    gum = torch.zeros(T_eff, N, 31)
    for t in range(1, T_eff):
        gum[t - 1].scatter_(1, fed[t].unsqueeze(1), 1e4)
    return coin, gum


def _xe_loss(logp, labels, masks):
    """LanguageModelCriterion (losses.py:203-219) in fp64"""
    T = logp.shape[1]
    tgt = labels[..., 1:].reshape(logp.shape[0], -1)[:, :T]
    m = masks[..., 1:].reshape(logp.shape[0], -1)[:, :T].to(ref.D)
    return -(logp.gather(2, tgt.unsqueeze(2)).squeeze(2) * m).sum() / m.sum()


def _grads(P, fn):
    Pg = {k: v.to(ref.D).requires_grad_(True) for k, v in P.items()}
    loss = fn(Pg)
    loss.backward()
    return loss, {k: v.grad for k, v in Pg.items()}


def _close_grads(g, fx, prefix):
    for k, v in g.items():
        r = fx[prefix + k]
        np.testing.assert_allclose(v.numpy(), r, rtol=1e-4, atol=1e-6 + 1e-5 * np.abs(r).max(), err_msg=k)


@pytest.mark.parametrize('name', VARIANTS)
def test_restatement_reproduces_the_reference_fixture(name):
    fx = Fixture(name)
    P = fx.params()
    fc, att, am = fx.t('fc'), fx.t('att'), fx.t('att_masks')
    labels, masks = fx.t('labels'), fx.t('masks')
    # eval-mode XE (ragged att_masks): log-probs, loss, every gradient
    logp = ref.xe(P, fc, att, am, labels[..., :-1])
    np.testing.assert_allclose(logp.numpy(), fx['xe_logp'], rtol=1e-5, atol=1e-6)
    loss, g = _grads(P, lambda Pg: _xe_loss(ref.xe(Pg, fc, att, am, labels[..., :-1]), labels, masks))
    np.testing.assert_allclose(loss.item(), fx['xe_loss'], rtol=1e-5)
    _close_grads(g, fx, 'xe_grad.')
    # greedy decode
    seq, slp = ref.rollout(P, fc, att, am, 1, 8)
    assert np.array_equal(seq.numpy(), fx['greedy_seq'])
    np.testing.assert_allclose(slp.numpy(), fx['greedy_logp'], rtol=1e-5, atol=1e-6)
    # RewardCriterion over the fixed (greedy, sample_n 2) sequence
    seq, slp = ref.rollout(P, fc, att, am, 2, 8)
    assert np.array_equal(seq.numpy(), fx['rl_seq'])
    np.testing.assert_allclose(slp.numpy(), fx['rl_logp'], rtol=1e-5, atol=1e-6)
    reward = fx.t('rl_reward').to(ref.D)

    def rl(Pg):
        s, lp = ref.rollout(Pg, fc, att, am, 2, 8)
        sel = lp.gather(2, s.unsqueeze(2)).squeeze(2)
        m = torch.cat([torch.ones(s.shape[0], 1, dtype=ref.D), (s > 0).to(ref.D)[:, :-1]], 1)
        return -(sel * reward * m).sum() / m.sum()
    loss, g = _grads(P, rl)
    np.testing.assert_allclose(loss.item(), fx['rl_loss'], rtol=1e-5)
    _close_grads(g, fx, 'rl_grad.')
    # train mode, the recorded dropout masks replayed in recorded order (no att_masks): this pins the dropout sites
    T_steps = fx['train_logp'].shape[1] - 1          # the trailing all-pad column is not run
    drops = ref.unpack_drops(fx.z, name + '.train', T_steps)
    assert drops['tile'].shape == (T_steps, 6, 7, 16) and drops['fc'].shape == (3, 16)
    logp = ref.xe(P, fc, att, None, labels[..., :-1], drops)
    np.testing.assert_allclose(logp.numpy(), fx['train_logp'], rtol=1e-5, atol=1e-6)
    loss, g = _grads(P, lambda Pg: _xe_loss(ref.xe(Pg, fc, att, None, labels[..., :-1], drops), labels, masks))
    np.testing.assert_allclose(loss.item(), fx['train_loss'], rtol=1e-5)
    _close_grads(g, fx, 'train_grad.')
    # scheduled sampling with the recorded inputs
    coin, gum = ss_draws(fx)
    logp = ref.xe(P, fc, att, am, labels[..., :-1], ss_coin=coin, ss_gumbel=gum)
    np.testing.assert_allclose(logp.numpy(), fx['ss_logp'], rtol=1e-5, atol=1e-6)
    loss, g = _grads(P, lambda Pg: _xe_loss(ref.xe(Pg, fc, att, am, labels[..., :-1], ss_coin=coin, ss_gumbel=gum), labels, masks))
    np.testing.assert_allclose(loss.item(), fx['ss_loss'], rtol=1e-5)
    _close_grads(g, fx, 'ss_grad.')


@pytest.mark.parametrize('name', VARIANTS)
def test_fixture_decodes_are_not_degenerate(name):
    fx = Fixture(name)
    for key in ('greedy_seq', 'rl_seq', 'beam3_seq'):
        seq = fx[key]
        lens = (seq > 0).sum(1)
        for row, ln in zip(seq, lens):
            assert ln < 2 or len(set(row[:ln].tolist())) > 1, (key, row)
    lens = (fx['greedy_seq'] > 0).sum(1)
    assert lens.min() < 8 and lens.max() == 8
    assert not np.array_equal(fx['beam3_seq'], fx['greedy_seq'])
    assert float(fx['beam3_min_gap']) >= 1e-3
    assert int((fx['ss_fed'] != fx['labels'][..., :-1].reshape(6, -1)[:, :fx['ss_fed'].shape[0]].T).sum()) > 10


@pytest.mark.parametrize('name', VARIANTS)
def test_setup_builds_the_reference_parameter_tree(name):
    from imagecaptioning.pytorch_amd.captioning import models
    fx = Fixture(name)
    P = fx.params()
    m = models.setup(tiny_opt(name))
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in P.items()}
    m.load_state_dict(P)
    h, c = m.init_hidden(4)
    assert h.shape == (1, 4, 16) and c.shape == (1, 4, 16)
    assert m.core.lstm.w2h.weight.shape[0] == (80 if name == 'adaattmo' else 64)


def test_constructor_refusals_and_out_of_scope_names():
    from imagecaptioning.pytorch_amd.captioning import models
    with pytest.raises(NotImplementedError, match='16, 16, 12'):
        models.setup(tiny_opt(att_hid_size=12))
    with pytest.raises(NotImplementedError, match='16, 24, 16'):
        models.setup(tiny_opt(rnn_size=24))
    for kw in (dict(num_layers=2), dict(use_bn=1), dict(logit_layers=2), dict(eos_idx=1), dict(bos_idx=2), dict(pad_idx=3)):
        for name in VARIANTS:
            with pytest.raises(NotImplementedError):
                models.setup(tiny_opt(name, **kw))
    for name in ('att2in', 'att2all2', 'stackatt', 'denseatt', 'fc', 'show_tell'):
        assert name in models._OUT_OF_SCOPE
        with pytest.raises(NotImplementedError):
            models.setup(tiny_opt(name))
    assert 'adaatt' not in models._OUT_OF_SCOPE and 'adaattmo' not in models._OUT_OF_SCOPE


def test_new_struct_layouts_match_header():
    """Field order of the ctypes structs == field order in include/capmi.h (same parsing as tests/test_abi.py)."""
    from imagecaptioning.pytorch_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'capmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)

    def fields(struct):
        body = re.search(r'typedef struct (?:%s )?\{([^{}]*?)\} %s;' % (struct, struct), src, flags=re.S).group(1)
        names = []
        for stmt in body.split(';'):
            stmt = stmt.strip()
            if not stmt:
                continue
            for part in stmt.split(','):
                names.append(re.findall(r'(\w+)\s*(?:\[\w+\])?$', part.strip())[0])
        return names

    pairs = {'capmi_tile_drop': _lib.TileDrop, 'capmi_adaatt_weights': _lib.AdaAttWeights, 'capmi_adaatt_rollout': _lib.AdaAttRollout,
             'capmi_adaatt_grads': _lib.AdaAttGrads, 'capmi_adaatt_bwd_scratch': _lib.AdaAttBwdScratch,
             'capmi_adaatt_step': _lib.AdaAttStep}
    for cname, cls in pairs.items():
        assert fields(cname) == [f[0] for f in cls._fields_], cname
