"""Att2in2 (caption_model att2in2, configs/a2i2*.yml) without a GPU: the fp64 restatement reproduces the reference's fixture,
the model's parameter tree is the reference's, and the new C structs match their ctypes mirrors."""
import argparse
import os
import re

import numpy as np
import torch

from conftest import ROOT, GOLDEN
import att2in2_ref64 as ref

Z = os.path.join(GOLDEN, 'att2in2_tiny.npz')


def tiny_opt(**kw):
    V = 30
    o = argparse.Namespace(caption_model='att2in2', vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1,
                           drop_prob_lm=0.0, seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=12,
                           use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _load():
    z = np.load(Z)
    P = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('P.')}
    return z, P


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


def _close_grads(g, z, prefix):
    for k, v in g.items():
        r = z[prefix + k]
        np.testing.assert_allclose(v.numpy(), r, rtol=1e-4, atol=1e-6 + 1e-5 * np.abs(r).max(), err_msg=k)


def test_restatement_reproduces_the_reference_fixture():
    z, P = _load()
    att, am = torch.from_numpy(z['att']), torch.from_numpy(z['att_masks'])
    labels, masks = torch.from_numpy(z['labels']), torch.from_numpy(z['masks'])
    # eval-mode XE (ragged att_masks): log-probs, loss, every gradient
    logp = ref.xe(P, att, am, labels[..., :-1])
    np.testing.assert_allclose(logp.numpy(), z['xe_logp'], rtol=1e-5, atol=1e-6)
    loss, g = _grads(P, lambda Pg: _xe_loss(ref.xe(Pg, att, am, labels[..., :-1]), labels, masks))
    np.testing.assert_allclose(loss.item(), z['xe_loss'], rtol=1e-5)
    _close_grads(g, z, 'xe_grad.')
    # greedy decode
    seq, slp = ref.rollout(P, att, am, 1, 8)
    assert np.array_equal(seq.numpy(), z['greedy_seq'])
    np.testing.assert_allclose(slp.numpy(), z['greedy_logp'], rtol=1e-5, atol=1e-6)
    # RewardCriterion over the fixed (greedy, sample_n 2) sequence
    seq, slp = ref.rollout(P, att, am, 2, 8)
    assert np.array_equal(seq.numpy(), z['rl_seq'])
    np.testing.assert_allclose(slp.numpy(), z['rl_logp'], rtol=1e-5, atol=1e-6)
    reward = torch.from_numpy(z['rl_reward']).to(ref.D)

    def rl(Pg):
        s, lp = ref.rollout(Pg, att, am, 2, 8)
        sel = lp.gather(2, s.unsqueeze(2)).squeeze(2)
        m = torch.cat([torch.ones(s.shape[0], 1, dtype=ref.D), (s > 0).to(ref.D)[:, :-1]], 1)
        return -(sel * reward * m).sum() / m.sum()
    loss, g = _grads(P, rl)
    np.testing.assert_allclose(loss.item(), z['rl_loss'], rtol=1e-5)
    _close_grads(g, z, 'rl_grad.')
    # train mode, recorded dropout masks (no att_masks)
    T_steps = z['train_logp'].shape[1] - 1          # the trailing all-pad column is not run
    drops = ref.unpack_drops(z, 'train', T_steps)
    logp = ref.xe(P, att, None, labels[..., :-1], *drops)
    np.testing.assert_allclose(logp.numpy(), z['train_logp'], rtol=1e-5, atol=1e-6)
    loss, g = _grads(P, lambda Pg: _xe_loss(ref.xe(Pg, att, None, labels[..., :-1], *drops), labels, masks))
    np.testing.assert_allclose(loss.item(), z['train_loss'], rtol=1e-5)
    _close_grads(g, z, 'train_grad.')


def test_fixture_has_mixed_lengths_and_a_distinct_beam():
    z, _ = _load()
    lens = (z['greedy_seq'] > 0).sum(1)
    assert lens.min() < lens.max()
    assert not np.array_equal(z['beam3_seq'], z['greedy_seq'])


def test_setup_builds_the_reference_parameter_tree():
    from imagecaptioning.pytorch_amd.captioning import models
    z, P = _load()
    m = models.setup(tiny_opt())
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in P.items()}
    m.load_state_dict(P)
    h, c = m.init_hidden(4)
    assert h.shape == (1, 4, 16) and c.shape == (1, 4, 16)
    assert m.fc_embed is not None and torch.equal(m.fc_embed(torch.ones(2)), torch.ones(2))
    # att2in stays out of scope
    import pytest
    with pytest.raises(NotImplementedError):
        models.setup(tiny_opt(caption_model='att2in'))


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

    pairs = {'capmi_att2in2_weights': _lib.Att2in2Weights, 'capmi_att2in2_rollout': _lib.Att2in2Rollout,
             'capmi_att2in2_grads': _lib.Att2in2Grads, 'capmi_att2in2_bwd_scratch': _lib.Att2in2BwdScratch,
             'capmi_att2in2_step': _lib.Att2in2Step}
    for cname, cls in pairs.items():
        assert fields(cname) == [f[0] for f in cls._fields_], cname
