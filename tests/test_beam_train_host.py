"""Beam search as a training rollout (train_sample_method greedy, train_beam_size > 1) -- what can be checked without a GPU:

* tests/beam_train_ref64.py (search with masks by search row, finalise, lineage, forced replay) reproduces the REAL reference's
  train-mode beam search recorded in tests/golden/beam_train_tiny.npz: beams exactly, log-probs and every parameter gradient --
  this pins the lineage rule and the mask order before any kernel is involved;
* the NumPy restatement of the finalise rule equals beam.assemble_done_beams on CPU tensors;
* the header declares, the library exports and _lib binds the new entry points;
* the families without a training beam search refuse by name instead of returning log-probs without a graph.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import beam_train_ref64 as ref

RUNS = ('a3', 'a1', 'b3', 'b1')
BEAM, L = 3, 8


def load(family):
    z = np.load(os.path.join(GOLDEN, 'beam_train_tiny.npz'))
    pre = family + '.'
    zz = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    P = {k[2:]: torch.from_numpy(v) for k, v in zz.items() if k.startswith('P.')}
    return zz, P


def inputs(zz):
    fc, att = torch.from_numpy(zz['fc']), torch.from_numpy(zz['att'])
    am = torch.from_numpy(zz['att_masks']) if 'att_masks' in zz else None
    return fc, att, am


def test_fixture_is_a_fair_search():
    for family in ('updown', 'newfc'):
        zz, _ = load(family)
        assert float(zz['min_gap']) >= 1e-3
        lens = np.concatenate([(zz[t + '.seq'] > 0).sum(1) for t in RUNS])
        assert lens.min() < L - 1 and lens.max() >= L - 1          # some beams end early, some run to the end
        assert {float(zz[t + '.opt'][0]) for t in RUNS} == {0.0, 0.5}
        assert {int(zz[t + '.opt'][1]) for t in RUNS} == {1, 3}
        assert {str(zz[t + '.length_penalty']) for t in RUNS} == {'', 'wu_0.5'}


@pytest.mark.parametrize('tag', RUNS)
@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_ref64_reproduces_the_reference(family, tag):
    zz, P = load(family)
    fc, att, am = inputs(zz)
    drop, sample_n = float(zz[tag + '.opt'][0]), int(zz[tag + '.opt'][1])
    pen = str(zz[tag + '.length_penalty'])
    masks = ref.recorded_masks(zz, tag, family, fc.shape[0], BEAM, L, am) if drop > 0 else None
    r = ref.run(family, P, fc, att, am, BEAM, sample_n, L, pen, masks, reward=zz[tag + '.reward'])
    assert np.array_equal(r['seq'], zz[tag + '.seq'])
    np.testing.assert_allclose(r['logp'].numpy(), zz[tag + '.logp'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r['loss'], zz[tag + '.loss'], rtol=1e-5)
    for k in P:
        g = zz['%s.grad.%s' % (tag, k)]
        np.testing.assert_allclose(r['grads'][k].numpy(), g, rtol=1e-4, atol=1e-6 + 1e-5 * np.abs(g).max(), err_msg=k)
    # the lineage is what makes the dropout runs agree: a beam that changed rows must exist, or the fixture shows nothing
    if drop > 0 and sample_n == BEAM:
        lin = r['lineage']
        own = np.arange(lin.shape[1])[None, :]
        assert ((lin[1:] != own) & (lin[1:] >= 0)).any()


def random_tables(rng, B, bd, Lx, repeats):
    parent = rng.randint(0, bd, (Lx, B, bd)).astype(np.int32)
    parent[0] = 0
    token = rng.randint(0, 6, (Lx, B, bd)).astype(np.int64)
    score = -rng.rand(Lx, B, bd).astype(np.float32) * 20
    if repeats:
        score = np.round(score)                                  # many equal scores: the stable order decides
    ended = (token == 0).astype(np.uint8)
    ended[Lx - 1] = 1
    return parent, token, score, ended


@pytest.mark.parametrize('pen', ['', 'wu_0.7', 'avg_0'])
@pytest.mark.parametrize('repeats', [False, True])
def test_finalize_rule_equals_assemble_done_beams(pen, repeats):
    from imagecaptioning.pytorch_amd import beam

    class M:
        pass
    rng = np.random.RandomState(3 + repeats)
    for B, bd, Lx in ((4, 3, 6), (2, 5, 9), (3, 1, 4)):
        parent, token, score, ended = random_tables(rng, B, bd, Lx, repeats)
        V1 = 7
        logp_rows = torch.from_numpy(rng.randn(Lx, B * bd, V1).astype(np.float32))
        for sample_n in sorted({1, bd}):
            m = M()
            seq_h, slp_h = beam.assemble_done_beams(m, *(torch.from_numpy(a) for a in (parent, token, score, ended)), logp_rows,
                                                    B, bd, Lx, V1, sample_n, bd, {'length_penalty': pen})
            seq, lineage, length, p, _ = ref.finalize(parent, token, score, ended, sample_n, pen)
            assert np.array_equal(seq, seq_h.numpy())
            for b in range(B):
                for i in range(sample_n):
                    row = b * sample_n + i
                    db = m.done_beams[b][i]
                    assert length[row] == db['seq'].shape[0] and p[row] == db['p']
                    for t in range(length[row]):                 # the rows the host code gathers
                        assert torch.equal(slp_h[row, t], logp_rows[t, lineage[t, row]])
                    assert (lineage[length[row]:, row] == -1).all()


def test_new_entry_points_are_declared_exported_and_bound():
    from imagecaptioning.pytorch_amd import _lib
    names = ('capmi_updown_beam_search_train', 'capmi_beam_finalize', 'capmi_lineage_gather')
    src = open(os.path.join(ROOT, 'include', 'capmi.h')).read()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    for n in names:
        assert re.search(r'\bint\s+%s\s*\(' % n, src), n
        assert re.search(r' T %s\b' % n, out), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert 'typedef struct capmi_updown_beam_train' in src
    assert [f[0] for f in _lib.UpDownBeamTrain._fields_] == ['b', 'drop_xt', 'drop_out', 'h_drop']
    assert _lib.UpDownBeamTrain._fields_[0][1] is _lib.UpDownBeam


class _OnDevice(torch.Tensor):
    """A CPU tensor that claims to live on the device: carries a call past the device check, so that what is raised next is
    raised before anything is launched."""
    is_cuda = property(lambda self: True)


def _fake(*shape):
    return torch.zeros(*shape).as_subclass(_OnDevice)


FAMILIES = [('att2in2', {}), ('adaatt', dict(att_hid_size=16)), ('adaattmo', dict(att_hid_size=16)), ('transformer', dict(N_enc=1, N_dec=1, d_model=16, d_ff=32, num_att_heads=2, dropout=0.1)),
            ('aoa', dict(num_heads=2, num_layers=2))]


def _tiny_model(family, extra):
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    kw = dict(caption_model=family, input_encoding_size=16, rnn_size=16, att_hid_size=8, seq_length=5, max_length=5, vocab_size=20,
              fc_feat_size=12, att_feat_size=12, vocab={str(i): 'w%d' % i for i in range(1, 21)})
    kw.update(extra)
    opt = synthetic.updown_opt(**kw)
    return models.setup(opt)


@pytest.mark.parametrize('family,extra', FAMILIES)
def test_other_families_refuse_a_training_beam_search(family, extra):
    model = _tiny_model(family, extra)
    model.train()
    for method in ('greedy', 'beam_search'):
        with pytest.raises(NotImplementedError, match='train_beam_size'):
            model(_fake(2, 12), _fake(2, 3, 12), None, opt=dict(sample_method=method, beam_size=2, sample_n=2), mode='sample')


def test_ensemble_refuses_a_training_beam_search():
    from imagecaptioning.pytorch_amd.captioning.models.AttEnsemble import AttEnsemble
    e = AttEnsemble([_tiny_model('updown', {}), _tiny_model('newfc', {})])
    e.train()
    with pytest.raises(NotImplementedError, match='train_beam_size'):
        e(_fake(2, 12), _fake(2, 3, 12), None, opt=dict(beam_size=2, sample_n=2), mode='sample')


@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_unsupported_options_are_named(family):
    model = _tiny_model(family, {})
    model.train()
    base = dict(beam_size=2, sample_n=2)
    for name, o in (('group_size', dict(group_size=2, beam_size=4)), ('decoding_constraint', dict(decoding_constraint=1)),
                    ('remove_bad_endings', dict(remove_bad_endings=1)), ('temperature', dict(temperature=0.5)),
                    ('output_logsoftmax', dict(output_logsoftmax=0)), ('use_ppo', dict(use_ppo=1))):
        with pytest.raises(NotImplementedError, match=name):
            model(_fake(2, 12), _fake(2, 3, 12), None, opt=dict(base, **o), mode='sample')
    with pytest.raises(AssertionError, match='sample_n'):
        model(_fake(2, 12), _fake(2, 3, 12), None, opt=dict(beam_size=3, sample_n=2), mode='sample')


def test_loss_wrapper_refuses_ppo_with_a_training_beam_search():
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    model = _tiny_model('updown', {})
    opt = synthetic.updown_opt(structure_loss_type='new_self_critical', structure_loss_weight=1.0, use_ppo=1, train_sample_method='greedy',
                               train_beam_size=2, train_sample_n=2)
    lw = LossWrapper.__new__(LossWrapper)
    torch.nn.Module.__init__(lw)
    lw.opt, lw.model = opt, model
    with pytest.raises(NotImplementedError, match='train_beam_size'):
        lw(_fake(2, 12), _fake(2, 3, 12), None, None, None, None, None, False, True, False)
