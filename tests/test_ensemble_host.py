"""Test-time ensembles (AttEnsemble, capmi_ensemble_logprobs, tools/eval_ensemble.py) without a GPU: the mixture formula against
the reference's recorded ensemble, the C struct against its ctypes mirror, the argument checks, and the --ids parsing."""
import argparse
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, GOLDEN

Z = os.path.join(GOLDEN, 'ensemble_tiny.npz')
MEMBERS = {'ua': ('updown', 'att2in2'), 'uta': ('updown', 'transformer', 'aoa'), 'nu': ('newfc', 'updown')}   # make_ensemble.SETS
SETS = tuple(MEMBERS)


def mixture64(members, weights):
    """log( sum_i w_i softmax(x_i) / sum_i w_i ) in fp64 (AttEnsemble.py:45-53)"""
    w = torch.tensor(weights, dtype=torch.float64)
    w = w / w.sum()
    p = sum(wi * torch.softmax(torch.as_tensor(x, dtype=torch.float64), -1) for wi, x in zip(w, members))
    return p.log()


@pytest.mark.parametrize('tag', SETS)
def test_fp64_mixture_of_members_is_the_reference_ensemble(tag):
    z = np.load(Z)
    ref = torch.from_numpy(z[tag + '_tf_logp']).double()
    n = len([k for k in z.files if k.startswith(tag + '_tf_member')])
    members = [z['%s_tf_member%d' % (tag, i)] for i in range(n)]
    mix = mixture64(members, z[tag + '_weights'].tolist())
    # the ensemble's AttModel._forward stops at the first all-pad column (AttModel.py:158-159): from there on its rows are zero
    # (a Transformer member's own forward has no such break)
    zero = (ref == 0).all(-1)
    assert zero.any(), 'the fixture exercises the trailing all-pad break'
    assert zero[:, -1].all() and not zero[:, 0].any()
    assert (zero == zero[:1]).all(), 'the break is a column of the batch'
    u = np.load(os.path.join(GOLDEN, 'updown_tiny.npz'))
    labels, masks = torch.from_numpy(u['labels']), torch.from_numpy(u['masks']).double()
    N, T = ref.shape[:2]
    inp = labels[..., :-1].reshape(N, -1)
    live = ~zero
    if 'transformer' in MEMBERS[tag]:
        # the reference ensemble steps the Transformer through get_logprobs_state (causal mask only) while its own forward also
        # masks the pad tokens of the input (TransformerModel.py:324-328): the two differ only at positions whose input prefix
        # holds a pad, i.e. after the caption ended, where the loss mask is 0.  AttEnsemble uses the member's own forward.
        live &= torch.stack([(inp[:, 1:t + 1] != 0).all(1) for t in range(T)], 1)
    keep = ref[live].exp() > 1e-30
    assert float((mix[live][keep] - ref[live][keep]).abs().max()) < 1e-5
    # the LanguageModelCriterion of the mixture is the loss recorded next to it
    mix[zero] = 0
    tgt = labels[..., 1:].reshape(N, -1)[:, :T]
    m = masks[..., 1:].reshape(N, -1)[:, :T]
    loss = -(mix.gather(2, tgt.unsqueeze(2)).squeeze(2) * m).sum() / m.sum()
    assert abs(float(loss) - float(z[tag + '_tf_loss'])) < 1e-5


def test_ensemble_struct_matches_header():
    from imagecaptioning.pytorch_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'capmi.h')).read(), flags=re.S)
    body = re.search(r'typedef struct capmi_ensemble \{([^{}]*?)\} capmi_ensemble;', src, flags=re.S).group(1)
    names = []
    for stmt in body.split(';'):
        for part in stmt.strip().split(',') if stmt.strip() else []:
            names.append(re.findall(r'(\w+)\s*(?:\[\w+\])?$', part.strip())[0])
    assert names == [f[0] for f in _lib.Ensemble._fields_]
    assert re.search(r'#define CAPMI_ENSEMBLE_MAX %d\b' % _lib.ENSEMBLE_MAX, src)
    assert dict(_lib.Ensemble._fields_)['in']._length_ == _lib.ENSEMBLE_MAX
    assert dict(_lib.Ensemble._fields_)['w']._length_ == _lib.ENSEMBLE_MAX
    assert 'capmi_ensemble_logprobs' in _lib.SIGNATURES


def test_weights_are_checked_and_normalised():
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import CapmiError
    assert ops.ensemble_weights(None, 3) == pytest.approx([1 / 3] * 3)
    assert ops.ensemble_weights([1, 2, 1], 3) == pytest.approx([0.25, 0.5, 0.25])
    assert ops.ensemble_weights(torch.tensor([0.0, 3.0]), 2) == pytest.approx([0.0, 1.0])
    for bad, M in (([-0.1, 1.0], 2), ([0.0, 0.0], 2), ([float('nan'), 1.0], 2), ([float('inf'), 1.0], 2), ([1.0], 2),
                   ([1.0] * 9, 9), ([], 0)):
        with pytest.raises(CapmiError):
            ops.ensemble_weights(bad, M)


def test_ensemble_logprobs_rejects_bad_inputs_before_any_launch():
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import CapmiError
    x = torch.zeros(4, 31)
    with pytest.raises(CapmiError, match='>= 0'):
        ops.ensemble_logprobs([x, x], [-1.0, 2.0])
    with pytest.raises(CapmiError, match='positive sum'):
        ops.ensemble_logprobs([x, x], [0.0, 0.0])
    with pytest.raises(CapmiError, match='1..8'):
        ops.ensemble_logprobs([x] * 9)
    with pytest.raises(CapmiError, match='same shape'):
        ops.ensemble_logprobs([x, torch.zeros(4, 30)])
    with pytest.raises(CapmiError, match='float32'):
        ops.ensemble_logprobs([x, x.double()])
    with pytest.raises(CapmiError, match='device'):
        ops.ensemble_logprobs([x, x])              # CPU tensors: there is no CPU path


def _tiny(V=30, **kw):
    o = argparse.Namespace(caption_model='updown', vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1, drop_prob_lm=0.0,
                           seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=12, use_bn=0, logit_layers=1,
                           vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    vars(o).update(kw)
    return o


def test_att_ensemble_constructor_contract():
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    from imagecaptioning.pytorch_amd._lib import CapmiError
    a, b = models.setup(_tiny()), models.setup(_tiny(caption_model='att2in2', max_length=5))
    e = AttEnsemble([a, b], weights=[0.3, 0.7])
    # the reference's state-dict layout: models.{i}.* and the weights buffer
    keys = set(e.state_dict())
    assert 'weights' in keys and {'models.0.' + k for k in a.state_dict()} <= keys and {'models.1.' + k for k in b.state_dict()} <= keys
    assert e.weights.tolist() == pytest.approx([0.3, 0.7])
    assert AttEnsemble([a, b]).weights.tolist() == [1.0, 1.0]
    assert (e.vocab_size, e.seq_length, e.vocab, e.unk_idx) == (30, 8, a.vocab, None)
    assert e.bad_endings_ix == a.bad_endings_ix
    with pytest.raises(ValueError, match='vocabulary'):
        AttEnsemble([a, models.setup(_tiny(V=29))])
    with pytest.raises(CapmiError):
        AttEnsemble([a, b], weights=[-1.0, 1.0])
    with pytest.raises(CapmiError):
        AttEnsemble([a, b], weights=[0.0, 0.0])
    with pytest.raises(CapmiError):
        AttEnsemble([a] * 9)
    # evaluation only: a forward in train mode or with gradients raises, the closing model.train() of eval_split still works
    e.train()
    with pytest.raises(RuntimeError, match='evaluation only'):
        e(torch.zeros(1, 20), torch.zeros(1, 3, 20), torch.zeros(1, 5, dtype=torch.long))
    e.eval()
    with pytest.raises(RuntimeError, match='no_grad'):
        e(torch.zeros(1, 20), torch.zeros(1, 3, 20), None, opt={}, mode='sample')
    e.train()
    assert e.training and all(m.training for m in e.models)


def test_eval_ensemble_parses_ids_into_infos_and_model_paths(tmp_path):
    from imagecaptioning.pytorch_amd.tools import eval_ensemble as EE
    from imagecaptioning.pytorch_amd.captioning.utils import misc
    ids, weights, root, explicit = EE.parse_args(['--ids', 'a', 'b-best', '--weights', '0.3', '0.7', '--log_root', str(tmp_path),
                                                  '--beam_size', '3'])
    assert ids == ['a', 'b-best'] and weights == [0.3, 0.7] and root == str(tmp_path) and explicit == {'beam_size': 3}
    paths = EE.member_paths(ids, root)
    assert paths == [(os.path.join(root, 'log_a'), 'a', '', os.path.join(root, 'log_a', 'infos_a.pkl'),
                      os.path.join(root, 'log_a', 'model.pth')),
                     (os.path.join(root, 'log_b'), 'b', 'best', os.path.join(root, 'log_b', 'infos_b-best.pkl'),
                      os.path.join(root, 'log_b', 'model-best.pth'))]
    # the suffix-aware reader finds what misc.save_checkpoint(..., append='best') wrote; load_infos keeps its meaning
    os.makedirs(os.path.join(root, 'log_b'))
    with open(paths[1][3], 'wb') as f:
        pickle.dump({'opt': argparse.Namespace(caption_model='updown'), 'vocab': {'1': 'w1'}}, f)
    assert misc.load_infos_suffixed(paths[1][0], 'b', 'best')['vocab'] == {'1': 'w1'}
    assert misc.load_infos(paths[1][0], 'b') == {}
    with pytest.raises(FileNotFoundError):
        misc.load_infos_suffixed(os.path.join(root, 'log_a'), 'a')
    # eval options come from the command line, model and data options from the first member's infos
    opt = EE.build_opt({'opt': argparse.Namespace(caption_model='newfc', rnn_size=16, beam_size=7, batch_size=4)}, explicit)
    assert (opt.caption_model, opt.rnn_size, opt.beam_size, opt.batch_size) == ('newfc', 16, 3, 4)
