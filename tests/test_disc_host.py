"""Discriminative decoding (opt['distractors']; imagecaptioning/pytorch_amd/disc.py, csrc/disc.hip) without a GPU: the float64
restatement tests/disc_ref64.py pinned by hand-computed values, the options, every refusal, the slot tables, the pickers of the
command line, and the bindings."""
import math
import os
import re

import pytest
import torch

from conftest import ROOT

import disc_ref64 as R
from test_att_trace_host import tiny_opt

FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')


def _model(name):
    from imagecaptioning.pytorch_amd.captioning import models
    if name == 'ensemble':
        return models.AttEnsemble([models.setup(tiny_opt('updown')), models.setup(tiny_opt('att2in2'))])
    return models.setup(tiny_opt(name))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement, by hand: V1 = 3, D = 1.  Target probabilities (1/2, 1/4, 1/4), distractor (1/4, 1/4, 1/2).
# ---------------------------------------------------------------------------------------------------------------------------
PT, PD = (0.5, 0.25, 0.25), (0.25, 0.25, 0.5)


def _hand_logits(shift=(0.0, 0.0)):
    """[1, 2, 1, 3] logits with those softmaxes (a shift per slot must not matter: every slot is normalised)"""
    return torch.tensor([[[[math.log(p) + shift[0] for p in PT]], [[math.log(p) + shift[1] for p in PD]]]], dtype=torch.float64)


@pytest.mark.parametrize('shift', ((0.0, 0.0), (3.0, -7.5)))
def test_restatement_by_hand(shift):
    x, both = _hand_logits(shift), torch.tensor([[1, 1]])
    lt = [math.log(p) for p in PT]
    # suppress, lambda = 0.5: log pt - 0.5 log pd
    want = [math.log(a) - 0.5 * math.log(b) for a, b in zip(PT, PD)]
    assert torch.allclose(R.combine(x, both, 0.5, 'suppress')[0, 0], torch.tensor(want, dtype=torch.float64), atol=1e-12)
    # suppress, lambda = 0: log (pt / pd) = log 2, 0, -log 2
    assert torch.allclose(R.combine(x, both, 0.0, 'suppress')[0, 0], torch.tensor([math.log(2), 0.0, -math.log(2)], dtype=torch.float64),
                          atol=1e-12)
    # listener, lambda = 0.5: log pt + 0.5 log (pt / (pt + pd)); posteriors 2/3, 1/2, 1/3
    want = [math.log(a) + 0.5 * math.log(a / (a + b)) for a, b in zip(PT, PD)]
    assert torch.allclose(R.combine(x, both, 0.5, 'listener')[0, 0], torch.tensor(want, dtype=torch.float64), atol=1e-12)
    want = [math.log(0.5 * 2 / 3), math.log(0.25 / 2), math.log(0.25 / 3)]
    assert torch.allclose(R.combine(x, both, 0.0, 'listener')[0, 0], torch.tensor(want, dtype=torch.float64), atol=1e-12)
    for mode in R.MODES:
        # lambda = 1 and an absent slot: the target's log-softmax
        assert torch.allclose(R.combine(x, both, 1.0, mode)[0, 0], torch.tensor(lt, dtype=torch.float64), atol=1e-12)
        assert torch.allclose(R.combine(x, torch.tensor([[1, 0]]), 0.3, mode)[0, 0], torch.tensor(lt, dtype=torch.float64), atol=1e-12)


def test_restatement_mean_of_two_distractors_and_non_finite_columns():
    x = torch.cat([_hand_logits(), _hand_logits()[:, 1:].flip(-1)], 1)                     # second distractor (1/2, 1/4, 1/4)
    mean = [(a + b) / 2 for a, b in zip(PD, PD[::-1])]
    want = [math.log(a) - 0.7 * math.log(m) for a, m in zip(PT, mean)]
    assert torch.allclose(R.combine(x, torch.tensor([[1, 1, 1]]), 0.3, 'suppress')[0, 0], torch.tensor(want, dtype=torch.float64),
                          atol=1e-12)
    # a hole in the middle: the second distractor alone
    want = [math.log(a) - 0.7 * math.log(b) for a, b in zip(PT, PD[::-1])]
    assert torch.allclose(R.combine(x, torch.tensor([[1, 0, 1]]), 0.3, 'suppress')[0, 0], torch.tensor(want, dtype=torch.float64),
                          atol=1e-12)
    y = _hand_logits()
    y[0, 0, 0, 2] = float('-inf')                                                          # the target cannot say word 2
    y[0, 1, 0, 0] = float('-inf')                                                          # the distractor cannot say word 0
    u = R.combine(y, torch.tensor([[1, 1]]), 0.5, 'suppress')[0, 0]
    assert u[2] == float('-inf') and u[0] == float('inf') and torch.isfinite(u[1])
    u = R.combine(y, torch.tensor([[1, 1]]), 0.5, 'listener')[0, 0]
    assert u[2] == float('-inf') and torch.isfinite(u[:2]).all()
    assert abs(float(u[0]) - math.log(2 / 3)) < 1e-12                                      # the listener is sure: u = lt


def test_replay_beam_search_finds_the_best_of_a_small_tree():
    """V1 = 3, L = 3, bd = 9 keeps every candidate of every step: the replay must return the best sequence of all"""
    import itertools
    gen = torch.Generator().manual_seed(4)
    table = {}
    for n in range(3):
        for prefix in itertools.product(range(3), repeat=n):
            table[prefix] = torch.log_softmax(torch.randn(3, generator=gen, dtype=torch.float64) * 1.5, 0)
    out = R.beam_search(lambda k, prefix: table[prefix], 1, 3, 3, 9)
    best = None
    for n in range(1, 4):
        for seq in itertools.product(range(3), repeat=n):
            if 0 in seq[:-1] or (seq[-1] != 0 and n < 3):
                continue
            s = sum(float(table[seq[:i]][v]) for i, v in enumerate(seq))
            if best is None or s > best[0]:
                best = (s, seq)
    n = int(out['length'][0])
    assert tuple(out['seq'][0, :n].tolist()) == best[1] and abs(float(out['score'][0]) - best[0]) < 1e-12
    assert abs(float(out['logp'][0].gather(1, out['seq'][0].unsqueeze(1))[:n].sum()) - best[0]) < 1e-12
    assert not out['logp'][0, n:].any()


# ---------------------------------------------------------------------------------------------------------------------------
# options, refusals, tables
# ---------------------------------------------------------------------------------------------------------------------------
def test_option_defaults_and_parsing():
    from imagecaptioning.pytorch_amd import disc
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    assert opts.DEFAULTS['disc_lambda'] < 0 and opts.DEFAULTS['disc_distractors'] == 1
    assert opts.DEFAULTS['disc_mode'] == 'suppress' and opts.DEFAULTS['disc_pick'] == 'nearest'
    o = opts.parse_opt(['--disc_lambda', '0.25', '--disc_distractors', '3', '--disc_mode', 'listener', '--disc_pick', 'random'])
    assert (o.disc_lambda, o.disc_distractors, o.disc_mode, o.disc_pick) == (0.25, 3, 'listener', 'random')
    assert opts.parse_opt([]).disc_lambda < 0
    assert not disc.wanted(None) and not disc.wanted({}) and not disc.wanted({'distractors': None, 'disc_lambda': 0.5})
    assert disc.wanted({'distractors': torch.zeros(1, 1, dtype=torch.long)})
    assert disc.D_MAX == 7 and disc.MODES == ('suppress', 'listener')
    model = _model('att2in2').eval()
    req = disc.check_options(model, {'distractors': torch.tensor([[1], [0]])}, 2)
    assert (req.lam, req.mode, req.B, req.D, req.D1, req.cbs) == (0.5, 'suppress', 2, 1, 2, None)
    req = disc.check_options(model, {'distractors': torch.tensor([[1], [0]], dtype=torch.int32), 'disc_lambda': 0, 'disc_mode': 'listener'}, 2)
    assert (req.lam, req.mode) == (0.0, 'listener')


def test_tools_eval_settings():
    import argparse
    from imagecaptioning.pytorch_amd.tools import eval as ev
    assert ev.Distractors.load(argparse.Namespace(disc_lambda=-1.0)) is None and ev.Distractors.load(argparse.Namespace()) is None
    d = ev.Distractors.load(argparse.Namespace(disc_lambda=0.5, disc_distractors=2, disc_mode='listener', disc_pick='random', seed=7))
    assert d.settings() == {'disc_lambda': 0.5, 'disc_distractors': 2, 'disc_mode': 'listener', 'disc_pick': 'random', 'seed': 7}
    infos = [{'id': 100 + i} for i in range(4)]
    kw = d.for_batch(torch.randn(4, 3, 5), None, infos, 3)
    assert sorted(kw) == ['disc_lambda', 'disc_mode', 'distractors'] and kw['distractors'].shape == (4, 2)
    assert sorted(d.rows) == [100, 101, 102]                                               # the image past the cut is not noted
    assert all(len(v) == 2 and k not in v and set(v) <= {100, 101, 102, 103} for k, v in d.rows.items())
    for bad in (dict(lam=1.5), dict(lam=0.5, D=0), dict(lam=0.5, D=8), dict(lam=0.5, mode='x'), dict(lam=0.5, pick='x')):
        with pytest.raises(ValueError):
            ev.Distractors(**bad)


def _call(model, opt, B=3):
    fc, att = torch.randn(B, 20), torch.randn(B, 5, 20)                  # CPU tensors: a refusal must come before the device check
    return model(fc, att, None, opt=opt, mode='sample')


def _ring(B=3, D=1):
    return torch.stack([(torch.arange(B) + d + 1) % B for d in range(D)], 1)


@pytest.mark.parametrize('name', FAMILIES)
def test_refusals_come_before_any_device_work(name):
    model = _model(name).eval()
    ok = {'distractors': _ring(), 'disc_lambda': 0.5}
    for bad, exc, word in (
            (dict(ok, output_logsoftmax=0), NotImplementedError, 'output_logsoftmax'),
            (dict(ok, return_attention=1), NotImplementedError, 'return_attention'),
            (dict(ok, distractors=torch.tensor([[1], [2], [2]])), ValueError, 'own distractor'),
            (dict(ok, distractors=torch.tensor([[1], [2], [3]])), ValueError, 'indices lie in'),
            (dict(ok, distractors=torch.tensor([[1], [2], [-2]])), ValueError, 'indices lie in'),
            (dict(ok, distractors=_ring(3, 1)[:2]), ValueError, 'the batch holds 3'),
            (dict(ok, distractors=torch.zeros(3, 8, dtype=torch.long)), ValueError, '1 <= D <= 7'),
            (dict(ok, distractors=torch.zeros(3, 0, dtype=torch.long)), ValueError, '1 <= D <= 7'),
            (dict(ok, distractors=_ring().float()), ValueError, 'integer tensor'),
            (dict(ok, distractors=[[1], [2], [0]]), ValueError, 'integer tensor'),
            (dict(ok, disc_lambda=1.5), ValueError, 'disc_lambda'),
            (dict(ok, disc_lambda=-0.1), ValueError, 'disc_lambda'),
            (dict(ok, disc_lambda=float('nan')), ValueError, 'disc_lambda'),
            (dict(ok, disc_mode='speaker'), ValueError, 'disc_mode'),
            (dict(ok, sample_method='sbs', sample_n=17), ValueError, 'sample_n'),
            (dict(ok, constraints=[[], [], []], sample_n=2), NotImplementedError, 'sample_n = 1')):
        with pytest.raises(exc, match=re.escape(word)):
            _call(model, bad)
        assert model.last_disc is None
    model.train()
    with pytest.raises(NotImplementedError, match='test-time option'):
        _call(model, dict(ok))
    with pytest.raises(NotImplementedError, match='train_beam_size > 1'):
        _call(model, dict(ok, beam_size=3, sample_n=1))
    model.eval()
    # a well-formed call gets as far as the device check (there is no CPU path), with the request's refusals behind it
    from imagecaptioning.pytorch_amd._lib import CapmiError
    with pytest.raises(CapmiError, match='HIP device'):
        _call(model, dict(ok))


def test_models_without_a_single_step_decoder_are_refused():
    from imagecaptioning.pytorch_amd import disc
    from imagecaptioning.pytorch_amd.captioning.models.CaptionModel import CaptionModel
    ens = _model('ensemble').eval()
    with pytest.raises(NotImplementedError, match='decode the members one by one'):
        _call(ens, {'distractors': _ring()})

    class Bare(CaptionModel):
        vocab_size, seq_length = 12, 6
    with pytest.raises(NotImplementedError, match='no single-step decoder'):
        disc.check_options(Bare().eval(), {'distractors': _ring()}, 3)
    assert CaptionModel.last_disc is None and _model('updown').last_disc is None


def test_row_bound_names_both_numbers():
    from imagecaptioning.pytorch_amd import disc, score
    model = _model('att2in2').eval()
    limit = score.default_rows(model.vocab_size + 1, model.rnn_size)
    B = limit // (8 * 4) + 1                                                               # B * (1 + 7) * 4 rows: just above
    d = torch.full((B, 7), -1, dtype=torch.long)
    rows = B * 8 * 4
    with pytest.raises(ValueError, match='%d rows.*%d' % (rows, limit)):
        disc.check_options(model, {'distractors': d, 'sample_method': 'sbs', 'sample_n': 4}, B)
    with pytest.raises(ValueError, match='%d rows.*%d' % (rows, limit)):
        disc.check_options(model, {'distractors': d, 'beam_size': 4, 'sample_n': 1}, B)
    with pytest.raises(ValueError, match='%d rows.*%d' % (rows, limit)):                   # 2 constraints: 4 states of one slot
        disc.check_options(model, {'distractors': d, 'beam_size': 1, 'constraints': [[[1], [2]]] + [[]] * (B - 1)}, B)
    assert disc.check_options(model, {'distractors': d[:B - 1], 'beam_size': 4, 'sample_n': 1}, B - 1).B == B - 1
    assert disc.rows_per_image({}) == 1 and disc.rows_per_image({'sample_n': 5, 'sample_method': 'sample'}) == 5
    assert disc.rows_per_image({'beam_size': 6, 'group_size': 3}) == 2 and disc.rows_per_image({'group_size': 3}) == 3


def test_slots_and_present():
    from imagecaptioning.pytorch_amd import disc
    model = _model('updown').eval()
    d = torch.tensor([[1, 2, 3], [-1, -1, -1], [0, -1, 3], [-1, 2, -1]])
    req = disc.check_options(model, {'distractors': d, 'disc_lambda': 0.25}, 4)
    assert req.slots.dtype == torch.long and req.present.dtype == torch.uint8
    assert req.slots.tolist() == [[0, 1, 2, 3], [1, 1, 1, 1], [2, 0, 2, 3], [3, 3, 2, 3]]    # an absent slot steps the image itself
    assert req.present.tolist() == [[1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 0, 1], [1, 0, 1, 0]]
    assert torch.equal(req.distractors, d) and req.device is None
    with pytest.raises(ValueError, match='Request.on'):
        disc.DiscStepper(None, req, 1)


def test_pickers():
    from imagecaptioning.pytorch_amd import disc
    gen = torch.Generator().manual_seed(2)
    att = torch.randn(6, 4, 8, generator=gen)
    att[3] = att[0] * 2.0 + 0.01 * torch.randn(4, 8, generator=gen)                         # image 3 looks like image 0
    masks = torch.ones(6, 4)
    masks[1, 2:] = 0
    near = disc.pick_nearest(att, masks, 2)
    assert near.shape == (6, 2) and near.dtype == torch.long
    assert near[0, 0] == 3 and near[3, 0] == 0
    for b in range(6):
        assert b not in near[b].tolist() and len(set(near[b].tolist())) == 2
    # the padded regions of image 1 do not count
    att2 = att.clone()
    att2[1, 2:] = 1e3
    assert torch.equal(disc.pick_nearest(att2, masks, 2), near)
    p = disc.pooled_regions(att, masks)
    assert torch.allclose(p[1], att[1, :2].mean(0)) and torch.allclose(p[0], att[0].mean(0))
    assert torch.allclose(disc.pooled_regions(att), att.mean(1))
    # fewer than D + 1 images: -1 pads
    assert disc.pick_nearest(att[:2], None, 3).tolist() == [[1, -1, -1], [0, -1, -1]]
    assert disc.pick_nearest(att[:1], None, 2).tolist() == [[-1, -1]]
    a = disc.pick_random(6, 3, torch.Generator().manual_seed(9))
    b = disc.pick_random(6, 3, torch.Generator().manual_seed(9))
    c = disc.pick_random(6, 3, torch.Generator().manual_seed(10))
    assert torch.equal(a, b) and not torch.equal(a, c)
    for k in range(6):
        assert k not in a[k].tolist() and len(set(a[k].tolist())) == 3 and 0 <= int(a[k].min()) and int(a[k].max()) < 6
    assert disc.pick_random(2, 3, torch.Generator().manual_seed(1)).tolist() == [[1, -1, -1], [0, -1, -1]]
    assert disc.pick_random(1, 2).tolist() == [[-1, -1]]


# ---------------------------------------------------------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_constants_match_the_header():
    from imagecaptioning.pytorch_amd import _lib, disc
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

    assert fields('capmi_disc') == [f[0] for f in _lib.Disc._fields_]
    assert fields('capmi_disc') == ['B', 'D1', 'cur', 'V1', 'ld_in', 'ld_out', 'mode', 'lambda', 'in', 'present', 'out']
    assert int(re.search(r'#define CAPMI_DISC_MAX (\d+)', src).group(1)) == _lib.DISC_MAX == disc.D_MAX + 1 == 8
    assert len(_lib.SIGNATURES['capmi_disc_combine']) == 2
    assert (_lib.DISC_SUPPRESS, _lib.DISC_LISTENER) == (0, 1)


def test_ops_argument_checks_come_before_the_launch():
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import CapmiError
    x, p = torch.zeros(4, 5), torch.ones(2, 2, dtype=torch.uint8)
    for args in ((x, p, 0.5, 'speaker', 2, 2, 1), (x, p, 0.5, 'suppress', 2, 9, 1), (x, p, 1.5, 'suppress', 2, 2, 1),
                 (x, p, float('nan'), 'suppress', 2, 2, 1), (x, p, 0.5, 'suppress', 2, 2, 1)):          # the last: CPU tensors
        with pytest.raises(CapmiError):
            ops.disc_combine(*args)
