"""Knowledge distillation on the CPU: DistillCriterion's generic route against the float64 restatement (tests/distill_ref64.py), its
limits (lambda 0 = LanguageModelCriterion, teacher == student), the edge cases of the formula, the start-up refusals, the ctypes
struct against include/capmi.h and the LossWrapper / options wiring."""
import argparse
import os
import re

import pytest
import torch

from conftest import ROOT
from distill_ref64 import distill64

HEADER = os.path.join(ROOT, 'include', 'capmi.h')


def tiny_opt(**kw):
    V = 30
    o = argparse.Namespace(caption_model='updown', vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1,
                           drop_prob_lm=0.0, seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20,
                           att_hid_size=12, use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)},
                           label_smoothing=0, structure_loss_type=None, train_sample_method='sample', train_beam_size=1,
                           train_sample_n=2, use_ppo=0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def inputs(N=6, T=5, Tt=7, V1=11, ld=9, seed=0):
    """float64 student / teacher log-probs (the teacher longer than T), tokens and masks of pitch `ld` with zero positions
    mid-row and one fully masked sample"""
    g = torch.Generator().manual_seed(seed)
    ls = torch.log_softmax(2 * torch.randn(N, T, V1, generator=g, dtype=torch.float64), 2)
    lt = torch.log_softmax(2 * torch.randn(N, Tt, V1, generator=g, dtype=torch.float64), 2)
    tok = torch.randint(0, V1, (N, ld), generator=g)
    mask = (torch.rand(N, ld, generator=g) > 0.3).double()
    mask[:, 0] = 1
    mask[1, 2] = 0
    mask[3] = 0
    return ls, lt, tok, mask


def crit_of(lam, tau):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    return losses.DistillCriterion(lam, tau)


@pytest.mark.parametrize('red', ('mean', 'none'))
@pytest.mark.parametrize('lam,tau', [(0.0, 1.0), (0.3, 0.5), (0.3, 2.0), (1.0, 1.0), (1.0, 2.0)])
def test_generic_equals_ref64(lam, tau, red):
    ls, lt, tok, mask = inputs()
    u = torch.linspace(0.5, 1.5, ls.shape[0], dtype=torch.float64) if red == 'none' else 0.7
    ref = distill64(ls, lt, tok, mask, lam, tau, per_row=(red == 'none'), u=u)
    x = ls.clone().requires_grad_(True)
    o = crit_of(lam, tau)(x, lt, tok, mask, reduction=red)
    if red == 'none':
        live = mask[:, :5].sum(1) > 0
        assert torch.isnan(o['loss'][3]) and bool(torch.isfinite(o['loss'][live]).all())      # NaN in the masked sample only
        (o['loss'][live] * u[live]).sum().backward()
        assert float((o['loss'][live] - ref['loss'][live]).abs().max()) <= 1e-12
    else:
        (o['loss'] * u).backward()
        assert abs(float(o['loss'] - ref['loss'])) <= 1e-12
    assert abs(float(o['lm_loss'] - ref['lm_loss'])) <= 1e-12 and abs(float(o['kd_loss'] - ref['kd_loss'])) <= 1e-12
    assert float((x.grad - ref['grad']).abs().max()) <= 1e-12
    off = mask[:, :5] == 0
    assert torch.equal(x.grad[off], torch.zeros_like(x.grad[off]))


@pytest.mark.parametrize('red', ('mean', 'none'))
def test_lambda_zero_is_the_language_model_criterion(red):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    ls, lt, tok, mask = inputs()
    mask[3, 0] = 1
    x1, x2 = ls.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    a = crit_of(0.0, 2.0)(x1, lt, tok, mask, reduction=red)
    b = losses.LanguageModelCriterion()(x2, tok, mask, reduction=red)
    assert float((a['loss'] - b).abs().max()) <= 1e-14 and float((a['lm_loss'] - (b if red == 'mean' else a['lm_loss'])).abs()) <= 1e-14
    a['loss'].sum().backward()
    b.sum().backward()
    assert float((x1.grad - x2.grad).abs().max()) <= 1e-14


def test_teacher_equal_to_student_gives_zero():
    ls, _, tok, mask = inputs()
    x = ls.clone().requires_grad_(True)
    o = crit_of(1.0, 2.0)(x, ls.clone(), tok, mask)
    o['loss'].backward()
    assert abs(float(o['loss'])) <= 1e-15 and abs(float(o['kd_loss'])) <= 1e-15
    assert float(x.grad.abs().max()) <= 1e-15


def test_zero_probability_teacher_column_contributes_nothing():
    ls, lt, tok, mask = inputs()
    lt = lt[:, :5].clone()
    lt[:, :, 4] = -float('inf')
    lt = torch.log_softmax(lt, 2)
    x = ls.clone().requires_grad_(True)
    o = crit_of(0.6, 1.0)(x, lt, tok, mask)
    o['loss'].backward()
    assert bool(torch.isfinite(o['loss'])) and bool(torch.isfinite(x.grad).all())
    keep = [v for v in range(ls.shape[2]) if v != 4]
    # the same KL over the remaining columns alone: the student's mass on column 4 only enters through its normaliser
    lp_s = torch.log_softmax(ls, 2)[:, :, keep]
    kl = (lt[:, :, keep].exp() * (lt[:, :, keep] - lp_s)).sum(2)
    m = mask[:, :5]
    assert abs(float(o['kd_loss']) - float((kl * m).sum() / m.sum())) <= 1e-12
    ref = distill64(ls, lt, tok, mask, 0.6, 1.0)
    assert abs(float(o['loss'] - ref['loss'])) <= 1e-12


def test_token_outside_the_vocabulary_gives_nan():
    ls, lt, tok, mask = inputs()
    tok[0, 0] = ls.shape[2]
    o = crit_of(0.5, 1.0)(ls, lt, tok, mask)
    assert torch.isnan(o['loss']) and torch.isnan(o['lm_loss']) and bool(torch.isfinite(o['kd_loss']))


class _Fake(torch.nn.Module):
    def __init__(self, vocab_size, shift=0.0, steps=None):
        super().__init__()
        self.vocab_size, self.shift, self.steps = vocab_size, shift, steps
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, fc, att, seq, att_masks):
        T = self.steps or seq.shape[-1]
        g = torch.Generator().manual_seed(int(self.shift * 100))
        return torch.log_softmax(torch.randn(fc.shape[0], T, self.vocab_size + 1, generator=g, dtype=torch.float64), 2)


def test_refusals_and_vocabulary_mismatch():
    from imagecaptioning.pytorch_amd import _lib
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    student = _Fake(30)
    base = dict(distill_weight=0.5, distill_temperature=2.0, distill_from=['a', 'b'], distill_weights=[])
    for bad, word in ((dict(label_smoothing=0.1), 'label_smoothing'), (dict(scheduled_sampling_start=0), 'scheduled sampling'),
                      (dict(distill_from=[]), 'distill_from'),
                      (dict(distill_from=['m%d' % i for i in range(_lib.ENSEMBLE_MAX + 1)]), 'CAPMI_ENSEMBLE_MAX')):
        opt = tiny_opt(**{**base, **bad})
        with pytest.raises(NotImplementedError, match=word):
            losses.DistillTeacher(opt, student, members=[_Fake(30)] * len(opt.distill_from))
        with pytest.raises(NotImplementedError, match=word):          # LossWrapper refuses before it loads anything
            LossWrapper(student, opt)
    with pytest.raises(ValueError, match="'b'"):
        losses.DistillTeacher(tiny_opt(**base), student, members=[_Fake(30), _Fake(31)])
    with pytest.raises(ValueError):
        losses.DistillTeacher(tiny_opt(**{**base, 'distill_weights': [1.0]}), student, members=[_Fake(30), _Fake(30)])


def test_teacher_mixture_and_freezing_on_fake_members():
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    student = _Fake(30)
    members = [_Fake(30, 0.01), _Fake(30, 0.02, steps=7)]
    t = losses.DistillTeacher(tiny_opt(distill_weight=0.5, distill_from=['a', 'b'], distill_weights=[1.0, 3.0]), student, members=members)
    assert t.weights == [0.25, 0.75]
    assert all(not p.requires_grad for m in members for p in m.parameters()) and all(not m.training for m in members)
    fc, seq = torch.zeros(4, 3), torch.zeros(4, 5, dtype=torch.long)
    got = t(fc, None, seq, None, 5)
    l1, l2 = members[0](fc, None, seq, None), members[1](fc, None, seq, None)[:, :5]
    want = torch.log(0.25 * l1.exp() + 0.75 * l2.exp())
    assert got.shape == (4, 5, 31) and float((got - want).abs().max()) <= 1e-12
    one = losses.DistillTeacher(tiny_opt(distill_weight=0.5, distill_from=['b']), student, members=members[1:])
    assert one(fc, None, seq, None, 5).shape == (4, 7, 31)              # a single member is handed on as it is; the criterion cuts
    assert not isinstance(t, torch.nn.Module)


def test_struct_layout_matches_header():
    """field order of _lib.Distill == field order of capmi_distill (parsed as tests/test_abi.py parses the header)"""
    from imagecaptioning.pytorch_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct (?:capmi_distill )?\{([^{}]*?)\} capmi_distill;', src, flags=re.S).group(1)
    names = []
    for stmt in body.split(';'):
        stmt = stmt.strip()
        if not stmt:
            continue
        for part in stmt.split(','):
            names.append(re.findall(r'(\w+)\s*(?:\[\w+\])?$', part.strip())[0])
    assert names == [f[0] for f in _lib.Distill._fields_]
    assert 'capmi_distill_loss_fwd' in _lib.SIGNATURES and 'capmi_distill_loss_bwd' in _lib.SIGNATURES
    import ctypes as C
    assert C.sizeof(_lib.Distill) == 10 * 4 + 2 * 4 + 10 * 8


def test_default_options_keep_the_old_criterion():
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    d = opts.DEFAULTS
    assert (d['distill_from'], d['distill_weights'], d['distill_weight'], d['distill_temperature']) == ([], [], 0.0, 1.0)
    o = opts.parse_opt([])
    assert o.distill_from == [] and o.distill_weight == 0.0 and o.distill_from is not d['distill_from']
    o = opts.parse_opt(['--distill_from', 'A', 'B-best', '--distill_weight', '0.7', '--distill_temperature', '2', '--distill_weights',
                        '1', '3'])
    assert (o.distill_from, o.distill_weight, o.distill_temperature, o.distill_weights) == (['A', 'B-best'], 0.7, 2.0, [1.0, 3.0])
    lw = LossWrapper(_Fake(30), tiny_opt())
    assert type(lw.crit) is losses.LanguageModelCriterion and lw.distill_crit is None and lw.distill_teacher is None
    lw = LossWrapper(_Fake(30), opts.parse_opt([]))
    assert type(lw.crit) is losses.LanguageModelCriterion and lw.distill_crit is None
    assert not any('distill' in k or 'teacher' in k for k in lw.state_dict())


def test_loss_wrapper_xe_branch_uses_the_distillation_criterion(monkeypatch):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    student = _Fake(30, 0.05)
    members = [_Fake(30, 0.01), _Fake(30, 0.02)]
    monkeypatch.setattr(losses.DistillTeacher, '_load', lambda self, opt, model: members)
    lw = LossWrapper(student, tiny_opt(distill_weight=0.4, distill_temperature=2.0, distill_from=['a', 'b']))
    assert set(k for k, _ in lw.named_parameters()) == {'model.w'}        # the teachers are no parameters of the wrapper
    fc = torch.zeros(4, 3)
    labels = torch.randint(1, 31, (4, 7))
    masks = torch.ones(4, 7, dtype=torch.float64)
    out = lw(fc, None, labels, masks, None, None, None, False, False, False)
    ls = student(fc, None, labels[:, :-1], None)
    lt = lw.distill_teacher(fc, None, labels[:, :-1], None, 6)
    ref = distill64(ls, lt, labels[:, 1:], masks[:, 1:], 0.4, 2.0)
    for k in ('loss', 'lm_loss', 'kd_loss'):
        assert abs(float(out[k] - ref[k])) <= 1e-12, k
    rows = lw(fc, None, labels, masks, None, None, None, False, False, True)['loss']
    assert rows.shape == (4,) and abs(float(rows.mean() - ref['loss'])) <= 1e-12      # (equal mask sums: the mean of the rows)
