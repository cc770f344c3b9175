"""Discriminative decoding on the device (csrc/disc.hip, imagecaptioning/pytorch_amd/disc.py, opt['distractors'], tools/eval.py
--disc_lambda) against the float64 restatement tests/disc_ref64.py: the kernel at every shape and dispatch arm, the wrapping
stepper against plain steppers of the same family, the whole search against a float64 replay, and the command line.

What the kernel does with non-finite columns (pinned below): a column that is -inf under the target gives -inf; a column that is
-inf under every present distractor and finite under the target gives +inf in mode 'suppress' (no distractor can say the word) and
the target's log-probability in mode 'listener'.

Seeds of the search case: the region features are torch.randn(3, 6, 20) * 0.5 of the first seed 4100 + i, i = 0, 1, ..., whose
float64 replay separates the last kept from the first dropped candidate of every step and image, and the returned caption from
the best other finished one, by more than 1e-4; the choice reads the replay alone (plain steppers of the family, float64
arithmetic), never the code under test."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import disc_ref64 as R
from test_att_trace_host import tiny_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
TOL = 2e-5             # the bound tests/test_ensemble_gpu.py holds the mixture kernel to


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _present(B, D1):
    """image 0: every slot; image 1: no distractor; image 2: a hole in the middle (B = 1: the hole)"""
    p = torch.ones(B, D1, dtype=torch.uint8)
    hole = torch.tensor([1, 1, 0, 1, 0, 0, 1, 1][:D1] if D1 > 2 else [1] * D1, dtype=torch.uint8)
    if B == 1:
        p[0] = hole
    else:
        p[1, 1:] = 0
        p[2] = hole
    p[:, 0] = 1
    return p


def _strided(rows, V1, ld, seed, fill=float('nan')):
    """float32 [rows, V1] view of a [rows, ld] buffer whose padding holds `fill` (a kernel that reads it shows NaN)"""
    buf = torch.full((rows, ld), fill, dtype=torch.float32)
    buf[:, :V1] = torch.randn(rows, V1, generator=torch.Generator().manual_seed(seed)) * 3.0
    dev = buf.to(DEV)
    return dev[:, :V1], buf[:, :V1]


@pytest.mark.parametrize('D1', (1, 2, 8))
@pytest.mark.parametrize('V1', (1, 3, 31, 9488))
def test_kernel_against_the_restatement(V1, D1):
    """B in {1, 3}, cur in {1, 3}, ld_in / ld_out in {V1, V1 + 1} (rows of differing 16-byte phase: the scalar cut), both modes,
    lambda in {0, 0.5, 1}; masks with an image without distractors and one with a hole in the middle"""
    from imagecaptioning.pytorch_amd import ops
    worst = 0.0
    for B in (1, 3):
        for cur in (1, 3):
            present = _present(B, D1)
            for pad_in, pad_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
                x_dev, x = _strided(B * D1 * cur, V1, V1 + pad_in, 1000 * V1 + 100 * D1 + 10 * B + cur + pad_in)
                out = torch.full((B * cur, V1 + pad_out), 7.0, dtype=torch.float32, device=DEV)
                for mode in R.MODES:
                    for lam in (0.0, 0.5, 1.0):
                        got = ops.disc_combine(x_dev, present.to(DEV), lam, mode, B, D1, cur, out[:, :V1])
                        want = R.combine(x.reshape(B, D1, cur, V1), present, lam, mode).view(B * cur, V1)
                        err = float((got.double().cpu() - want).abs().max())
                        worst = max(worst, err)
                        assert err < TOL, (B, cur, pad_in, pad_out, mode, lam, err)
                        if lam == 1.0 or D1 == 1:
                            lsm = torch.log_softmax(x.reshape(B, D1, cur, V1)[:, 0].double(), -1).view(B * cur, V1)
                            assert float((got.double().cpu() - lsm).abs().max()) < TOL
                if pad_out:
                    assert (out[:, V1:] == 7.0).all()                        # nothing is written behind a row
    print('disc_combine V1 %d D1 %d: max abs error %.3g' % (V1, D1, worst))


def test_kernel_non_finite_columns():
    from imagecaptioning.pytorch_amd import ops
    B, D1, cur, V1 = 2, 3, 2, 37
    x = torch.randn(B * D1 * cur, V1, generator=torch.Generator().manual_seed(5)) * 2.0
    xv = x.reshape(B, D1, cur, V1)
    xv[:, 0, :, 4] = float('-inf')                   # the target cannot say word 4
    xv[:, 1:, :, 9] = float('-inf')                  # no distractor can say word 9
    xv[:, :, :, 11] = float('-inf')                  # nobody can say word 11
    xv[0, 2, 1, 20] = float('nan')                   # a NaN under one distractor of hypothesis (0, 1)
    present = torch.ones(B, D1, dtype=torch.uint8)
    for mode in R.MODES:
        got = ops.disc_combine(x.to(DEV), present.to(DEV), 0.5, mode, B, D1, cur).cpu().view(B, cur, V1)
        want = R.combine(xv, present, 0.5, mode)
        assert torch.isneginf(got[..., 4]).all() and torch.isneginf(got[..., 11]).all()
        clean = torch.ones(B, cur, dtype=torch.bool)
        clean[0, 1] = False
        if mode == 'suppress':
            assert (got[..., 9][clean] == float('inf')).all()
        else:
            lt = torch.log_softmax(xv[:, 0].double(), -1)
            assert float((got[..., 9].double() - lt[..., 9])[clean].abs().max()) < TOL
        other = [v for v in range(V1) if v not in (4, 11)]       # the NaN slot's sum is NaN: every column the target can say
        assert torch.isnan(got[0, 1, other]).all() and torch.isnan(want[0, 1, other]).all()
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin)
        assert float((got.double() - want)[fin].abs().max()) < TOL
        assert not torch.isnan(got[1]).any() and not torch.isnan(got[0, 0]).any()


@pytest.mark.parametrize('ld_pad', (0, 1))
def test_absent_slots_are_not_read(ld_pad):
    from imagecaptioning.pytorch_amd import ops
    B, D1, cur, V1 = 3, 8, 3, 1031
    present = _present(B, D1)
    x_dev, _ = _strided(B * D1 * cur, V1, V1 + ld_pad, 77, fill=0.0)
    absent = (present == 0).to(DEV).view(B, D1, 1, 1).expand(B, D1, cur, V1).reshape(B * D1 * cur, V1)
    zeros, nans = (torch.zeros(B * D1 * cur, V1 + ld_pad, device=DEV)[:, :V1] for _ in range(2))      # strided like x_dev
    zeros.copy_(torch.where(absent, torch.zeros_like(x_dev), x_dev))
    nans.copy_(torch.where(absent, torch.full_like(x_dev, float('nan')), x_dev))
    for mode in R.MODES:
        for lam in (0.0, 0.5):
            a = ops.disc_combine(zeros, present.to(DEV), lam, mode, B, D1, cur)
            b = ops.disc_combine(nans, present.to(DEV), lam, mode, B, D1, cur)
            assert torch.equal(a, b) and torch.isfinite(a).all()
    # lambda = 1: no slot behind the target is read at all
    every = torch.ones(B, D1, dtype=torch.uint8, device=DEV)
    poisoned = x_dev.clone().view(B, D1, cur, V1)
    poisoned[:, 1:] = float('nan')
    a = ops.disc_combine(poisoned.view(-1, V1), every, 1.0, 'suppress', B, D1, cur)
    assert torch.isfinite(a).all()


def test_invalid_arguments_and_empty_calls():
    from imagecaptioning.pytorch_amd import _lib
    from imagecaptioning.pytorch_amd._lib import lib, stream_ptr
    B, D1, cur, V1 = 2, 3, 2, 16
    x = torch.randn(B * D1 * cur, V1, device=DEV)
    p = torch.ones(B, D1, dtype=torch.uint8, device=DEV)
    out = torch.empty(B * cur, V1, device=DEV)

    def call(**kw):
        d = _lib.Disc()
        d.B, d.D1, d.cur, d.V1, d.ld_in, d.ld_out, d.mode = B, D1, cur, V1, V1, V1, 0
        setattr(d, 'lambda', 0.5)
        setattr(d, 'in', x.data_ptr())
        d.present, d.out = p.data_ptr(), out.data_ptr()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.capmi_disc_combine(C.byref(d), stream_ptr())

    assert call() == 0
    for bad in (dict(D1=0), dict(D1=9), dict(ld_in=V1 - 1), dict(ld_out=V1 - 1), dict(V1=0), dict(B=-1), dict(cur=-1), dict(mode=2),
                {'in': None}, dict(present=None), dict(out=None), {'lambda': -0.1}, {'lambda': 1.1}, {'lambda': float('nan')},
                {'lambda': float('inf')}, dict(out=x.data_ptr()), dict(out=x.data_ptr() + 4 * V1 * (B * D1 * cur - 1))):
        assert call(**bad) == _lib.EINVAL, bad
    assert lib.capmi_disc_combine(None, stream_ptr()) == _lib.EINVAL
    out.fill_(3.0)
    assert call(B=0) == 0 and call(cur=0) == 0 and (out == 3.0).all()                      # rows == 0: nothing launched


# ---------------------------------------------------------------------------------------------------------------------------
# the stepper
# ---------------------------------------------------------------------------------------------------------------------------
def _golden_family(name):
    from imagecaptioning.pytorch_amd.captioning import models
    z = np.load(os.path.join(GOLDEN, '%s_tiny.npz' % name))
    model = models.setup(tiny_opt(name, vocab_size=30, att_hid_size=12, seq_length=8, max_length=8,
                                  vocab={str(i): 'w%d' % i for i in range(1, 31)}))
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('P.')})
    return model.to(DEV).eval(), tuple(torch.from_numpy(z[k]).to(DEV) for k in ('fc', 'att', 'att_masks'))


def _family_and_feats(name):
    if name == 'transformer':
        from test_sbs_gpu import _family, _feats
        return _family('transformer'), _feats() + (None,)
    return _golden_family(name)


def _take(t, idx):
    return None if t is None else t[idx]


@pytest.mark.parametrize('name', ('updown', 'att2in2', 'transformer'))
def test_stepper_against_plain_steppers(name):
    """B = 3, D = 2 (one slot absent), bd = 3: step 0 from BOS, the fan-out, a step, a reorder with a non-identity parent, two more
    steps -- u against the restatement over the logits of plain steppers on the target's and on each distractor's features"""
    from imagecaptioning.pytorch_amd import disc
    model, (fc, att, masks) = _family_and_feats(name)
    B, bd, L, V1 = 3, 3, model.seq_length, model.vocab_size + 1
    d = torch.tensor([[1, 2], [2, -1], [1, 0]])
    req = disc.check_options(model, {'distractors': d, 'disc_lambda': 0.4, 'beam_size': bd, 'sample_n': 1}, B).on(torch.device(DEV, 0))
    with torch.no_grad():
        st = disc.make_stepper(model, req, fc, att, masks, L)(bd)
        assert (st.B, st.V1, st.cap) == (B, V1, bd)
        plain = [model._decode_stepper(_take(fc, req.slots[:, s].to(DEV)), att[req.slots[:, s].to(DEV)],
                                       _take(masks, req.slots[:, s].to(DEV)), L)(bd) for s in range(req.D1)]
        gen = torch.Generator().manual_seed(3)
        script = [('step', torch.zeros(B, dtype=torch.long), 1),
                  ('reorder', torch.zeros(B, bd, dtype=torch.int32), 1),
                  ('step', torch.randint(1, V1, (B * bd,), generator=gen), bd),
                  ('reorder', torch.tensor([[2, 0, 0], [1, 1, 0], [0, 2, 1]], dtype=torch.int32), bd),
                  ('step', torch.randint(1, V1, (B * bd,), generator=gen), bd),
                  ('step', torch.randint(0, V1, (B * bd,), generator=gen), bd)]
        t = 0
        for what, arg, cur in script:
            arg = arg.to(DEV)
            if what == 'reorder':
                st.reorder(arg, cur)
                for p in plain:
                    p.reorder(arg, cur)
                continue
            u = st.step(t, arg, cur)
            assert u.shape == (B * cur, V1)
            logits = torch.stack([p.step(t, arg, cur).clone().view(B, cur, V1) for p in plain], 1)        # [B, D1, cur, V1]
            want = R.combine(logits.cpu(), req.present, 0.4, req.mode).view(B * cur, V1)
            err = float((u.double().cpu() - want).abs().max())
            print('stepper', name, 't', t, 'max abs error %.3g' % err)
            assert err < TOL, (name, t, err)
            t += 1


# ---------------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------------
DISTRACTORS = torch.tensor([[1, 2], [2, -1], [1, 0]])


def _replay(model, fc, att, masks, distractors, lam, mode, bd):
    """float64 beam search over the restatement's rows; the decoder rows come from plain steppers of the family, one image's
    slots at a time, stepped from BOS along the prefix"""
    B, D = distractors.shape
    L, V1 = model.seq_length, model.vocab_size + 1
    own = torch.arange(B).unsqueeze(1)
    slots = torch.cat([own, torch.where(distractors >= 0, distractors, own.expand(B, D))], 1)
    present = torch.cat([torch.ones(B, 1, dtype=torch.uint8), (distractors >= 0).to(torch.uint8)], 1)
    cache = {}

    def decoder(k, prefix):
        if (k, prefix) not in cache:
            idx = slots[k].to(DEV)
            st = model._decode_stepper(_take(fc, idx), att[idx], _take(masks, idx), L)(1)
            for t, tok in enumerate((0,) + prefix):
                logits = st.step(t, torch.full((1 + D,), tok, dtype=torch.long, device=DEV), 1)
            u = R.combine(logits.cpu().view(1, 1 + D, 1, V1), present[k:k + 1], lam, mode)[0, 0]
            cache[k, prefix] = torch.log_softmax(u, 0)
        return cache[k, prefix]
    with torch.no_grad():
        return R.beam_search(decoder, B, V1, L, bd)


def _search_case():
    model, (fc, _, masks) = _golden_family('att2in2')
    for i in range(20):
        att = (torch.randn(3, 6, 20, generator=torch.Generator().manual_seed(4100 + i)) * 0.5).to(DEV)
        ref = _replay(model, fc, att, masks, DISTRACTORS, 0.3, 'suppress', 3)
        if float(ref['step_gap'].min()) > 1e-4 and float(ref['final_gap'].min()) > 1e-4:
            return model, fc, att, masks, ref, i
    raise AssertionError('no seed separates the candidates')


def test_beam_search_against_the_float64_replay():
    model, fc, att, masks, ref, i = _search_case()
    print('search case: seed index', i, 'step gap %.3g final gap %.3g' % (float(ref['step_gap'].min()), float(ref['final_gap'].min())))
    assert float(ref['step_gap'].min()) > 1e-4 and float(ref['final_gap'].min()) > 1e-4    # on the replay alone
    with torch.no_grad():
        seq, logp = model(fc, att, masks, opt={'beam_size': 3, 'sample_n': 1, 'distractors': DISTRACTORS, 'disc_lambda': 0.3},
                          mode='sample')
    assert seq.shape == (3, 8) and logp.shape == (3, 8, 31)
    assert torch.equal(seq.cpu(), ref['seq']), (seq.cpu(), ref['seq'])
    err = float((logp.double().cpu() - ref['logp']).abs().max())
    print('search: max abs seqLogprobs error %.3g' % err)
    assert err < 1e-4
    last = model.last_disc
    assert sorted(last) == ['distractors', 'lambda', 'mode'] and (last['lambda'], last['mode']) == (0.3, 'suppress')
    assert last['distractors'].is_cuda and torch.equal(last['distractors'].cpu(), DISTRACTORS)
    # the pragmatic caption differs from the plain one somewhere, and a call without the option clears last_disc
    with torch.no_grad():
        plain, _ = model(fc, att, masks, opt={'beam_size': 3, 'sample_n': 1}, mode='sample')
        assert model.last_disc is None
        # lambda = 1 is the plain beam search
        same, same_logp = model(fc, att, masks, opt={'beam_size': 3, 'sample_n': 1, 'distractors': DISTRACTORS, 'disc_lambda': 1.0},
                                mode='sample')
    assert torch.equal(same, plain) and model.last_disc['lambda'] == 1.0
    # distractors on the device are the same call
    with torch.no_grad():
        again, again_logp = model(fc, att, masks, opt={'beam_size': 3, 'sample_n': 1, 'distractors': DISTRACTORS.to(DEV),
                                                       'disc_lambda': 0.3}, mode='sample')
    assert torch.equal(again, seq) and torch.equal(again_logp, logp)


def test_identical_images_give_a_uniform_row():
    """target and distractor the same image, suppress, lambda = 0, D = 1: u = lt - ld = 0 in every column, a uniform distribution;
    ties go to the lower index, so every search ends its caption at once (token 0)"""
    model, (fc, att, masks) = _golden_family('att2in2')
    fc, att, masks = fc[:1].expand(3, -1).contiguous(), att[:1].expand(3, -1, -1).contiguous(), masks[:1].expand(3, -1).contiguous()
    ring = torch.tensor([[1], [2], [0]])
    for o in ({}, {'beam_size': 3, 'sample_n': 1}):
        with torch.no_grad():
            seq, logp = model(fc, att, masks, opt=dict(o, distractors=ring, disc_lambda=0.0), mode='sample')
        assert not seq.any(), (o, seq)
        assert float((logp[:, 0] + math.log(31)).abs().max()) < 1e-6


def test_every_search_takes_distractors():
    model, (fc, att, masks) = _golden_family('att2in2')
    L, V1 = 8, 31
    base = {'distractors': DISTRACTORS, 'disc_lambda': 0.5, 'disc_mode': 'listener'}
    with torch.no_grad():
        seq, logp = model(fc, att, masks, opt=dict(base), mode='sample')                                         # greedy
        assert seq.shape == (3, L) and logp.shape == (3, L, V1) and model.last_disc['mode'] == 'listener'
        mass = logp[:, 0].exp().sum(1)
        assert torch.allclose(mass, torch.ones_like(mass), atol=1e-4)                 # the pragmatic distribution is normalised
        torch.manual_seed(2)
        seq, logp = model(fc, att, masks, opt=dict(base, sample_method='sbs', sample_n=3), mode='sample')
        assert seq.shape == (9, L) and logp.shape == (9, L, V1) and model.last_sbs['phi'].shape == (3, 3)
        for img in seq.view(3, 3, L).cpu().tolist():
            assert len({tuple(r) for r in img}) == 3, img
        seq, logp = model(fc, att, masks, opt=dict(base, beam_size=2, constraints=[[[5]], [], [[7, 8], [9]]]), mode='sample')
        assert seq.shape == (3, L) and logp.shape == (3, L, V1)
        assert model.last_cbs['satisfied'].tolist() == [1, 0, 2] and model.last_disc is not None
        rows = seq.cpu().tolist()
        assert 5 in rows[0] and (7 in rows[2] or 8 in rows[2]) and 9 in rows[2]
        seq, _ = model(fc, att, masks, opt=dict(base, sample_method='sample', sample_n=2, decoding_constraint=1), mode='sample')
        assert seq.shape == (6, L)
        model(fc, att, masks, opt={}, mode='sample')
        assert model.last_disc is None and model.last_cbs is None and model.last_sbs is None


@pytest.mark.parametrize('name', ('newfc', 'adaatt', 'aoa'))
def test_other_families_decode_with_distractors(name):
    from test_sbs_gpu import _family, _feats, B_, L_
    model = _family(name)
    fc, att = _feats()
    with torch.no_grad():
        seq, logp = model(fc, att, None, opt={'beam_size': 2, 'sample_n': 1, 'distractors': torch.tensor([[1], [2], [-1]])}, mode='sample')
        plain, plain_logp = model(fc, att, None, opt={'beam_size': 2, 'sample_n': 1}, mode='sample')
    assert seq.shape == (B_, L_) and model.last_disc is None
    # the image without a distractor decodes as the plain search does
    assert torch.equal(seq[2], plain[2]) and float((logp[2] - plain_logp[2]).abs().max()) < 1e-4


def test_a_call_without_the_option_is_the_parent_commits_call():
    """tokens and log-probabilities of the tiny Att2in2 model, greedy and beam 3, bit for bit as the commit before this option
    returned them (tests/golden/disc_parent_att2in2.npz, recorded from that build on an MI355X)"""
    z = np.load(os.path.join(GOLDEN, 'disc_parent_att2in2.npz'))
    model, (fc, att, masks) = _golden_family('att2in2')
    with torch.no_grad():
        for key, o in (('greedy', {'sample_method': 'greedy'}), ('beam3', {'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1})):
            seq, logp = model(fc, att, masks, opt=o, mode='sample')
            assert np.array_equal(seq.cpu().numpy(), z[key + '_seq']), key
            assert np.array_equal(logp.cpu().numpy().view(np.uint32), z[key + '_logp'].view(np.uint32)), key
            assert model.last_disc is None


# ---------------------------------------------------------------------------------------------------------------------------
# tools/eval.py
# ---------------------------------------------------------------------------------------------------------------------------
def test_eval_entrypoint(tmp_path):
    from test_langeval_gpu import SMALL, _opts
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    out_dir = tmp_path / 'disc'
    _, preds = E.main(_opts(SMALL + ['--num_images', '10', '--split', 'val', '--disc_lambda', '0.5', '--disc_distractors', '2',
                                     '--self_retrieval', '1', '--retrieval_pool', '8', '--eval_results_dir', str(out_dir)]))
    assert sorted(os.listdir(out_dir)) == ['capmi_val_disc.json', 'capmi_val_ret.json'] and len(preds) == 10
    disc = json.load(open(out_dir / 'capmi_val_disc.json'))
    assert disc['settings'] == {'disc_lambda': 0.5, 'disc_distractors': 2, 'disc_mode': 'suppress', 'disc_pick': 'nearest', 'seed': 1234}
    assert len(disc['images']) == 10 and all(sorted(im) == ['distractors', 'image_id'] for im in disc['images'])
    ids = {p['image_id'] for p in preds}
    for p in preds:
        assert len(p['distractors']) <= 2 and p['image_id'] not in p['distractors']
        assert 'retrieval_rank' in p and 'retrieval_log_post' in p
    assert {im['image_id'] for im in disc['images']} == ids and any(len(p['distractors']) == 2 for p in preds)
    ret = json.load(open(out_dir / 'capmi_val_ret.json'))['overall']
    assert {'R@1', 'R@5', 'R@10', 'MRR', 'median_rank', 'mean_rank'} <= set(ret) and ret['captions'] == 10 and ret['pool_size'] == 8
