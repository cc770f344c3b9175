"""Per-word region attention on the device (opt['return_attention'], csrc/att_trace.hip) against the reference fixture
(tests/golden/att_trace_tiny.npz: weights recomputed in float64 from the scores hooked off the reference's alpha_net), against torch
restatements of the two copy kernels bit for bit, against forced replays of beam-search results, and against the float64 replay of
the grounding kernel (tests/att_trace_ref64.py).

Bounds: 5e-5 on weights is the bound DESIGN section 2 sets for decode-option values (the trace is the same arithmetic); 1e-5 on the
sum of a kept row (K <= 7 float32 weights of a renormalised softmax: a few ulp of 1); the grounding numbers are compared with the
float64 replay of the device's OWN att, with boxes in [0, 1], so their error is float32 rounding of at most 7 products (~1e-6).
"""
import argparse
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import att_trace_ref64 as R64

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
Z = os.path.join(GOLDEN, 'att_trace_tiny.npz')
FAMILIES = ('updown', 'att2in2', 'adaatt', 'adaattmo')
CASES = (('n1', True, 1), ('n2', True, 2), ('nomask', False, 1))
TOL = 5e-5
_cache = {}


def fixture():
    if 'z' not in _cache:
        z = np.load(Z)
        _cache['z'] = {k: z[k] for k in z.files}
    return _cache['z']


def golden_model(name):
    from imagecaptioning.pytorch_amd.captioning import models
    z = fixture()
    V = 12
    opt = argparse.Namespace(caption_model=name, vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1, drop_prob_lm=0.0,
                             seq_length=6, max_length=6, fc_feat_size=20, att_feat_size=20, att_hid_size=16, use_bn=0, logit_layers=1,
                             vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    model = models.setup(opt)
    pre = name + '.P.'
    model.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in z.items() if k.startswith(pre)})
    return model.to(DEV).eval()


def feeds(name, masked=True):
    z = fixture()
    t = lambda k: torch.from_numpy(z['%s.%s' % (name, k)]).to(DEV)      # noqa: E731
    return t('fc'), t('att'), (t('att_masks') if masked else None), (t('boxes') / 100.0).contiguous()


def sample(model, fc, att, masks, **opt):
    with torch.no_grad():
        return model(fc, att, masks, opt=opt, mode='sample')


def check_structure(la, seq, K, col0):
    """exact zeros where nothing was attended, unit rows elsewhere, top = -1 exactly on the zeroed steps"""
    att = la['att']
    kept = torch.from_numpy(R64.shifted_mask(seq.cpu().numpy())).to(att.device)
    assert not att[~kept].any() and not att[:, :, K + col0:].any()
    s = att.double().sum(-1)[kept]
    print('row sums: max |sum - 1| = %.3g' % float((s - 1).abs().max()))
    assert float((s - 1).abs().max()) <= 1e-5
    assert torch.equal(la['top'] < 0, ~kept) and not la['top_w'][~kept].any() and not la['entropy'][~kept].any()
    return kept


def check_ground(la, n, boxes, col0):
    att64 = la['att'].double().cpu().numpy()
    want = R64.ground(att64, None if boxes is None else boxes.cpu().numpy(), n, col0)
    assert np.array_equal(la['top'].cpu().numpy(), want['top'])
    for k in ('top_w', 'entropy') + (('box',) if boxes is not None else ()):
        err = float(np.abs(la[k].double().cpu().numpy() - want[k]).max())
        print('%s: max error against the float64 replay %.3g' % (k, err))
        assert err <= TOL, k


@pytest.mark.parametrize('case', [c[0] for c in CASES])
@pytest.mark.parametrize('name', FAMILIES)
def test_greedy_trace_is_the_reference_attention(name, case):
    z = fixture()
    _, masked, n = next(c for c in CASES if c[0] == case)
    model = golden_model(name)
    fc, att, masks, boxes = feeds(name, masked)
    col0 = int(name.startswith('adaatt'))
    seq, _ = sample(model, fc, att, masks, sample_method='greedy', beam_size=1, sample_n=n, return_attention=1, boxes=boxes)
    la = model.last_attention
    assert sorted(la) == ['att', 'box', 'entropy', 'top', 'top_w']
    assert np.array_equal(seq.cpu().numpy(), z['%s.%s.seq' % (name, case)])                 # tokens: exact
    want = z['%s.%s.trace' % (name, case)]
    got = la['att'].double().cpu().numpy()
    assert got.shape == want.shape == (3 * n, 6, 6 + col0)
    err = float(np.abs(got - want).max())
    print('%s %s: max |att - reference| = %.3g' % (name, case, err))
    assert err <= TOL
    K = 5 if masked else 6
    kept = check_structure(la, seq, K, col0).cpu().numpy()
    if col0:
        # the sentinel sits where AdaAtt_attention concatenates it: column 0, in front of the regions
        assert (want[..., 0][kept] > 0).all() and float(np.abs(got[..., 0] - want[..., 0]).max()) <= TOL
    if masked:
        for r in range(3 * n):
            assert not got[r, :, int(z[name + '.att_masks'][r // n].sum()) + col0:].any()
    ref = R64.ground(want)
    assert np.array_equal(la['top'].cpu().numpy()[kept], ref['top'][kept])                  # the fixture's gaps exceed 1e-4
    check_ground(la, n, boxes, col0)
    assert model._trace_req is None


@pytest.mark.parametrize('name', FAMILIES)
def test_rollout_trace_is_the_rollouts_own_alpha_bit_for_bit(name, monkeypatch):
    from imagecaptioning.pytorch_amd import att_trace
    got = {}
    real = att_trace.from_rollout
    monkeypatch.setattr(att_trace, 'from_rollout', lambda model, ro: (got.setdefault('ro', ro), real(model, ro))[1])
    model = golden_model(name)
    fc, att, masks, _ = feeds(name)
    col0 = int(name.startswith('adaatt'))
    seq, _ = sample(model, fc, att, masks, sample_method='greedy', beam_size=1, sample_n=2, return_attention=1)
    ro = got['ro']
    alpha = getattr(ro, ro.TRACE)                                   # [T, N, K (+ 1)]
    T, N, Kc = alpha.shape
    assert (T, N, Kc) == (6, 6, 5 + col0)
    want = torch.zeros(N, 6, 6 + col0, device=DEV)
    want[:, :, :Kc] = alpha.transpose(0, 1)
    keep = torch.cat([torch.ones(N, 1, dtype=torch.bool, device=DEV), seq[:, :-1] > 0], 1)
    want = torch.where(keep.unsqueeze(2), want, torch.zeros((), device=DEV))
    assert torch.equal(model.last_attention['att'], want)


@pytest.mark.parametrize('T,N,L,K,Kout,beta', [(5, 3, 5, 3, 7, False), (6, 7, 6, 5, 8, False), (4, 9, 7, 6, 8, True),
                                               (3, 2, 3, 70, 73, True), (2, 1, 2, 130, 132, False)])
def test_rollout_kernel_against_torch(T, N, L, K, Kout, beta):
    """odd widths (dword stores), widths that are a multiple of 4 (16-byte stores), more regions than lanes, more (row, step) pairs
    than one workgroup holds, fewer steps than the pitch, the optional leading column; source values behind a caption's end are
    NaN and must not reach the output"""
    from imagecaptioning.pytorch_amd import att_trace
    g = torch.Generator().manual_seed(T * 100 + N)
    alpha = torch.rand(T, N, K, generator=g)
    b = torch.rand(T, N, generator=g) if beta else None
    seq = torch.randint(1, 9, (N, L), generator=g)
    for r in range(N):
        end = int(torch.randint(0, L + 1, (1,), generator=g))
        seq[r, end:] = 0
    keep = torch.cat([torch.ones(N, 1, dtype=torch.bool), seq[:, :-1] > 0], 1)
    keep[:, T:] = False
    off = int(beta)
    want = torch.zeros(N, L, Kout)
    want[:, :T, off:off + K] = alpha.transpose(0, 1)
    if beta:
        want[:, :T, 0] = b.t()
    want = want * keep.unsqueeze(2)
    poison = alpha.clone()
    poison[~keep[:, :T].t()] = float('nan')
    got = att_trace.rollout(poison.to(DEV), seq.to(DEV), Kout, beta=None if b is None else b.to(DEV))
    assert torch.equal(got.cpu(), want)


def test_beam_kernel_against_torch():
    from imagecaptioning.pytorch_amd import att_trace
    g = torch.Generator().manual_seed(7)
    L, rows_src, rows, K = 6, 9, 5, 5
    for Kout in (6, 8):
        alpha = torch.rand(L, rows_src, K, generator=g)
        lineage = torch.randint(0, rows_src, (L, rows), generator=g).to(torch.int32)
        length = torch.tensor([6, 1, 3, 0, 4], dtype=torch.int32)
        for i in range(rows):
            lineage[int(length[i]):, i] = -1
        want = torch.zeros(rows, L, Kout)
        for i in range(rows):
            for t in range(int(length[i])):
                want[i, t, :K] = alpha[t, lineage[t, i]]
        got = att_trace.beam(alpha.to(DEV), lineage.to(DEV), length.to(DEV), Kout)
        assert torch.equal(got.cpu(), want)


def _replay(model, fc, att, masks, seq, n):
    """the trace of a forced replay of `seq` (rows image-major, n per image)"""
    sample(model, fc, att, masks, sample_method='greedy', beam_size=1, sample_n=n, _forced_seq=seq, return_attention=1)
    return model.last_attention


@pytest.mark.parametrize('opts', [dict(beam_size=3, sample_n=3), dict(beam_size=3, sample_n=1),
                                  dict(beam_size=4, group_size=2, sample_n=1, diversity_lambda=0.5),
                                  dict(beam_size=3, sample_n=1, decoding_constraint=1)],
                         ids=['beam3_all', 'beam3_best', 'diverse_2x2', 'beam3_constraint'])
def test_beam_trace_is_the_forced_replay_of_the_returned_beams(opts):
    """5e-5, not bit for bit: the search takes its first step on one row per image and the others on beam_size rows, through the
    single-step decoder, while the replay is one rollout of sample_n rows per image whose decode GEMMs read plane-staged operands
    -- other row counts and another accumulation order for the same weights (DESIGN section 2's bound for decode options)."""
    model = golden_model('updown')
    fc, att, masks, _ = feeds('updown')
    base = dict(sample_method='beam_search', **opts)
    seq0, logp0 = sample(model, fc, att, masks, **base)
    assert model.last_attention is None
    seq, logp = sample(model, fc, att, masks, return_attention=1, **base)
    la = model.last_attention
    assert torch.equal(seq, seq0) and torch.equal(logp, logp0)
    n = opts['sample_n']
    assert la['att'].shape == (3 * n, 6, 6)
    check_structure(la, seq, 5, 0)
    rep = _replay(model, fc, att, masks, seq, n)
    err = float((la['att'].double() - rep['att'].double()).abs().max())
    print('%s: max |beam trace - forced replay| = %.3g' % (opts, err))
    assert err <= TOL
    assert torch.equal(la['att'] == 0, rep['att'] == 0)
    check_ground(la, n, None, 0)


@pytest.mark.parametrize('name', ('att2in2', 'adaatt'))
def test_beam_trace_of_the_stepper_families(name):
    model = golden_model(name)
    fc, att, masks, _ = feeds(name)
    col0 = int(name.startswith('adaatt'))
    seq0, logp0 = sample(model, fc, att, masks, sample_method='beam_search', beam_size=3, sample_n=3)
    seq, logp = sample(model, fc, att, masks, sample_method='beam_search', beam_size=3, sample_n=3, return_attention=1)
    assert torch.equal(seq, seq0) and torch.equal(logp, logp0)
    la = model.last_attention
    assert la['att'].shape == (9, 6, 6 + col0)
    check_structure(la, seq, 5, col0)
    check_ground(la, 3, None, col0)


@pytest.mark.parametrize('opts', [dict(group_size=2, sample_method='greedy'), dict(sample_n=2, decoding_constraint=1, sample_method='greedy')],
                         ids=['diverse_sample', 'constraint'])
def test_host_stepped_sampling_trace_is_the_forced_replay(opts):
    """_diverse_sample and the constrained sampler run on the single-step decoder: rows stay aligned with the returned seq.  5e-5
    for the reason given above (stepper against rollout)."""
    model = golden_model('updown')
    fc, att, masks, _ = feeds('updown')
    seq0 = sample(model, fc, att, masks, beam_size=1, **opts)[0]
    seq = sample(model, fc, att, masks, beam_size=1, return_attention=1, **opts)[0]
    la = model.last_attention
    assert torch.equal(seq, seq0) and la['att'].shape == (6, 6, 6)
    check_structure(la, seq, 5, 0)
    rep = _replay(model, fc, att, masks, seq.contiguous(), 2)
    err = float((la['att'].double() - rep['att'].double()).abs().max())
    print('%s: max |stepper trace - forced replay| = %.3g' % (opts, err))
    assert err <= TOL


def test_ground_ties_zero_steps_and_wide_rows():
    from imagecaptioning.pytorch_amd import att_trace
    att = torch.zeros(2, 3, 4)
    att[0, 0] = torch.tensor([0.25, 0.375, 0.375, 0.0])             # a hand-made tie: the lowest index wins
    att[0, 1] = torch.tensor([0.0, 0.0, 0.5, 0.5])
    att[1, 2] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    g = att_trace.ground(att.to(DEV))
    assert g['top'].cpu().tolist() == [[1, 2, -1], [-1, -1, 3]]
    assert g['top_w'].cpu().tolist() == [[0.375, 0.5, 0.0], [0.0, 0.0, 1.0]]
    assert g['entropy'][1, 2].item() == 0.0 and g['entropy'][0, 2].item() == 0.0
    assert abs(g['entropy'][0, 1].item() - np.log(2.0)) < 1e-6
    # more regions than lanes, a tie across two lanes' strides, several workgroups, n rows per image, a leading column without a box
    gen = torch.Generator().manual_seed(3)
    N, L, Kw, n = 6, 5, 131, 2
    a = torch.rand(N, L, Kw, generator=gen)
    a[0, 0, 100] = a[0, 0, 36] = 2.0
    a = a / a.sum(-1, keepdim=True)
    a[3, 2:] = 0
    boxes = torch.rand(N // n, Kw - 1, 4, generator=gen)
    g = att_trace.ground(a.to(DEV), n, boxes.to(DEV), col0=1)
    want = R64.ground(a.double().numpy(), boxes.numpy(), n, 1)
    assert np.array_equal(g['top'].cpu().numpy(), want['top']) and want['top'][0, 0] == 36 and want['top'][3, 2] == -1
    for k in ('top_w', 'entropy', 'box'):
        assert float(np.abs(g[k].double().cpu().numpy() - want[k]).max()) <= TOL, k


def test_native_entries_refuse_bad_arguments():
    from imagecaptioning.pytorch_amd import _lib
    a = torch.zeros(2, 2, 4, device=DEV)
    seq = torch.zeros(2, 2, dtype=torch.long, device=DEV)
    out = torch.zeros(2, 2, 4, device=DEV)
    p = _lib.ptr
    assert _lib.lib.capmi_att_trace_rollout(p(a), None, p(seq), 2, 2, 2, 4, 3, p(out), None) == _lib.EINVAL      # K > Kout
    assert _lib.lib.capmi_att_trace_rollout(p(a), p(a), p(seq), 2, 2, 2, 4, 4, p(out), None) == _lib.EINVAL      # no room for beta
    assert _lib.lib.capmi_att_trace_rollout(p(a), None, p(seq), 3, 2, 2, 4, 4, p(out), None) == _lib.EINVAL      # T > L
    assert _lib.lib.capmi_att_trace_rollout(None, None, p(seq), 2, 2, 2, 4, 4, p(out), None) == _lib.EINVAL
    assert _lib.lib.capmi_att_trace_beam(p(a), None, None, 2, 2, 2, 4, 4, p(out), None) == _lib.EINVAL
    i32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert _lib.lib.capmi_att_ground(p(a), 2, 2, 4, p(a), 2, 1, 0, 4, p(i32), p(out), p(out), None, None) == _lib.EINVAL   # boxes without box
    assert _lib.lib.capmi_att_ground(p(a), 2, 2, 4, p(a), 1, 1, 0, 4, p(i32), p(out), p(out), p(out), None) == _lib.EINVAL  # B * n < N


@pytest.mark.parametrize('name', ('updown', 'adaatt'))
def test_option_off_changes_nothing(name):
    model = golden_model(name)
    fc, att, masks, _ = feeds(name)
    for opts in (dict(sample_method='greedy', beam_size=1, sample_n=2), dict(sample_method='beam_search', beam_size=3, sample_n=1)):
        seq0, logp0 = sample(model, fc, att, masks, **opts)                          # before the option was ever set on this model
        assert model.last_attention is None
        sample(model, fc, att, masks, return_attention=1, **opts)
        assert model.last_attention is not None
        seq1, logp1 = sample(model, fc, att, masks, return_attention=0, **opts)
        assert model.last_attention is None and model._trace_req is None
        seq2, logp2 = sample(model, fc, att, masks, **opts)
        assert torch.equal(seq0, seq1) and torch.equal(logp0, logp1) and torch.equal(seq0, seq2) and torch.equal(logp0, logp2)


def test_diverse_beam_with_sample_n_of_a_group_uses_each_images_own_boxes():
    """sample_n == beam_size // group_size > 1: as in the reference only the first B rows of seq are filled, row k with image k's best
    beam (CaptionModel.py:207-208, AttModel.py:247-256).  Their boxes are image k's, not image k // sample_n's; the other rows are
    zero rows with top -1."""
    model = golden_model('updown')
    fc, att, masks, boxes = feeds('updown')
    opts = dict(sample_method='beam_search', beam_size=4, group_size=2, sample_n=2, diversity_lambda=0.5)
    seq0, _ = sample(model, fc, att, masks, **opts)
    seq, _ = sample(model, fc, att, masks, return_attention=1, boxes=boxes, **opts)
    la = model.last_attention
    assert torch.equal(seq, seq0) and seq.shape[0] == 6 and not seq[3:].any()
    assert la['att'].shape == (6, 6, 6) and la['box'].shape == (6, 6, 4)
    assert not la['att'][3:].any() and bool((la['top'][3:] == -1).all()) and not la['box'][3:].any() and not la['entropy'][3:].any()
    first = {k: v[:3] for k, v in la.items()}
    check_structure(first, seq[:3], 5, 0)
    check_ground(first, 1, boxes, 0)                    # row k against boxes[k]
    rep = _replay(model, fc, att, masks, seq[:3].contiguous(), 1)
    assert float((first['att'].double() - rep['att'].double()).abs().max()) <= TOL
