"""Beam-search SCST (train_beam_size > 1) at CONFIG SIZE under dropout against the float64 restatement tests/beam_train_ref64.py,
computed on the CPU inside each test (nothing is stored), and kernel-level tests of the small beam kernels.

What tests/test_beam_train_gpu.py cannot see: at its fixture (R = E = 16, V1 = 31) every GEMM takes the small-shape route and a
wrong mask row gives a different but equally plausible number only the tiny golden notices.  Here B = 10, bd = 5, L = 20, K = 36,
R = E = 1000, V1 = 9488 (split-K slabs, A-plane kernels, 16-byte cells, top-5 of 47 440 candidates), keep masks injected through
opt['_beam_masks'] so that both sides see the same bits.

Ties: a top-bd choice between candidates closer than fp32 rounding is a coin flip.  Every case asserts on the REFERENCE's values,
before it looks at the HIP output, that the smallest kept / dropped gap and the smallest finalise-key gap are >= 1e-4 (the bound
of shapes.py's config-size beam fixtures); the seeds in shapes.BEAM_TRAIN_SEED were picked with the reference alone.

Tolerances (all from the project, none from the kernels' output): score / p / seqLogprobs rtol = atol = 1e-4
(test_beam5_at_config_size_vs_the_reference_itself); loss 1e-4 absolute and max|grad - ref| / max|ref| < 1e-3 per parameter
(test_full_size_scst_sample_and_grads_vs_oracle; core.attention.alpha_net.bias is mathematically zero and excluded as there).  A
parameter that misses 1e-3 is not waved through: the same restatement is then run in float32 on the CPU and the parameter must be
within 4 x that run's own error against float64 (fp32 GEMMs with different summation orders differ by a small multiple of each
other; a real defect shows as percent-level error).  The odd-sized tiny cases use LOGP_TOL and the gradient rule of
tests/test_beam_train_gpu.py.
"""
import numpy as np
import pytest
import torch

import beam_train_ref64 as ref
import shapes
from test_beam_train_gpu import LOGP_TOL, d, masks_to_dev, philox_search_and_replay_agree

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MIN_GAP = 1e-4
CONFIG_TOL = dict(rtol=1e-4, atol=1e-4)
NAN = float('nan')


# --------------------------------------------------------------------------------------------------------------- cases
def _opt(family, **over):
    from imagecaptioning.pytorch_amd import synthetic
    return synthetic.updown_opt(caption_model=family, drop_prob_lm=0.5, **over)


def _shapes_of(opt):
    """state_dict shapes of the HIP mirror (built on the CPU; nothing is launched)."""
    from imagecaptioning.pytorch_amd.captioning import models
    return {k: v.shape for k, v in models.setup(opt).state_dict().items()}


def _sharpen(st, eos_bias):
    st['logit.weight'] = st['logit.weight'] * shapes.BEAM5_LOGIT_SCALE
    st['logit.bias'] = st['logit.bias'].clone()
    st['logit.bias'][0] += eos_bias
    return st


ODD = dict(rnn_size=30, input_encoding_size=18, att_hid_size=10, vocab_size=36, seq_length=7, max_length=7, fc_feat_size=22,
           att_feat_size=22, vocab={str(i): 'w%d' % i for i in range(1, 37)})

#        name             family    weights     B   bd  n   L   penalty   att_masks
CASES = {'mid':          ('updown', 'mid',      10, 5,  5,  20, '',        True),
         'mid_wu':       ('updown', 'mid',      10, 5,  5,  20, 'wu_0.7',  True),
         'sharp_n1':     ('updown', 'sharp',    10, 5,  1,  20, '',        False),
         'rows80':       ('updown', 'mid',      16, 5,  5,  12, '',        True),
         'newfc_n5':     ('newfc',  'sharp',    10, 5,  5,  20, '',        False),
         'newfc_n1':     ('newfc',  'sharp',    10, 5,  1,  20, '',        False),
         'odd_updown':   ('updown', 'odd',      3,  3,  3,  7,  '',        True),
         'odd_newfc':    ('newfc',  'odd',      3,  3,  3,  7,  '',        False)}
CONFIG_CASES = [c for c in CASES if not c.startswith('odd')]


def make_case(name, seed=None, mask_seed=None):
    """Everything a case needs, on the CPU, from seeded generators: opt, weights, inputs, keep masks by search row, reward."""
    from oracle import att_lstm as O
    family, weights, B, bd, n, L, pen, masked = CASES[name]
    seed = shapes.BEAM_TRAIN_SEED[name][0] if seed is None else seed
    mask_seed = shapes.BEAM_TRAIN_SEED[name][1] if mask_seed is None else mask_seed
    odd = weights == 'odd'
    opt = _opt(family, **ODD) if odd else _opt(family, seq_length=L, max_length=L)
    K, F = (6, 22) if odd else (36, 2048)
    if weights == 'mid':
        P = shapes.mid_state('updown', None, seed)
    elif weights == 'sharp' and family == 'updown':
        P = shapes.beam5_state('updown', None, seed)
    elif weights == 'sharp':
        P = _sharpen(shapes.seeded_state(_shapes_of(opt), seed), shapes.BEAM_TRAIN_NEWFC_EOS_BIAS)
    else:       # odd sizes: a random-init logit layer is nearly uniform over 37 words (the search would not depend on the masks)
        P = shapes.seeded_state(_shapes_of(opt), seed)
        P['logit.weight'] = P['logit.weight'] * shapes.BEAM_TRAIN_ODD_LOGIT_SCALE
        P['logit.bias'] = P['logit.bias'].clone()
        P['logit.bias'][0] += shapes.BEAM_TRAIN_ODD_EOS_BIAS
    fc, att = shapes.feats(B, K=K, F=F, seed=seed)
    am = shapes.ragged_masks(B, K=K, seed=seed, lo=3 if odd else 10) if masked else None
    g = torch.Generator().manual_seed(mask_seed)
    masks = ref.mask_dict(family, O.make_drops(0.5, B, K, B * bd, L, opt.input_encoding_size, opt.rnn_size, g))
    reward = torch.randn(B * n, 1, generator=g).repeat(1, L)
    return dict(name=name, family=family, opt=opt, P=P, fc=fc, att=att, am=am, masks=masks, reward=reward, B=B, bd=bd, n=n, L=L, pen=pen)


def reference(c):
    r = ref.run(c['family'], c['P'], c['fc'], c['att'], c['am'], c['bd'], c['n'], c['L'], c['pen'], c['masks'], reward=c['reward'])
    print('%s: reference gap %.3e  p_gap %.3e  min score %.2f  lengths %s' % (c['name'], r['gap'], r['p_gap'], r['score'][r['score'] > -500].min(),
                                                                            sorted(set(r['length'].tolist()))))
    return r


def assert_fair(c, r):
    """on the reference alone, before the HIP output is looked at"""
    assert r['gap'] >= MIN_GAP and r['p_gap'] >= MIN_GAP, \
        '%s: the float64 search has a near tie (gap %.3e, finalise-key gap %.3e < %.0e): pick another seed in shapes.BEAM_TRAIN_SEED' \
        % (c['name'], r['gap'], r['p_gap'], MIN_GAP)


def hip_model(c):
    from imagecaptioning.pytorch_amd.captioning import models
    model = models.setup(c['opt'])
    model.load_state_dict(c['P'])
    return model.to(DEV).train()


def hip_run(c, model):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    model.zero_grad(set_to_none=True)
    o = dict(sample_method='greedy', beam_size=c['bd'], sample_n=c['n'], length_penalty=c['pen'], _beam_masks=masks_to_dev(c['masks']))
    seq, slp = model(d(c['fc']), d(c['att']), d(c['am']), opt=o, mode='sample')
    assert slp.requires_grad and model.done_beams is None
    loss = losses.RewardCriterion()(slp, seq.data, c['reward'].to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return seq, slp.detach(), loss.item(), {k: v.clone() for k, v in model._last_beam.items()}


def compare_search(c, r, seq, slp, tabs, tol):
    for k in ('parent', 'token', 'ended'):
        assert np.array_equal(tabs[k].cpu().numpy().astype(np.int64), r[k].astype(np.int64)), k
    np.testing.assert_allclose(tabs['score'].cpu().numpy(), r['score'], **tol)
    assert np.array_equal(seq.cpu().numpy(), r['seq'])
    assert np.array_equal(tabs['length'].cpu().numpy(), r['length'])
    assert np.array_equal(tabs['lineage'].cpu().numpy(), r['lineage'])          # -1 behind a beam's end on both sides
    np.testing.assert_allclose(tabs['p'].cpu().numpy(), r['p'], **tol)
    got = slp.cpu().numpy()
    for row in range(got.shape[0]):                                             # rows zero behind a beam's end
        assert not got[row, int(r['length'][row]):].any(), row
    np.testing.assert_allclose(got, r['logp'].numpy(), **tol)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def compare_grads_config(c, r, model, loss):
    assert abs(loss - r['loss']) < 1e-4, (loss, r['loss'])
    missed = []
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        g = r['grads'][k]
        err = _rel(p.grad, g)
        print('%s %-34s max|ref| %.3e  max err %.3e  rel %.3e' % (c['name'], k, float(g.abs().max()),
                                                                  float((p.grad.double().cpu() - g).abs().max()), err))
        if k != 'core.attention.alpha_net.bias' and not err < 1e-3:             # alpha_net.bias: mathematically zero
            missed.append((k, err))
    if missed:
        _, _, g32 = ref.replay_loss_grads(c['family'], c['P'], c['fc'], c['att'], c['am'], r['seq'], r['lineage'], c['n'], c['masks'],
                                          c['reward'], dtype=torch.float32)
        for k, err in missed:
            own = _rel(g32[k], r['grads'][k])
            print('%s %-34s rel %.3e misses 1e-3; float32 restatement on the CPU: rel %.3e, bound %.3e' % (c['name'], k, err, own, 4 * own))
            assert err < 4 * own, (k, err, own)


# ------------------------------------------------------------------------------------------- 1. config-size parity
@pytest.mark.parametrize('name', CONFIG_CASES)
def test_config_size_beam_search_scst_under_dropout_vs_float64(name):
    """Search tables / seq / lineage / length exact, score / p / seqLogprobs within 1e-4, RewardCriterion loss within 1e-4 and
    every parameter gradient within 1e-3 of its largest reference element (module docstring).  `rows80` runs 80 search rows: the
    A-plane kernels stop at 64, so search steps and replay take the other GEMM route.  A wrong mask slot in the search, a lineage
    read at the wrong step or a gather that takes the replay's row count for the search's changes tokens or log-probs at percent
    level here and fails on the first comparison that sees it."""
    c = make_case(name)
    r = reference(c)
    assert_fair(c, r)
    model = hip_model(c)
    seq, slp, loss, tabs = hip_run(c, model)
    compare_search(c, r, seq, slp, tabs, CONFIG_TOL)
    compare_grads_config(c, r, model, loss)


@pytest.mark.parametrize('family', ['updown', 'newfc'])
def test_odd_sized_model_trains_with_a_beam_search(family):
    """rnn_size 30, input_encoding_size 18, att_hid_size 10, V1 37, L 7, bd 3, B 3, ragged att_masks (updown): no dimension is a
    multiple of 4, so every kernel takes its scalar route and the selection runs as BSEL<4>.  capmi_lineage_gather used to
    refuse widths off a multiple of 4 (`C_a % 4` -> CAPMI_EINVAL, read from its code) while every other kernel a plain sampled
    SCST step reaches has a scalar route; it now has one too, and the sampled step below is run to show the sizes train."""
    c = make_case('odd_' + family)
    r = reference(c)
    assert_fair(c, r)
    model = hip_model(c)
    torch.manual_seed(3)
    s_seq, s_slp = model(d(c['fc']), d(c['att']), d(c['am']), opt=dict(sample_method='sample', sample_n=3), mode='sample')
    s_slp.gather(2, s_seq.unsqueeze(2)).sum().backward()                       # plain sampled SCST at these sizes
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    seq, slp, loss, tabs = hip_run(c, model)
    compare_search(c, r, seq, slp, tabs, LOGP_TOL)
    np.testing.assert_allclose(loss, r['loss'], rtol=1e-5)
    for k, p in model.named_parameters():
        g = r['grads'][k].numpy()
        print('%s %-34s max|ref| %.3e  max err %.3e' % (c['name'], k, np.abs(g).max(), np.abs(p.grad.cpu().numpy() - g).max()))
        np.testing.assert_allclose(p.grad.cpu().numpy(), g, rtol=5e-4, atol=1e-6 + 2e-5 * np.abs(g).max(), err_msg=k)


@pytest.mark.parametrize('name', ['mid', 'newfc_n5'])
def test_philox_masks_are_shared_by_search_and_replay_at_config_size(name):
    """Without injected masks (drop_prob_lm 0.5, model._dropout_masks(B, K, B*bd, L, dev) / ops.dropout_mask laid out by search
    row): the check of the tiny-size test at B = 10, bd = 5, L = 20, with the config-size log-prob tolerance."""
    c = make_case(name)
    model = hip_model(c)
    philox_search_and_replay_agree(model, d(c['fc']), d(c['att']), d(c['am']), c['bd'], CONFIG_TOL)


# ------------------------------------------------------------------------------------------- 2. the small beam kernels
PAD = 256


def guarded(shape, misalign=0):
    """a float32 tensor of `shape` inside a larger buffer filled with NaN: (buffer, view).  A write past either end is seen by
    guard_intact; a position the kernel left out stays NaN."""
    n = int(np.prod(shape))
    buf = torch.full((PAD + misalign + n + PAD,), NAN, device=DEV)
    return buf, buf[PAD + misalign:PAD + misalign + n].view(*shape)


def guard_intact(buf, view, misalign=0):
    n = view.numel()
    return bool(torch.isnan(buf[:PAD + misalign]).all()) and bool(torch.isnan(buf[PAD + misalign + n:]).all())


def _lineage(g, L, rows_src, rows_dst):
    lin = torch.randint(0, rows_src, (L, rows_dst), generator=g, dtype=torch.int32)
    for i in range(rows_dst):
        n = int(torch.randint(1, L + 1, (1,), generator=g))
        lin[n:, i] = -1                                                         # behind the beam's end
    lin[0, 0] = rows_src + 3                                                    # clamped, never followed out of the array
    return lin


#                 L   rows_src rows_dst C_a   C_b   misalign
GATHER_CASES = [(8,  50,      10,      4,    None, 0),
                (20, 50,      50,      1000, None, 0),
                (20, 50,      10,      1000, 1000, 0),
                (24, 50,      50,      1024, 1024, 0),           # 614 400 float4 moves: more than one grid stride (2048 x 256)
                (20, 50,      10,      None, 1024, 0),
                (20, 50,      50,      4,    1000, 1),           # widths allow 16-byte moves, the pointers do not
                (7,  9,       9,       30,   18,   0),           # the scalar route
                (7,  9,       3,       30,   None, 0),
                (7,  9,       9,       None, 1,    0),
                (5,  50,      50,      1,    4,    0),
                (20, 50,      50,      1001, None, 0)]           # 1 001 000 scalar moves: more than one grid stride


@pytest.mark.parametrize('L,rows_src,rows_dst,Ca,Cb,misalign', GATHER_CASES)
def test_lineage_gather_vs_torch(L, rows_src, rows_dst, Ca, Cb, misalign):
    """capmi_lineage_gather == src[t, lineage[t].clamp(0, rows_src - 1)], exactly, for one array, two arrays and the second
    alone, and nothing is written around the outputs."""
    from imagecaptioning.pytorch_amd._lib import lib, check, ptr, stream_ptr
    g = torch.Generator().manual_seed(L * 1000 + rows_dst + (Ca or 0) + (Cb or 0))
    lin = _lineage(g, L, rows_src, rows_dst)
    src, out = [], []
    for C in (Ca, Cb):
        src.append(None if C is None else torch.randn(L, rows_src, C, generator=g).to(DEV))
        out.append((None, None) if C is None else guarded((L, rows_dst, C), misalign))
    lin_d = lin.to(DEV)
    check(lib.capmi_lineage_gather(ptr(lin_d), L, rows_src, rows_dst, ptr(src[0]), ptr(out[0][1]), Ca or 0, ptr(src[1]), ptr(out[1][1]),
                                   Cb or 0, stream_ptr()), 'capmi_lineage_gather')
    torch.cuda.synchronize()
    idx = lin.long().clamp(0, rows_src - 1)
    for s, (buf, view) in zip(src, out):
        if s is None:
            continue
        want = torch.stack([s.cpu()[t, idx[t]] for t in range(L)])
        assert torch.equal(view.cpu(), want)
        assert guard_intact(buf, view, misalign)


def test_lineage_gather_through_the_python_wrapper():
    from imagecaptioning.pytorch_amd import beam
    g = torch.Generator().manual_seed(11)
    for rows_dst, Ca, Cb in ((10, 1000, 1000), (50, 30, None), (10, None, 18)):
        L, rows_src = 20, 50
        lin = _lineage(g, L, rows_src, rows_dst)
        a = None if Ca is None else torch.randn(L, rows_src, Ca, generator=g).to(DEV)
        b = None if Cb is None else torch.randn(L, rows_src, Cb, generator=g).to(DEV)
        oa, ob = beam.lineage_gather(lin.to(DEV), rows_src, a, b)
        idx = lin.long().clamp(0, rows_src - 1)
        for s, o in ((a, oa), (b, ob)):
            assert (s is None) == (o is None)
            if s is not None:
                assert torch.equal(o.cpu(), torch.stack([s.cpu()[t, idx[t]] for t in range(L)]))


@pytest.mark.parametrize('arrays,B,bd,R', [(1, 10, 5, 1000), (2, 10, 5, 1000), (4, 10, 5, 1000), (4, 3, 3, 30), (2, 16, 5, 30),
                                           (4, 32, 5, 1000)])          # the last: 640 000 elements, above 2048 blocks x 256
@pytest.mark.parametrize('first', [True, False])
def test_beam_reorder_vs_torch(arrays, B, bd, R, first):
    """capmi_beam_reorder == src[a, b*cur + parent[b, j]] for cur = 1 (first step: B live rows inside [B*bd]-row arrays) and
    cur = bd, exactly, nothing written around the output."""
    from imagecaptioning.pytorch_amd import beam
    cur = 1 if first else bd
    g = torch.Generator().manual_seed(arrays * 100 + B + R + cur)
    src = torch.randn(arrays, B * bd, R, generator=g)
    parent = torch.randint(0, cur, (B, bd), generator=g, dtype=torch.int32)
    buf, dst = guarded((arrays, B * bd, R))
    beam.reorder_rows(src.to(DEV), dst, parent.to(DEV), B, cur, bd)
    torch.cuda.synchronize()
    rows = (torch.arange(B).unsqueeze(1) * cur + parent.long()).reshape(-1)
    assert torch.equal(dst.cpu(), src[:, rows])
    assert guard_intact(buf, dst)


@pytest.mark.parametrize('V1', [31, 9488, 10241])
@pytest.mark.parametrize('temperature', [1.0, 2.0])
@pytest.mark.parametrize('unk', [False, True])
def test_beam_logsoftmax_vs_float64(V1, temperature, unk):
    """capmi_beam_logsoftmax vs float64: log_softmax(x), divided by the temperature and normalised again (CaptionModel.py:203-204
    as the kernel documents it), the UNK column pushed down by 1000 -- rows with a -inf logit and rows with one dominant logit
    included.  1e-5 absolute, the bound of test_log_softmax_rows (values down to about -40: a few fp32 ulps); the UNK column,
    stored near -1000, gets float32's own half unit in the last place (3.05e-5) on top -- measured there on an MI355X: 2.97e-5."""
    from imagecaptioning.pytorch_amd._lib import lib, check, ptr, stream_ptr
    rows = 50
    g = torch.Generator().manual_seed(V1 + int(temperature * 10) + unk)
    x = torch.randn(rows, V1, generator=g) * 4
    x[3, 5] = float('-inf')
    x[4, V1 - 1] = float('-inf')
    x[7, 11] = x[7].max() + 15.0                                                # one dominant logit: p > 0.999
    x[8, 0] = x[8].max() + 15.0
    unk_col = V1 - 1 if unk else -1
    buf, out = guarded((rows, V1))
    check(lib.capmi_beam_logsoftmax(ptr(x.to(DEV)), ptr(out), rows, V1, temperature, unk_col, stream_ptr()), 'capmi_beam_logsoftmax')
    torch.cuda.synchronize()
    want = torch.log_softmax(torch.log_softmax(x.double(), -1) / temperature, -1)
    if unk:
        want[:, unk_col] -= 1000.0
    got = out.double().cpu()
    inf = torch.isinf(want)
    assert int(inf.sum()) == 2 and torch.equal(got[inf], want[inf])
    # 1e-5 on the value; the pushed-down UNK column sits near -1000, where float32 itself resolves 6.1e-5: half a unit in the last
    # place of the stored number is added there (the kernel's `y -= 1000.f` rounds once), and nowhere else
    bound = torch.full_like(want, 1e-5)
    if unk:
        bound[:, unk_col] += 0.5 * torch.from_numpy(np.spacing(want[:, unk_col].abs().float().numpy())).double()
    live = ~inf
    assert bool(((got[live] - want[live]).abs() < bound[live]).all()), float((got[live] - want[live]).abs().max())
    assert guard_intact(buf, out)


def test_beam_finalize_at_its_size_limit_and_beyond():
    """L * bd == 1024 (the LDS table of capmi_beam_finalize) equals ref.finalize; L * bd > 1024 and sample_n > bd are refused
    by name before anything is launched."""
    from imagecaptioning.pytorch_amd import beam
    from imagecaptioning.pytorch_amd._lib import CapmiError
    from test_beam_train_host import random_tables
    rng = np.random.RandomState(17)
    B, bd, L = 2, 16, 64
    tabs = random_tables(rng, B, bd, L, False)
    dev = [torch.from_numpy(a).to(DEV) for a in tabs]
    for sample_n, pen in ((16, ''), (1, 'wu_0.7')):
        seq, lineage, length, p = beam.finalize(*dev, sample_n, pen)
        torch.cuda.synchronize()
        seq_r, lin_r, len_r, p_r, _ = ref.finalize(*tabs, sample_n, pen)
        assert np.array_equal(seq.cpu().numpy(), seq_r) and np.array_equal(lineage.cpu().numpy(), lin_r)
        assert np.array_equal(length.cpu().numpy(), len_r)
        assert torch.equal(p.cpu(), torch.from_numpy(p_r).float())
    big = [torch.from_numpy(a).to(DEV) for a in random_tables(rng, B, bd, L + 1, False)]
    with pytest.raises(CapmiError, match='capmi_beam_finalize'):
        beam.finalize(*big, 1, '')
    with pytest.raises(CapmiError, match='capmi_beam_finalize'):
        beam.finalize(*dev, bd + 1, '')
