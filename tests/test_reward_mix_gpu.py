"""Device BLEU-4 and self-CIDEr rewards (csrc/reward_mix.hip, ciderd.DeviceCiderD.bleu4 / .self_cider, rewards.py, losses.py):
the kernels against the float64 restatement tests/rewards_ref64.py, the call site against tests/golden/reward_mix.npz (recorded
from the reference's own rewards.py / losses.py), LossWrapper end to end, the unchanged default, and a captured training step.
Integers must match exactly and K must be exactly symmetric; floats are held within 4 x the deviation measured on an MI355X where
K has full rank, and within the backward-error bound of a symmetric eigensolver where it has not."""
import argparse
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import ciderd as OC

import rewards_ref64 as W
from test_langeval_gpu import _rel
from test_model_api_gpu import tiny_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# Largest relative deviation from rewards_ref64.py over the cases of this file, measured on an MI355X.  The kernels work in double
# and in a fixed order; the deviation comes from the device's pow / exp / log / sqrt, the order of the n-gram sums (a dict's order
# in the restatement) and, for self-CIDEr, cyclic Jacobi against LAPACK (both backward stable; lambda_min > 1e-3 keeps that
# relative).  The bounds are 4 x the measured values, the margin tests/test_langeval_gpu.py uses.
# Self-CIDEr's figure is larger than the evaluation's (3.3e-15) because the weights are differences of logarithms, log(ref_len)
# on the host minus log(df) on the device: with ref_len = 60 here and df up to 59, one ulp between the two logarithms is
# amplified by log(60) / (log(60) - log(59)) = 243 before it reaches K.
# BLEU-4: only the case L = 5, n = 2 has a figure from the card, 1.599e-15; the other three are NOT MEASURED, so the constant is
# not a maximum over measurements.  It is reasoned instead and holds as it stands: host and device evaluate the same correctly rounded divisions, products
# and differences on equal integers, so they differ only by their pow (the fourth root) and exp (the brevity penalty): at most
# 2 ulp each on the device and 1 ulp each in glibc, plus the rounding of their product -- 6.5 ulp = 1.45e-15, taken as the figure.
MEASURED_BLEU_REL = 6.5 * 2.0 ** -52
MEASURED_SELF_CIDER_REL = 5.057e-14    # n = 2: 2.825e-14; n = 5: 4.794e-14; n = 32: 5.057e-14
BLEU_TOL = 4 * MEASURED_BLEU_REL
SELF_CIDER_TOL = 4 * MEASURED_SELF_CIDER_REL

V = 12                         # word ids 1..11: n-grams repeat and clip
CORPUS = OC.synthetic_corpus(60, V - 1, 5, 20, seed=5)
DF, REF_LEN = OC.build_document_frequency([[OC.tokens_of(r) for r in g] for g in CORPUS])


@pytest.fixture(scope='module')
def scorer():
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD
    return DeviceCiderD(DF, REF_LEN, torch.device(DEV))


def _words(rng, length, width):
    row = np.zeros(width, dtype=np.int64)
    row[:length] = rng.integers(1, V, size=length)
    return row


def _bleu_case(L, n):
    """4 images with 1, 2, 5, 5 references of widths 5, 20, 5, 20 (pack_refs pads to 20 and marks the full narrow rows with -1);
    n rows per image of width L, the special rows among them"""
    rng = np.random.default_rng(1000 * L + n)
    gts = [np.stack([_words(rng, 5, 5)]),                                                   # one full row: no 0, gets the marker
           np.stack([_words(rng, int(rng.integers(3, 21)), 20) for _ in range(2)]),
           np.stack([_words(rng, int(rng.integers(1, 4)), 5) for _ in range(5)]),            # at most 3 words + the 0
           np.stack([_words(rng, int(rng.integers(6, 21)), 20) for _ in range(5)])]          # at least 6 words
    B = len(gts)
    hyp = np.zeros((B * n, L), dtype=np.int64)
    for r in range(B * n):
        src = gts[r // n][int(rng.integers(0, len(gts[r // n])))]
        row = np.zeros(L, dtype=np.int64)
        m = min(L, src.shape[0])
        row[:m] = src[:m]
        flip = rng.random(L) < 0.3
        row[flip] = rng.integers(0, V, size=int(flip.sum()))
        hyp[r] = row
    hyp[0] = 0                                                                               # EOS at step 0: the caption "0"
    hyp[1, :min(L, 5)] = gts[0][0][:min(L, 5)]                                               # equal to a reference (L = 5)
    hyp[1, 5:] = 0
    hyp[n] = 0
    hyp[n, :min(L, 20)] = gts[1][0][:min(L, 20)]                                             # equal to a reference (L = 20)
    hyp[n + 1] = rng.integers(1, V, size=L)                                                  # no EOS
    hyp[2 * n] = rng.integers(1, V, size=L)                                                  # longer than every reference
    hyp[2 * n + 1, :4] = [V + 3, V + 4, 1, 2]                                                # words the table has never seen
    hyp[2 * n + 1, 4:] = 0
    hyp[3 * n] = 0
    hyp[3 * n, 0] = gts[3][0][0]                                                             # shorter than every reference
    hyp[3 * n + 1, :3] = 7                                                                   # a repeated word, clipped
    return gts, hyp


@pytest.mark.parametrize('L', [5, 20])
@pytest.mark.parametrize('n', [2, 5])
def test_bleu4_kernel_matches_the_restatement(scorer, L, n):
    gts, hyp = _bleu_case(L, n)
    H = hyp.shape[0]
    want_stats = np.array([g + c + [tl, rl] for g, c, tl, rl in (W.bleu_stats(hyp[r], gts[r // n]) for r in range(H))])
    want = np.array([W.bleu4(hyp[r], gts[r // n]) for r in range(H)])
    lens = np.array([len(W.tokens_of(r)) for r in hyp])
    ref_lens = [[len(W.tokens_of(r)) for r in g] for g in gts]
    assert lens[0] == 1 and lens[n + 1] == L and lens[2 * n] > max(ref_lens[2]) and lens[3 * n] < min(ref_lens[3])
    assert want[1 if L == 5 else n] > 1 - 1e-8                     # the row equal to a reference
    packed = scorer.pack_refs(gts)
    assert (packed[0].cpu().numpy() == -1).sum() == 1              # the full row of a narrow array
    hyp_d = torch.from_numpy(hyp).to(DEV)
    img = (torch.arange(H, device=DEV) // n).to(torch.int32)
    stats = torch.zeros(H, 10, dtype=torch.int32, device=DEV)
    got = scorer.bleu4(hyp_d, img, packed, 0.0, 1.0, stats=stats)
    np.testing.assert_array_equal(stats.cpu().numpy(), want_stats)
    dev = _rel(got.cpu().numpy(), want)
    print('bleu4 L = %d n = %d: max relative deviation %.3e' % (L, n, dev))
    # the mix: two rounded products and a rounded sum, as numpy computes them from the device's own BLEU
    base = torch.from_numpy(np.random.default_rng(3).random(H) * 3).to(DEV)
    mixed = scorer.bleu4(hyp_d, img, packed, 0.7, 0.3, base=base.clone())
    np.testing.assert_array_equal(mixed.cpu().numpy(), 0.7 * base.cpu().numpy() + 0.3 * got.cpu().numpy())
    np.testing.assert_array_equal(scorer.bleu4(hyp_d, img, packed, 0.7, 0.3).cpu().numpy(), 0.3 * got.cpu().numpy())
    assert torch.equal(scorer.bleu4(hyp_d, img, packed, 0.0, 1.0), got)          # run to run: the same bits
    assert dev <= BLEU_TOL, (dev, BLEU_TOL)


def _well_conditioned(n, L=20):
    """4 images, n captions each: a reference of the corpus of its own (none used twice) with about 30 % of its words replaced"""
    rng = np.random.default_rng(77 + n)
    pool = [r.astype(np.int64) for g in CORPUS for r in g]
    order = rng.permutation(len(pool))
    rows = np.zeros((4 * n, L), dtype=np.int64)
    for r in range(4 * n):
        row = pool[order[r]][:L].copy()
        words = int((row > 0).sum())
        flip = rng.random(words) < 0.3
        row[:words][flip] = rng.integers(1, V, size=int(flip.sum()))
        rows[r] = row
    return rows


@pytest.mark.parametrize('n', [2, 5, 32])
def test_self_cider_kernel_on_full_rank_groups(scorer, n):
    rows = _well_conditioned(n)
    sdf = W._shift_df(DF)
    parts = [W.self_cider_parts(rows[i:i + n], DF, REF_LEN, sdf) for i in range(0, len(rows), n)]
    assert min(p[1].min() for p in parts) > 1e-3                   # condition, not measurement: every image, none skipped
    got, K, eig = scorer.self_cider(torch.from_numpy(rows).to(DEV), n, parts=True)
    K, eig, got = K.cpu().numpy(), eig.cpu().numpy(), got.cpu().numpy()
    np.testing.assert_array_equal(K, K.transpose(0, 2, 1))
    dev = max(_rel(K, np.stack([p[0] for p in parts])), _rel(eig, np.stack([p[1] for p in parts])),
              _rel(got, np.array([p[2] for p in parts])))
    again = scorer.self_cider(torch.from_numpy(rows).to(DEV), n)
    assert np.array_equal(again.cpu().numpy(), got) and ((0 < got) & (got < 1)).all()
    print('self_cider n = %d: max relative deviation %.3e' % (n, dev))
    assert dev <= SELF_CIDER_TOL, (dev, SELF_CIDER_TOL)


def test_self_cider_kernel_on_rank_deficient_groups():
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD
    n, L = 5, 8
    df = dict(DF)
    import itertools
    for k in range(1, 5):                                          # every n-gram over {7, 0} is in every image: weight exactly 0
        for g in itertools.product((7, 0), repeat=k):
            df[g] = float(REF_LEN)
    sc = DeviceCiderD(df, REF_LEN, torch.device(DEV))
    rng = np.random.default_rng(9)
    groups = [[[3, 4, 5, 6, 1, 0, 0, 0]] * n,                                                        # identical captions
              [[7, 0, 0, 0, 0, 0, 0, 0], [7, 7, 0, 0, 0, 0, 0, 0], [7, 7, 7, 0, 0, 0, 0, 0], [0] * 8, [7] * 8],   # no weight at all
              [list(_words(rng, 6, L))] * 2 + [list(_words(rng, int(rng.integers(2, 8)), L)) for _ in range(3)],  # two equal rows
              [[V + 5, V + 6, V + 7, 0, 0, 0, 0, 0]] * 2 + [[1, 2, 0, 0, 0, 0, 0, 0]] * 3]           # two clusters, unseen words
    rows = np.array([r for g in groups for r in g], dtype=np.int64)
    sdf = W._shift_df(df)
    parts = [W.self_cider_parts(rows[i:i + n], df, REF_LEN, sdf) for i in range(0, len(rows), n)]
    got, K, eig = sc.self_cider(torch.from_numpy(rows).to(DEV), n, parts=True)
    K, eig, got = K.cpu().numpy(), eig.cpu().numpy(), got.cpu().numpy()
    np.testing.assert_array_equal(K, K.transpose(0, 2, 1))
    assert np.isfinite(got).all() and np.isfinite(eig).all()
    assert got[1] == 0.0 and not K[1].any() and parts[1][2] == 0.0           # the all-zero-weight image: 0.0, not NaN
    want_eig = np.stack([p[1] for p in parts])
    # backward error of a symmetric eigensolver on K/10 (entries <= 1, norm <= n), both solvers: delta absolute on eig; then
    # self_cider = -log(sqrt(l_max) / s) / log n with s = sum sqrt(l), and |sqrt(a) - sqrt(b)| <= sqrt(|a - b|)
    delta = 64 * n * n * 2.0 ** -52
    assert np.abs(eig - want_eig).max() <= delta
    assert _rel(K, np.stack([p[0] for p in parts])) <= 1e-13
    s = np.sqrt(np.clip(want_eig, 0, None)).sum(axis=1)
    want = np.array([p[2] for p in parts])
    assert (np.abs(got - want)[s > 0] <= n * np.sqrt(delta) / (s[s > 0] * np.log(n))).all(), (got, want)
    assert abs(got[0]) < 1e-6                                                # identical captions: no diversity


def test_bad_arguments_are_refused(scorer):
    from imagecaptioning.pytorch_amd._lib import CapmiError
    gts, hyp = _bleu_case(5, 2)
    packed = scorer.pack_refs(gts)
    img = (torch.arange(8, device=DEV) // 2).to(torch.int32)
    with pytest.raises(CapmiError):                                           # 65 columns: beyond capmi_ciderd_score's row width
        scorer.bleu4(torch.zeros(8, 65, dtype=torch.long, device=DEV), img, packed, 1.0, 1.0)
    for n in (1, 33):
        with pytest.raises(ValueError, match='self-CIDEr'):
            scorer.self_cider(torch.zeros(n * 2, 5, dtype=torch.long, device=DEV), n)
    with pytest.raises(CapmiError):
        scorer.self_cider(torch.zeros(4, 65, dtype=torch.long, device=DEV), 2)


# ---- call site ---------------------------------------------------------------------------------------------------------------
def _stub_scorer(z):
    """a DeviceCiderD whose three scorers hand back the fixture's recorded outputs as device tensors; the BLEU stub mixes as the
    BLEU launch does (that arithmetic is held bit for bit by test_bleu4_kernel_matches_the_restatement).  Everything around them
    -- which scorer runs for which weights, the advantage launches, the layout of the results -- is the product's."""
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD, PackedRefs

    class Stub(DeviceCiderD):
        def __init__(self):
            self.device = torch.device(DEV)
            self.calls = []

        def pack_refs(self, gts):
            return PackedRefs(torch.zeros(len(gts), 1, 1, dtype=torch.int32, device=DEV), torch.ones(len(gts), dtype=torch.int32, device=DEV))

        def score(self, hyp, hyp_img, refs, n_refs, cooked=None):
            self.calls.append('ciderd')
            return torch.from_numpy(z['cider'][:hyp.shape[0]].copy()).to(DEV)

        def bleu4(self, hyp, hyp_img, packed, cw, bw, base=None, stats=None):
            self.calls.append('bleu')
            b = bw * torch.from_numpy(z['bleu'][:hyp.shape[0]].copy()).to(DEV)
            return cw * base + b if base is not None else b

        def self_cider(self, hyp, n, parts=False):
            self.calls.append('self_cider')
            return torch.from_numpy(z['self_cider'].copy()).to(DEV)
    return Stub()


def test_call_site_matches_the_reference():
    from imagecaptioning.pytorch_amd.captioning.utils import rewards as R
    z = np.load(os.path.join(GOLDEN, 'reward_mix.npz'))
    B = int(z['B'])
    gts = [np.ones((2, 6), dtype=np.int64)] * B
    gen, greedy = torch.from_numpy(z['seq']).to(DEV), torch.from_numpy(z['greedy']).to(DEV)
    R.reset_scorer()
    R.CiderD_scorer = stub = _stub_scorer(z)
    try:
        for i, (cw, bw) in enumerate(z['pairs']):
            opt = argparse.Namespace(cider_reward_weight=float(cw), bleu_reward_weight=float(bw))
            del stub.calls[:]
            rew = R.get_self_critical_reward(greedy, gts, gen, opt)
            assert stub.calls == (['ciderd'] if cw > 0 else []) + ['bleu']           # a weight of 0 skips that scorer
            assert rew.dtype == np.float64 and rew.shape == z['seq'].shape
            np.testing.assert_allclose(rew, z['reward_%d' % i], rtol=0, atol=1e-15)
            np.testing.assert_allclose(R.get_scores(gts, gen, opt), z['scores_%d' % i], rtol=0, atol=1e-15)
            adv, _ = R.self_critical_reward_device(greedy, gts, gen, opt)
            assert adv.dtype == torch.float32
            np.testing.assert_allclose(adv.cpu().numpy(), z['reward_%d' % i][:, 0], rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(float(adv._capmi_mean), z['reward_%d' % i][:, 0].mean(), rtol=1e-5, atol=1e-7)
        np.testing.assert_array_equal(R.get_self_cider_scores(gts, gen, opt), z['self_cider'])
    finally:
        R.reset_scorer()


@pytest.mark.parametrize('red', ['mean', 'none'])
def test_structure_loss_call_site_matches_the_reference(red):
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    from imagecaptioning.pytorch_amd.captioning.utils import rewards as R
    z = np.load(os.path.join(GOLDEN, 'reward_mix.npz'))
    cw, bw, sw = (float(v) for v in z['struct_weights'])
    opt = argparse.Namespace(structure_loss_type='new_self_critical', train_sample_n=int(z['n']), entropy_reward_weight=0,
                             self_cider_reward_weight=sw, cider_reward_weight=cw, bleu_reward_weight=bw)
    R.reset_scorer()
    R.CiderD_scorer = stub = _stub_scorer(z)
    try:
        x = torch.log_softmax(torch.from_numpy(z['logits']).to(DEV), 2).requires_grad_(True)
        o = losses.StructureLosses(opt)(x, torch.from_numpy(z['seq']).to(DEV), [np.ones((2, 6), dtype=np.int64)] * int(z['B']),
                                        reduction=red)
        assert stub.calls == ['ciderd', 'bleu', 'self_cider']
        assert o['reward'].dtype == torch.float32 and o['reward'].shape == z['struct_%s_reward' % red].shape
        # float32 rounding of the fixture's values
        np.testing.assert_allclose(o['reward'].cpu().numpy(), z['struct_%s_reward' % red], rtol=2e-7, atol=0)
        np.testing.assert_allclose(o['loss'].detach().cpu().numpy(), z['struct_%s_loss' % red], rtol=1e-5, atol=1e-6)
        loss = o['loss']
        (loss if red == 'mean' else (loss * torch.linspace(0.5, 1.5, loss.numel(), device=DEV).view_as(loss)).sum()).backward()
        np.testing.assert_allclose(x.grad.cpu().numpy(), z['struct_%s_grad' % red], rtol=1e-5, atol=1e-7)
    finally:
        R.reset_scorer()


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _tiny_step(opt, sc_flag, struc_flag, fuse=True):
    """one LossWrapper step on a tiny UpDown; returns (out, what the criterion was given, gts, df, ref_len).  The first reference
    of every image is what the untrained model decodes greedily (the second, that with two words changed), so that 4-grams match
    and BLEU-4 is of order 1 for some rows, not 1e-6 for all."""
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules import loss_wrapper
    from imagecaptioning.pytorch_amd.captioning.utils import rewards
    torch.manual_seed(3)
    model = models.setup(opt).to(DEV)
    model.flatten_parameters_()
    lw = loss_wrapper.LossWrapper(model, opt)
    lw.fuse_scst_rollouts = fuse
    B, L = 4, 8
    rng = np.random.default_rng(0)
    ref_sets = [synthetic.zipf_rows(rng, 3, L, vocab=30, min_len=3) for _ in range(60)]
    df, ref_len = synthetic.document_frequency(ref_sets)
    rewards.reset_scorer()
    rewards.init_scorer((df, ref_len), device=torch.device(DEV))
    g = torch.Generator().manual_seed(1)
    fc = torch.randn(B, 20, generator=g).clamp_min(0).to(DEV)
    att = torch.randn(B, 6, 20, generator=g).clamp_min(0).to(DEV)
    model.eval()
    with torch.no_grad():
        decoded = model(fc, att, None, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')[0].cpu().numpy()
    model.train()
    gts = []
    for i in range(B):
        near = decoded[i].copy()
        near[[1, 4]] = [1 + (near[1] % 29), 1 + (near[4] % 29)]
        gts.append(np.stack([decoded[i], near, np.asarray(ref_sets[i][0], dtype=np.int64)]))
    seen = {}
    crit = lw.rl_crit if sc_flag else lw.struc_crit
    crit.register_forward_pre_hook(lambda mod, args: seen.update(input=args[0].detach().clone(), seq=args[1].detach().clone()))
    if sc_flag:
        real = loss_wrapper.self_critical_reward_device

        def spy(greedy_res, data_gts, gen_result, o):
            seen['greedy'] = greedy_res.detach().clone()
            return real(greedy_res, data_gts, gen_result, o)
        loss_wrapper.self_critical_reward_device = spy
    try:
        out = lw(fc, att, None, None, None, gts, torch.arange(B), sc_flag, struc_flag, False)
        out['loss'].backward()
    finally:
        if sc_flag:
            loss_wrapper.self_critical_reward_device = real
        rewards.reset_scorer()
    assert torch.isfinite(out['loss'])
    return out, seen, gts, df, ref_len


def _selected(seen):
    """(the log-probs of the sampled tokens [N, L] float64, the sampled rows) from what the criterion was given"""
    seq = seen['seq'].cpu().numpy()
    return seen['input'].double().gather(2, seen['seq'].unsqueeze(2)).squeeze(2).cpu().numpy(), seq


@pytest.mark.parametrize('fuse', [True, False])
def test_scst_step_with_a_bleu_weight(fuse):
    opt = tiny_opt(drop_prob_lm=0.5, cider_reward_weight=1.0, bleu_reward_weight=0.5)
    out, seen, gts, df, ref_len = _tiny_step(opt, True, False, fuse=fuse)
    sel, seq = _selected(seen)
    greedy = seen['greedy'].cpu().numpy()
    N, B, n = seq.shape[0], len(gts), seq.shape[0] // len(gts)
    oracle = OC.CiderD(df, ref_len)
    _, cider = OC.self_critical_reward(oracle, greedy, gts, seq)
    bleu = np.array([W.bleu4(seq[r], gts[r // n]) for r in range(N)] + [W.bleu4(greedy[i], gts[i]) for i in range(B)])
    reward = W.self_critical_reward(1.0, 0.5, cider, bleu, B, seq.shape[1])
    assert np.abs(bleu).max() > 0.5 and np.abs(reward).max() > 1e-3            # the BLEU term carries weight in this loss
    mask = np.concatenate([np.ones((N, 1)), (seq[:, :-1] > 0).astype(np.float64)], 1)
    want = (-sel * reward * mask).sum() / mask.sum()
    assert float(out['loss'].detach()) == pytest.approx(want, rel=1e-5)
    assert float(out['reward']) == pytest.approx(reward[:, 0].mean(), rel=1e-5, abs=1e-7)


def test_new_self_critical_step_with_both_weights():
    opt = tiny_opt(drop_prob_lm=0.5, structure_loss_type='new_self_critical', structure_loss_weight=1.0, entropy_reward_weight=0,
                   cider_reward_weight=1.0, bleu_reward_weight=0.5, self_cider_reward_weight=0.1)
    out, seen, gts, df, ref_len = _tiny_step(opt, False, True)
    sel, seq = _selected(seen)
    N, n = seq.shape[0], opt.train_sample_n
    cider = OC.sample_scores(OC.CiderD(df, ref_len), gts, seq)
    bleu = np.array([W.bleu4(seq[r], gts[r // n]) for r in range(N)])
    scores = W.mix(1.0, 0.5, cider, bleu)
    selfc = W.self_cider_scores(seq, n, df, ref_len)
    assert selfc.max() > 1e-3
    want = W.nsc_loss(sel, seq, W.nsc_weights(scores, n, selfc, 0.1))
    assert float(out['loss'].detach()) == pytest.approx(want, rel=1e-5)
    np.testing.assert_allclose(out['reward'].cpu().numpy(), scores.reshape(-1, n), rtol=1e-6, atol=1e-7)


# ---- unchanged default -------------------------------------------------------------------------------------------------------
def test_default_weights_take_the_path_they_took():
    from imagecaptioning.pytorch_amd.captioning.utils import rewards as R
    gts, hyp = _bleu_case(20, 2)
    R.reset_scorer()
    sc = R.init_scorer((DF, REF_LEN), device=torch.device(DEV))
    try:
        packed = R.pack_gts(gts)
        gen = torch.from_numpy(hyp).to(DEV)
        greedy = torch.from_numpy(hyp[::2].copy()).to(DEV)
        opt = argparse.Namespace(cider_reward_weight=1.0, bleu_reward_weight=0.0, self_cider_reward_weight=0.0)
        refs, n_refs = packed.packed
        adv0, s0 = sc.self_critical_reward(greedy, gen, refs, n_refs, 2, cooked=packed.packed.cooked)
        adv, s = R.self_critical_reward_device(greedy, packed, gen, opt)
        assert torch.equal(adv, adv0) and torch.equal(s, s0) and torch.equal(adv._capmi_mean, adv0._capmi_mean)
        img = (torch.arange(gen.shape[0], device=DEV) // 2).to(torch.int32)
        assert torch.equal(R.get_scores(packed, gen, opt, as_tensor=True), sc.score(gen, img, refs, n_refs, packed.packed.cooked) * 1.0)
    finally:
        R.reset_scorer()


# ---- captured step -----------------------------------------------------------------------------------------------------------
def test_captured_step_with_both_rewards_is_the_stepped_step_bit_for_bit():
    from imagecaptioning.pytorch_amd.graph_step import TrainStep
    from test_graph_step_gpu import _batches, _setup
    runs, its = {}, 6
    for mode in ('stepped', 'graph'):
        opt, model, flat, lw, dims = _setup('aoa')
        opt.bleu_reward_weight, opt.self_cider_reward_weight = 0.5, 0.1
        assert lw.struc_crit.opt is opt and opt.structure_loss_type == 'new_self_critical'
        batches = _batches('aoa', dims)
        ts = TrainStep(lw, flat, opt, DEV, graph=(mode == 'graph'))
        losses = [ts(batches[it % len(batches)], False, True, lr=1e-3)[0].clone() for it in range(its)]
        torch.cuda.synchronize()
        if mode == 'graph':
            assert ts.failed is None, ts.failed
            assert ts.captures == 1 and ts.replays == its - 1, (ts.captures, ts.replays, ts.stepped)
        runs[mode] = (torch.stack(losses).cpu(), flat.flat.clone().cpu())
    a, b = runs['stepped'], runs['graph']
    assert torch.isfinite(a[0]).all() and len(set(a[0].tolist())) > 3
    assert torch.equal(a[0], b[0]), (a[0], b[0])
    assert torch.equal(a[1], b[1])
