"""Consensus reranking on the MI355X (csrc/mbr.hip, imagecaptioning/pytorch_amd/mbr.py, CaptionModel.forward, tools/eval.py --rerank):
capmi_mbr_utility against capmi_ciderd_score / capmi_reward_bleu4 fed candidate j as the single reference and against the float64
restatement tests/mbr_ref64.py, capmi_mbr_select against the restatement, the refused arguments, the model API of three families and
the CLI.  Floats within 1e-10 absolute, the project's bar for its float64 metric kernels; choices exact, on
candidate sets whose two best distinct candidates the restatement holds more than 1e-6 apart."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import ciderd as OC

import mbr_ref64 as M
from test_model_api_gpu import DEV

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')
TOL = 1e-10
MARGIN = 1e-6

V = 12                          # word ids 1..11
# the documents of the table: 5 images, 2 captions each.  The end token and the word 1 are in every image (weight exactly 0), the
# words 9..11 and most longer n-grams of the candidates in none.  Five, because "exactly 0" is log_ref_len, the host's logarithm,
# minus the device's logarithm of the same count, and capmi_ciderd_score -- whose arithmetic CAPMI_MBR_CIDERD is -- does not snap a
# difference of one ulp to 0 (self-CIDEr does).  Where the two logarithms differ, the empty caption -- the word 0 alone, its only
# n-gram one of every image -- has a unigram norm of 1e-16 instead of 0 and scores 2.5 against itself, in capmi_ciderd_score and
# here alike, and 0 in the restatement.  Measured through capmi_ciderd_score on an MI355X for 2..64 images: the two agree for 2-5,
# 9-21, 23, 25-28, 30-33, 35-40, 46, 48, 52-57, 59 and 61-63 images and differ for the others (6, 7 and 8 among them).
DOCS = [[[1, 2, 3, 0], [1, 4, 0]], [[1, 2, 5, 6, 0], [2, 3, 0]], [[1, 7, 0], [1, 2, 3, 4, 0]], [[8, 1, 0], [1, 2, 0]],
        [[1, 5, 5, 0], [6, 1, 0]]]
DF, REF_LEN = OC.build_document_frequency(DOCS)
B = 3
NS, LS = (2, 5, 32), (1, 6, 64)
KINDS = {'ciderd': 'mbr_ciderd', 'bleu4': 'mbr_bleu4'}


def candidates(n, L):
    """[B * n, L]: image 0 holds the empty caption (n > 2 or L = 1), a completely filled row, two identical rows (n > 2) and
    variations of one sentence; image 1's candidates are all identical (n = 2: the empty caption); image 2's share no n-gram
    (filled rows of words of their own, no end token: the 0 would be a shared word), so its CIDEr-D utilities are all 0 and its
    BLEU-4 utilities all the same tiny number (bleu_scorer's 1e-15 in place of the matches)"""
    rng = np.random.default_rng(7 * n + L)
    rows = np.zeros((B * n, L), dtype=np.int64)
    base = rng.integers(1, V, size=L)
    for r in range(n):
        row = base.copy()
        flip = rng.random(L) < 0.35
        row[flip] = rng.integers(1, V, size=int(flip.sum()))
        ln = int(rng.integers(min(2, L), L + 1))
        row[ln:] = 0
        rows[r] = row
    rows[0] = base                                                        # completely filled: no end token
    if n > 2:
        rows[1] = 0                                                       # the empty caption
        rows[3] = rows[2]                                                 # two identical rows
    elif L == 1:
        rows[1] = 0
    else:
        # two candidates: U[0][1] and U[1][0] are all there is.  CIDEr-D tells them apart only where a count is clipped on one
        # side -- the word 9 (in no document) once in row 0, twice in row 1 --, BLEU-4 only by the lengths: row 1 is one shorter
        rows[0, 0] = 9
        rows[0, 1:][rows[0, 1:] == 9] = 10
        rows[1] = rows[0]
        rows[1, L - 3] = 9
        rows[1, L - 2:] = 0
    same = base.copy()
    same[L // 2 + 1:] = 0
    rows[n:2 * n] = 0 if n == 2 else same
    for r in range(n):
        rows[2 * n + r] = 100 + r
    return rows


def _table():
    tok = [t for img in DOCS for cap in img for t in cap]
    lens = [len(cap) for img in DOCS for cap in img]
    cap_off = np.concatenate([[0], np.cumsum(lens)])
    img_off = np.concatenate([[0], np.cumsum([len(img) for img in DOCS])])
    return np.array(tok, dtype=np.int64), cap_off, img_off


@pytest.fixture(scope='module')
def scorer():
    """the table built on the device by capmi_df_count / capmi_df_finalize"""
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD
    sc = DeviceCiderD.from_corpus(*_table(), torch.device(DEV))
    weights = {g: np.log(REF_LEN) - np.log(max(1.0, v)) for g, v in DF.items()}
    assert weights[(0,)] == 0 and weights[(1,)] == 0 and (9,) not in DF and REF_LEN == len(DOCS)
    return sc


_REF = {}


def reference(n, L, kind):
    """the restatement of a case, computed once: (rows, U, seq_weight, {prior: (expected, choice)})"""
    key = (n, L, kind)
    if key not in _REF:
        rows = candidates(n, L)
        wt = np.random.default_rng(1000 + 7 * n + L).normal(size=B * n) * 2.0
        U = np.stack([M.utility(rows[g * n:(g + 1) * n], kind, DF, REF_LEN) for g in range(B)])
        sel = {}
        for prior, w in (('uniform', None), ('model', wt)):
            out = [M.select(U[g], rows[g * n:(g + 1) * n], None if w is None else w[g * n:(g + 1) * n]) for g in range(B)]
            sel[prior] = (np.stack([e for e, _ in out]), np.array([c for _, c in out]))
        for a in (rows, U, wt):
            a.setflags(write=False)
        _REF[key] = (rows, U, wt, sel)
    return _REF[key]


def _single_refs(rows, n, j, L):
    """candidate j of every image as that image's only reference: int32 [B, 1, w], w = L + 1 padded with -1 (at L = 64 a row is as
    wide as a reference can be, and a filled one needs no marker: the width itself ends it)"""
    w = min(L + 1, 64)
    refs = np.full((B, 1, w), -1, dtype=np.int32)
    refs[:, 0, :L] = rows[j::n][:B]
    return torch.from_numpy(refs).to(DEV), torch.ones(B, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('kind', sorted(KINDS))
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('n', NS)
def test_utility_matches_the_rewards_and_the_restatement(scorer, n, L, kind):
    from imagecaptioning.pytorch_amd import mbr
    rows, want, _, _ = reference(n, L, kind)
    lens = [len(OC.tokens_of(r)) for r in rows]
    assert lens[0] == L and (1 in lens[:n] or n == 2) and (n == 2 or np.array_equal(rows[2], rows[3]))
    assert all(np.array_equal(rows[n], rows[n + r]) for r in range(n))
    off = ~np.eye(n, dtype=bool)
    assert not want[2][off].any() if kind == 'ciderd' else np.ptp(want[2][off]) == 0        # no shared n-gram
    seq = torch.tensor(rows, device=DEV)
    U = mbr.utility(seq, n, KINDS[kind], scorer)
    assert U.shape == (B, n, n) and U.dtype == torch.float64
    assert torch.equal(mbr.utility(seq, n, KINDS[kind], scorer), U)                          # run to run: the same bits
    got = U.cpu().numpy()
    img = (torch.arange(B * n, device=DEV) // n).to(torch.int32)
    col = np.zeros_like(got)
    for j in range(n):
        refs, n_refs = _single_refs(rows, n, j, L)
        s = scorer.score(seq, img, refs, n_refs) if kind == 'ciderd' else scorer.bleu4(seq, img, (refs, n_refs), 0.0, 1.0)
        col[:, :, j] = s.cpu().numpy().reshape(B, n)
    d_reward, d_ref = float(np.abs(got - col).max()), float(np.abs(got - want).max())
    print('utility %s n = %d L = %d: |U - reward| %.3e, |U - ref64| %.3e' % (kind, n, L, d_reward, d_ref))
    assert d_reward <= TOL and d_ref <= TOL


@pytest.mark.parametrize('kind', sorted(KINDS))
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('n', NS)
def test_select_matches_the_restatement(scorer, n, L, kind):
    from imagecaptioning.pytorch_amd import mbr
    rows, _, wt, sel = reference(n, L, kind)
    seq = torch.tensor(rows, device=DEV)
    U = mbr.utility(seq, n, KINDS[kind], scorer)
    for prior in ('uniform', 'model'):
        want_e, want_c = sel[prior]
        # the condition of an exact choice, on the restatement: image 0's two best distinct candidates are apart.  (n = 2, L = 1
        # leaves two one-word captions: they share nothing and their two values are one number, an exact tie.)  Images 1 and 2
        # are the deliberate ones: all identical -- candidate 0 is the only first occurrence -- and nothing shared, where every
        # expected value is the same number and the lowest index wins.  Only BLEU-4's nothing-shared image under the model prior
        # is held to no choice: its expected values are weighted means of one tiny number and differ by their rounding alone.
        tie = n == 2 and L == 1 and want_e[0][0] == want_e[0][1]
        assert M.margin(want_e[0], rows[:n]) > MARGIN or tie
        exact = [True, True, kind == 'ciderd' or prior == 'uniform']
        assert want_c[1] == 0 and (want_c[2] == 0 or not exact[2])
        assert np.ptp(want_e[2]) <= (0 if exact[2] else 8 * 2.0 ** -52 * want_e[2].max())
        e, c = mbr.select(U, seq, n, torch.tensor(wt, device=DEV) if prior == 'model' else None)
        assert c.dtype == torch.int32 and e.dtype == torch.float64
        e2, c2 = mbr.select(U, seq, n, torch.tensor(wt, device=DEV) if prior == 'model' else None)
        assert torch.equal(e, e2) and torch.equal(c, c2)
        dev = float(np.abs(e.cpu().numpy() - want_e).max())
        print('select %s %s n = %d L = %d: |expected - ref64| %.3e' % (kind, prior, n, L, dev))
        assert dev <= TOL
        got_c = c.cpu().tolist()
        assert [got_c[g] for g in range(B) if exact[g]] == [int(want_c[g]) for g in range(B) if exact[g]]
        assert 0 <= got_c[2] < n


def test_a_duplicate_of_the_winner_is_never_returned(scorer):
    from imagecaptioning.pytorch_amd import mbr
    rows = np.array([[2, 3, 0, 0], [1, 2, 3, 0], [5, 0, 0, 0], [1, 2, 3, 0], [1, 2, 4, 0], [1, 2, 3, 0]], dtype=np.int64)
    seq = torch.from_numpy(np.concatenate([rows, rows[::-1]])).to(DEV)
    for kind in sorted(KINDS):
        want = [M.select(M.utility(r, kind, DF, REF_LEN), r)[1] for r in (rows, rows[::-1])]
        assert want == [1, 0]                                             # the first of the three [1 2 3 0] on either side
        e, c = mbr.select(mbr.utility(seq, 6, KINDS[kind], scorer), seq, 6)
        assert c.cpu().tolist() == want
        e = e.cpu().numpy()
        assert abs(e[0, 1] - e[0, 3]) <= 1e-12 and abs(e[0, 1] - e[0, 5]) <= 1e-12


def test_bad_arguments_return_einval_and_launch_nothing(scorer):
    from imagecaptioning.pytorch_amd import _lib
    from imagecaptioning.pytorch_amd._lib import lib, ptr
    n, L = 3, 6
    seq = torch.from_numpy(candidates(n, L)).to(DEV)
    scratch = torch.zeros(B * n * _lib.CIDERD_COOKED_BYTES // 8, dtype=torch.int64, device=DEV)
    U = torch.full((B, n, n), -7.0, dtype=torch.float64, device=DEV)
    e = torch.full((B, n), -7.0, dtype=torch.float64, device=DEV)
    c = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    k, v, cap, lr = ptr(scorer.keys), ptr(scorer.vals), scorer.cap, scorer.log_ref_len

    def utility(hyp=ptr(seq), B_=B, n_=n, L_=L, kind=_lib.MBR_CIDERD, keys=k, vals=v, cap_=cap, scr=ptr(scratch), out=ptr(U)):
        return lib.capmi_mbr_utility(hyp, B_, n_, L_, kind, keys, vals, cap_, lr, scr, out, None)

    def select(u=ptr(U), hyp=ptr(seq), B_=B, n_=n, L_=L, ex=ptr(e), ch=ptr(c)):
        return lib.capmi_mbr_select(u, None, hyp, B_, n_, L_, ex, ch, None)

    bad = [utility(hyp=None), utility(scr=None), utility(out=None), utility(keys=None), utility(vals=None), utility(n_=1),
           utility(n_=33), utility(L_=65), utility(L_=0), utility(B_=0), utility(cap_=cap - 1), utility(cap_=0), utility(kind=2),
           utility(kind=_lib.MBR_BLEU4, n_=1), utility(kind=_lib.MBR_BLEU4, L_=65), utility(scr=ptr(scratch) + 4),
           select(u=None), select(hyp=None), select(ex=None), select(ch=None), select(n_=1), select(n_=33), select(L_=65),
           select(B_=0)]
    assert bad == [_lib.EINVAL] * len(bad)
    torch.cuda.synchronize()
    assert bool((U == -7).all()) and bool((e == -7).all()) and bool((c == -7).all()) and not scratch.any()
    # BLEU-4 takes no table
    assert utility(kind=_lib.MBR_BLEU4, keys=None, vals=None, cap_=0) == 0 and select() == 0
    torch.cuda.synchronize()
    assert bool((U != -7).all()) and bool((c >= 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the model API
# ---------------------------------------------------------------------------------------------------------------------------
def _model(name):
    from test_ensemble_gpu import family_model, ensemble
    return ensemble(['updown', 'att2in2']) if name == 'ensemble' else family_model(name)


def _sample(model, inputs, **opt):
    """one sample call under a fixed seed: the draws depend on torch's seed and on the model's own count of calls"""
    fc, att, am = inputs
    torch.manual_seed(11)
    for m in [model] + list(getattr(model, 'models', [])):
        m._rng_calls = 0
    with torch.no_grad():
        return model(fc, att, am, opt=opt, mode='sample')


@pytest.mark.parametrize('name', ('updown', 'transformer', 'ensemble'))
def test_model_api_returns_the_chosen_rows(name):
    from test_ensemble_gpu import inputs
    model = _model(name)
    inp = inputs()[:3]
    Bm, n = inp[0].shape[0], 4
    trace = {'return_attention': 1} if name == 'updown' else {}
    base = dict(sample_method='sample', sample_n=n, temperature=1.5, **trace)
    seq0, logp0 = _sample(model, inp, **base)
    att0 = model.last_attention['att'] if trace else None
    assert seq0.shape[0] == Bm * n and model.last_rerank is None
    for kind, prior in (('mbr_bleu4', 'uniform'), ('mbr_bleu4', 'model')):
        seq, logp = _sample(model, inp, rerank=kind, rerank_prior=prior, **base)
        last = model.last_rerank
        assert sorted(last) == ['candidate_logp_sum', 'candidates', 'choice', 'expected', 'utility']
        assert torch.equal(last['candidates'], seq0)
        rows = torch.arange(Bm, device=DEV) * n + last['choice'].long()
        assert seq.shape == (Bm, seq0.shape[1]) and logp.shape == (Bm,) + tuple(logp0.shape[1:])
        assert torch.equal(seq, seq0[rows]) and torch.equal(logp, logp0[rows])
        if trace:
            assert sorted(model.last_attention) == ['att', 'entropy', 'top', 'top_w']
            assert torch.equal(model.last_attention['att'], att0[rows]) and model.last_attention['top'].shape[0] == Bm
        # the choice is the restatement's, fed the call's own candidates and log-probs
        cand = seq0.cpu().numpy()
        sums = M.seq_weight(logp0.gather(2, seq0.unsqueeze(2)).squeeze(2).double().cpu().numpy(), cand)
        assert float(np.abs(last['candidate_logp_sum'].cpu().numpy() - sums).max()) <= 1e-9
        U, e, c = M.rerank(cand, n, 'bleu4', weight=sums if prior == 'model' else None)
        assert float(np.abs(last['utility'].cpu().numpy() - U).max()) <= TOL
        assert float(np.abs(last['expected'].cpu().numpy() - e).max()) <= TOL
        if all(M.margin(e[g], cand[g * n:(g + 1) * n]) > MARGIN for g in range(Bm)):
            assert last['choice'].cpu().tolist() == c.tolist()
    # the option off after it was on: what it was before, and no reranking left behind
    seq1, logp1 = _sample(model, inp, **base)
    assert torch.equal(seq1, seq0) and torch.equal(logp1, logp0) and model.last_rerank is None
    seq2, _ = _sample(model, inp, rerank='', **base)
    assert torch.equal(seq2, seq0) and model.last_rerank is None


def test_beam_candidates_with_the_model_prior(scorer):
    from test_ensemble_gpu import inputs
    from imagecaptioning.pytorch_amd.captioning.utils import rewards
    model = _model('updown')
    inp = inputs()[:3]
    Bm, n = inp[0].shape[0], 3
    base = dict(sample_method='beam_search', beam_size=n, sample_n=n)
    seq0, logp0 = _sample(model, inp, **base)
    assert seq0.shape[0] == Bm * n
    rewards.reset_scorer()
    try:
        rewards.CiderD_scorer = scorer
        seq, logp = _sample(model, inp, rerank='mbr_ciderd', rerank_prior='model', **base)
    finally:
        rewards.reset_scorer()
    last = model.last_rerank
    assert torch.equal(last['candidates'], seq0)
    cand = seq0.cpu().numpy()
    sums = M.seq_weight(logp0.gather(2, seq0.unsqueeze(2)).squeeze(2).double().cpu().numpy(), cand)      # the beams' own log-probs
    U, e, c = M.rerank(cand, n, 'ciderd', DF, REF_LEN, sums)
    assert float(np.abs(last['utility'].cpu().numpy() - U).max()) <= TOL
    assert float(np.abs(last['expected'].cpu().numpy() - e).max()) <= 1e-9       # the sums are float32 log-probs added in float64
    if all(M.margin(e[g], cand[g * n:(g + 1) * n]) > MARGIN for g in range(Bm)):
        assert last['choice'].cpu().tolist() == c.tolist()
    rows = torch.arange(Bm, device=DEV) * n + last['choice'].long()
    assert torch.equal(seq, seq0[rows]) and torch.equal(logp, logp0[rows])


# ---------------------------------------------------------------------------------------------------------------------------
# tools/eval.py --rerank
# ---------------------------------------------------------------------------------------------------------------------------
def test_eval_entrypoint_reranks(tmp_path):
    from test_langeval_gpu import SMALL, _opts
    sys.path.insert(0, PKG)
    from imagecaptioning.pytorch_amd.tools import eval as E
    common = SMALL + ['--num_images', '4', '--sample_n', '3', '--sample_n_method', 'sample', '--split', 'val', '--language_eval', '1']

    def run(name, extra):
        out_dir = tmp_path / name
        res = E.main(_opts(common + ['--eval_results_dir', str(out_dir)] + extra))
        return res, out_dir

    (loss, preds, stats), out_dir = run('mbr', ['--rerank', 'mbr_bleu4'])
    assert sorted(os.listdir(out_dir)) == ['capmi_val.json', 'capmi_val_mbr.npz']            # no _n.json: one caption per image
    assert len(preds) == 4 and all(np.isfinite(v) for v in stats.values())
    z = np.load(out_dir / 'capmi_val_mbr.npz')
    assert z['choice'].shape == (4,) and z['expected'].shape == (4, 3) and z['candidates'].shape == (4, 3, 6)
    assert [p['image_id'] for p in preds] == z['image_id'].tolist()
    from captioning.utils import misc
    loader, vocab = E.build_loader(_opts(common), torch.device(DEV))
    for i, p in enumerate(preds):
        assert p['mbr_choice'] == int(z['choice'][i]) and 0 <= p['mbr_choice'] < 3
        assert p['mbr_expected'] == float(z['expected'][i, p['mbr_choice']])
        e, c = M.select(M.utility(z['candidates'][i], 'bleu4'), z['candidates'][i])
        assert float(np.abs(e - z['expected'][i]).max()) <= TOL
        if M.margin(e, z['candidates'][i]) > MARGIN:
            assert c == p['mbr_choice']
        chosen = torch.from_numpy(z['candidates'][i, p['mbr_choice']][None])
        assert p['caption'] == misc.decode_sequence(vocab, chosen)[0]
    written = json.load(open(out_dir / 'capmi_val.json'))
    assert {v['caption'] for v in written['imgToEval'].values()} <= {p['caption'] for p in preds}
    # without the flag: what the command writes today -- the three files of a sample_n run, no reranking keys
    (_, preds0, _), out0 = run('plain', [])
    assert sorted(os.listdir(out0)) == ['capmi_val.json', 'capmi_val_n.json']
    assert all('mbr_choice' not in p and 'mbr_expected' not in p for p in preds0)
    (_, preds1, _), out1 = run('plain_again', ['--rerank', ''])
    assert preds1 == preds0
    for f in ('capmi_val.json', 'capmi_val_n.json'):
        assert open(out0 / f, 'rb').read() == open(out1 / f, 'rb').read()
