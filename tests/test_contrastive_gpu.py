"""Contrastive search (sample_method 'contrastive') on a real MI355X: capmi_contrastive_topk / capmi_contrastive_select against float64
numpy on every arm, the five supported families (AoA at out_res 0) end to end against the float64 replay (tests/contrastive_ref64.py) over their float64
single steps, greedy equivalence, decode-time constraints and the command line."""
import argparse
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import contrastive_ref64 as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _lib():
    from imagecaptioning.pytorch_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ the top-k kernel
@pytest.mark.parametrize('V1,k', [(31, 1), (31, 4), (33, 32), (9488, 5), (1029, 32)])
def test_topk_orders_by_value_then_id_and_counts_minus_infinity_as_a_value(V1, k):
    L = _lib()
    g = torch.Generator().manual_seed(V1 + k)
    N = 5
    x = torch.log_softmax(torch.randn(N, V1, generator=g) * 2, 1)
    x[1, 7] = x[1, 3] = x[1].max() + 0.5                       # a tie at the top: 3 before 7
    x[2, :] = float('-inf')
    x[2, V1 - 2] = -0.1                                        # one finite entry: the rest are the lowest-numbered -inf columns
    x[3, 5:] = float('-inf')                                   # five finite entries
    x[4] = x[4].round(decimals=1)                              # many ties
    ld = V1 + 3                                                # rows off the 16-byte grid
    buf = torch.full((N, ld), float('nan'), device=DEV)
    buf[:, :V1] = x.to(DEV)
    unf = torch.tensor([1, 1, 0, 1, 1], dtype=torch.uint8, device=DEV)
    tok = torch.full((N, k), -1, dtype=torch.long, device=DEV)
    lp = torch.full((N, k), 7.0, device=DEV)
    store = torch.full((N, 2, V1), 7.0, device=DEV)            # column t = 1 of a [N, 2, V1] seqLogprobs
    L.check(L.lib.capmi_contrastive_topk(buf.data_ptr(), ld, N, V1, k, unf.data_ptr(), tok.data_ptr(), lp.data_ptr(),
                                         store.data_ptr() + 4 * V1, 2 * V1, L.stream_ptr()), 'capmi_contrastive_topk')
    torch.cuda.synchronize()
    srt, ids = torch.sort(x.double(), dim=1, descending=True, stable=True)
    assert torch.equal(tok.cpu(), ids[:, :k])
    assert torch.equal(lp.cpu().double(), srt[:, :k])          # the values are copies
    assert tok[1, 0].item() == 3 and (k == 1 or tok[1, 1].item() == 7)
    if k > 1:
        assert tok[2].tolist() == [V1 - 2] + list(range(k - 1))
    got = store.cpu()
    assert bool((got[:, 0] == 7.0).all())
    for r in (0, 1, 3, 4):
        assert torch.equal(got[r, 1], x[r])
    assert bool(torch.isnan(got[2, 1, 0])) and got[2, 1, V1 - 2].item() == 0.0      # finished: logp * 0, -inf * 0 = NaN


def test_entry_points_refuse_what_the_header_rules_out():
    L = _lib()
    N, k, R_, S, L_ = 2, 3, 8, 5, 4
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)       # noqa: E731
    logp, tok, lp = z(N, 16), z(N, k, dt=torch.long), z(N, k)
    g, hist, inv = z(N * k, R_), z(N, S, R_), z(N, S)
    ch, par, fan = z(N, dt=torch.int32), z(N, dt=torch.int32), z(N, k, dt=torch.int32)
    seq, it, unf = z(N, L_, dt=torch.long), z(N, dt=torch.long), torch.ones(N, dtype=torch.uint8, device=DEV)

    def topk(**kw):
        a = dict(ld=16, N=N, V1=16, k=k)
        a.update(kw)
        return L.lib.capmi_contrastive_topk(logp.data_ptr(), a['ld'], a['N'], a['V1'], a['k'], unf.data_ptr(), tok.data_ptr(), lp.data_ptr(),
                                            None, 0, L.stream_ptr())

    def select(**kw):
        a = dict(ld=R_, k=k, R=R_, S=S, hl=1, t=0, L=L_, alpha=0.5, hist=hist.data_ptr())
        a.update(kw)
        return L.lib.capmi_contrastive_select(tok.data_ptr(), lp.data_ptr(), g.data_ptr(), a['ld'], a['hist'], inv.data_ptr(), N, a['k'],
                                              a['R'], a['S'], a['hl'], a['t'], a['L'], a['alpha'], ch.data_ptr(), par.data_ptr(),
                                              fan.data_ptr(), seq.data_ptr(), L_, it.data_ptr(), unf.data_ptr(), L.stream_ptr())
    for bad in (dict(k=0), dict(k=33), dict(k=17), dict(ld=15), dict(V1=0)):
        assert topk(**bad) == L.EINVAL, bad
    for bad in (dict(k=0), dict(k=33), dict(R=0), dict(ld=R_ - 1), dict(S=L_), dict(hl=S), dict(hl=-1), dict(t=L_), dict(t=-1),
                dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float('nan')), dict(hist=g.data_ptr())):
        assert select(**bad) == L.EINVAL, bad
    assert topk() == 0 and select() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the select kernel
N3 = 3


def _draw(seed, k, S, R_, ld, alpha, rows):
    """One launch's inputs (float32 values) for 3 rows of the kinds named in `rows`: 'plain', 'finished', 'zero' (candidate min(1, k - 1)
    is a zero vector), 'tail' (the last two candidates -- all but the first for k < 3 -- have p = 0) and 'none' (all have p = 0).
    Candidate j leans on a history row with a weight of its own, so that the cosines spread over (0, 1) at every R."""
    g = np.random.default_rng(seed)
    hist = g.standard_normal((N3, S, R_)).astype(np.float32)
    lean = g.uniform(0.0, 1.0, (N3, k, 1)).astype(np.float32)
    src = hist[np.arange(N3)[:, None], g.integers(0, S, (N3, k))]
    cand = np.zeros((N3, k, ld), np.float32)
    cand[:, :, :R_] = lean * src + (1 - lean) * g.standard_normal((N3, k, R_)).astype(np.float32)
    cand[:, :, R_:] = np.nan                                                        # the padding of ld > R is never read
    p = np.sort(g.dirichlet(np.ones(k + 3), N3)[:, :k], 1)[:, ::-1]
    lp = np.log(p).astype(np.float32)
    tok = np.stack([g.permutation(40)[:k] + 1 for _ in range(N3)]).astype(np.int64)
    tok[1, 0] = 0                                                                   # a row may pick the end token
    unf = np.ones(N3, bool)
    for i, kind in enumerate(rows):
        if kind == 'finished':
            unf[i] = False
        elif kind == 'zero':
            cand[i, min(1, k - 1), :R_] = 0.0
        elif kind == 'tail':
            lp[i, max(1, k - 2):] = -np.inf
        elif kind == 'none':
            lp[i, :] = -np.inf
    return tok, lp, cand, hist, unf


def _case(k, S, R_, ld, alpha, rows, base):
    """the first draw whose float64 score gap is at least 1e-3 in every row (a condition on the inputs)"""
    for s in range(200):
        tok, lp, cand, hist, unf = _draw(base + s, k, S, R_, ld, alpha, rows)
        ref = R.select(tok, lp, cand[:, :, :R_], hist, alpha, unf)
        if float(ref['gap'].min()) >= 1e-3:
            return tok, lp, cand, hist, unf, ref
    raise AssertionError('no draw separates the scores')


def _launch(tok, lp, cand, hist, unf, k, S, R_, ld, alpha, t, L_, S_max):
    L = _lib()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)               # noqa: E731
    hbuf = torch.full((N3, S_max, R_), float('nan'), device=DEV)
    hbuf[:, :S] = d(hist)
    inv = torch.full((N3, S_max), float('nan'), device=DEV)
    inv[:, :S] = d((1.0 / np.sqrt((hist.astype(np.float64) ** 2).sum(2))).astype(np.float32))
    tok_d, lp_d, cand_d, unf_d = d(tok), d(lp), d(cand.reshape(N3 * k, ld)), d(unf.astype(np.uint8))
    choice = torch.full((N3,), -1, dtype=torch.int32, device=DEV)
    parent, fan = torch.full_like(choice, -1), torch.full((N3, k), -1, dtype=torch.int32, device=DEV)
    seq = torch.full((N3, L_), -1, dtype=torch.long, device=DEV)
    it = torch.full((N3,), -1, dtype=torch.long, device=DEV)
    L.check(L.lib.capmi_contrastive_select(tok_d.data_ptr(), lp_d.data_ptr(), cand_d.data_ptr(), ld, hbuf.data_ptr(), inv.data_ptr(), N3, k,
                                           R_, S_max, S, t, L_, alpha, choice.data_ptr(), parent.data_ptr(), fan.data_ptr(),
                                           seq.data_ptr(), L_, it.data_ptr(), unf_d.data_ptr(), L.stream_ptr()), 'capmi_contrastive_select')
    torch.cuda.synchronize()
    return dict(choice=choice.cpu().numpy(), parent=parent.cpu().numpy(), fan=fan.cpu().numpy(), seq=seq.cpu().numpy(),
                it=it.cpu().numpy(), unf=unf_d.cpu().numpy(), hist=hbuf.cpu().numpy(), inv=inv.cpu().numpy())


ROW_SETS = (('finished', 'zero', 'tail'), ('plain', 'none', 'plain'))


@pytest.mark.parametrize('R_', [16, 18, 1000, 1028])
def test_select_kernel_against_float64(R_):
    """N = 3, k in {1, 2, 5, 32}, history length in {1, 7, 21}, alpha in {0, 0.6, 1}; R = 18 takes the element-by-element arm, the others
    the 16-byte one; the second row set runs with ld = R + 4 > R.  Index outputs exact, the appended row within rtol 1e-6 (a copy),
    and its inverse norm within the same 1e-6: the kernel sums |g|^2 in double, so the stored float is the rounding of a value good
    to 1e-15, one float ulp (6e-8) away at most."""
    L_, S_max, t = 24, 25, 21
    n = 0
    for k in (1, 2, 5, 32):
        for S in (1, 7, 21):
            for alpha in (0.0, 0.6, 1.0):
                for rs, rows in enumerate(ROW_SETS):
                    ld = R_ + 4 * rs
                    tok, lp, cand, hist, unf, ref = _case(k, S, R_, ld, alpha, rows, 1000 * R_ + 97 * n)
                    n += 1
                    assert float(ref['gap'].min()) >= 1e-3                       # on the float64 scores alone
                    got = _launch(tok, lp, cand, hist, unf, k, S, R_, ld, alpha, t, L_, S_max)
                    tag = (R_, k, S, alpha, rows)
                    assert np.array_equal(got['choice'], ref['choice']), tag
                    assert np.array_equal(got['parent'], ref['parent']), tag
                    assert np.array_equal(got['fan'], np.repeat(ref['choice'][:, None], k, 1)), tag
                    assert np.array_equal(got['seq'][:, t], ref['token']) and np.array_equal(got['it'], ref['token']), tag
                    assert bool((np.delete(got['seq'], t, 1) == -1).all()), tag
                    assert np.array_equal(got['unf'].astype(bool), ref['unfinished']), tag
                    np.testing.assert_allclose(got['hist'][:, S], ref['row'], rtol=1e-6, atol=0, err_msg=str(tag))
                    np.testing.assert_allclose(got['inv'][:, S], ref['inv'], rtol=1e-6, err_msg=str(tag))
                    assert np.array_equal(got['hist'][:, :S], hist) and bool(np.isnan(got['hist'][:, S + 1:]).all()), tag
                    if 'none' in rows:
                        assert got['choice'][1] == 0


def test_select_files_the_bos_row_with_an_empty_history():
    """k = 1, hist_len = 0, no token tables: the call that starts a decode -- row 0 of the history and its inverse norm, nothing else"""
    L = _lib()
    R_, S_max, L_ = 18, 4, 3
    h = torch.randn(N3, R_, generator=torch.Generator().manual_seed(3))
    h[1] = 0
    hd = h.to(DEV)
    hist = torch.full((N3, S_max, R_), float('nan'), device=DEV)
    inv = torch.full((N3, S_max), float('nan'), device=DEV)
    L.check(L.lib.capmi_contrastive_select(None, None, hd.data_ptr(), R_, hist.data_ptr(), inv.data_ptr(), N3, 1, R_, S_max, 0, 0, L_, 0.6,
                                           None, None, None, None, L_, None, None, L.stream_ptr()), 'capmi_contrastive_select')
    torch.cuda.synchronize()
    assert torch.equal(hist[:, 0].cpu(), h) and bool(torch.isnan(hist[:, 1:]).all())
    want = 1.0 / h.double().norm(dim=1)
    assert bool(torch.isinf(inv[1, 0])) and bool(torch.isnan(inv[:, 1:]).all())
    np.testing.assert_allclose(inv[[0, 2], 0].cpu().numpy(), want[[0, 2]].numpy(), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ the models
FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'aoa')
SETTINGS = ((4, 0.6), (3, 0.3))
BAD = list(range(1, 31, 3))          # a third of the vocabulary: captions do end on such a word


def _opt(name):
    V = 30
    return argparse.Namespace(caption_model=name, vocab_size=V, input_encoding_size=16, rnn_size=16, num_layers=1, drop_prob_lm=0.0,
                              seq_length=8, max_length=8, fc_feat_size=20, att_feat_size=20, att_hid_size=16 if name == 'adaatt' else 12,
                              use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)},
                              # aoa: configs/aoa.yml's switches (out_res 0) at the size of tests/golden/aoa_tiny.npz
                              refine=1, refine_aoa=1, use_ff=0, decoder_type='AoA', use_multi_head=2, num_heads=2, multi_head_scale=1,
                              mean_feats=1, ctx_drop=1, dropout_aoa=0.3, out_res=0)


@functools.lru_cache(maxsize=None)
def _golden(name):
    """(state_dict, fc, att, att_masks) of the family's tiny fixture; NewFC reads fc alone, the regions are UpDown's"""
    z = np.load(os.path.join(GOLDEN, '%s_tiny.npz' % name))
    pre = 'adaatt.' if name == 'adaatt' else ''
    P = {k[len(pre) + 2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre + 'P.')}
    u = np.load(os.path.join(GOLDEN, 'updown_tiny.npz'))
    get = lambda k: torch.from_numpy(z[pre + k] if pre + k in z.files else u[k])            # noqa: E731
    return P, get('fc'), get('att'), get('att_masks')


def _perturbed(P, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: v + 0.2 * torch.randn(v.shape, generator=g) for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def _replay(name, k, alpha, constrained=False):
    """the first weight perturbation (chosen on the CPU, from the float64 replay alone) whose smallest score gap and top-k boundary
    gap are both at least 5e-4: 100 x the log-prob tolerance below, and in which the penalty overrules the most probable token at
    least three times.  Returns (weights, replay)."""
    P0, fc, att, am = _golden(name)
    opts = dict(bad_endings=BAD, remove_bad_endings=1, block_trigrams=1) if constrained else {}
    for seed in range(400):
        P = _perturbed(P0, 100 + seed)
        step, state, N = R.family_step(name, P, fc, att, am, _opt(name))
        out = R.search(step, state, N, 31, 8, k, alpha, **opts)
        ok = out['score_gap'] >= 5e-4 and out['topk_gap'] >= 5e-4 and int((out['seq'] > 0).sum()) >= 8 and int((out['choice'] > 0).sum()) >= 3
        if constrained:
            # the constraints must bite where the test looks: a bad ending bars the end token of a live row (-inf in its row), a
            # trigram is penalised, and a row ends early, so that finished rows (logp * 0, token 0) are decoded too
            ok = ok and _constraints_bite(out)
        if ok:
            return P, out
    raise AssertionError('no perturbation separates the decisions')


def _constraints_bite(out):
    live = out['was_unfinished']
    barred = bool((torch.isneginf(out['lps'][:, :, 0]) & live).any())
    ended_early = bool((out['seq'][:, :-1] == 0).any()) and bool(live[:, -1].any())
    return barred and ended_early


def _model(name, P):
    from imagecaptioning.pytorch_amd.captioning import models
    model = models.setup(_opt(name))
    model.load_state_dict(P)
    model = model.to(DEV).eval()
    model.bad_endings_ix = BAD
    _, fc, att, am = _golden(name)
    return model, fc.to(DEV), att.to(DEV), am.to(DEV)


def _check(name, k, alpha, constrained=False):
    P, ref = _replay(name, k, alpha, constrained)
    assert ref['score_gap'] >= 5e-4 and ref['topk_gap'] >= 5e-4
    assert not constrained or _constraints_bite(ref)
    model, fc, att, am = _model(name, P)
    opt = {'sample_method': 'contrastive', 'penalty_alpha': alpha, 'contrastive_k': k}
    if constrained:
        opt.update(remove_bad_endings=1, block_trigrams=1)
    with torch.no_grad():
        seq, logp = model(fc, att, am, opt=opt, mode='sample')
    assert seq.shape == (3, 8) and logp.shape == (3, 8, 31) and seq.dtype == torch.long
    assert torch.equal(seq.cpu(), ref['seq']), (name, k, alpha, seq.cpu().tolist(), ref['seq'].tolist())
    got, lps = logp.double().cpu(), ref['lps']
    live = ref['was_unfinished'][:, :, None].expand_as(lps)
    fin = torch.isfinite(lps) & live
    assert torch.equal(torch.isneginf(got) & live, torch.isneginf(lps) & live)
    print('%s k %d alpha %s: score gap %.3g, top-k gap %.3g, max |seqLogprobs - float64| %.3g'
          % (name, k, alpha, ref['score_gap'], ref['topk_gap'], float((got - lps)[fin].abs().max())))
    np.testing.assert_allclose(got[fin].numpy(), lps[fin].numpy(), rtol=2e-5, atol=5e-6)
    assert bool((got[~live & torch.isfinite(lps)] == 0).all())
    return ref


@pytest.mark.parametrize('k,alpha', SETTINGS)
@pytest.mark.parametrize('name', FAMILIES)
def test_family_against_the_float64_replay(name, k, alpha):
    ref = _check(name, k, alpha)
    assert bool((ref['choice'] > 0).any())              # the penalty decided somewhere: not the greedy caption by another route


@pytest.mark.parametrize('name', FAMILIES)
def test_without_penalty_or_with_one_candidate_it_is_greedy(name):
    P, fc, att, am = _golden(name)
    model, fc, att, am = _model(name, P)
    with torch.no_grad():
        greedy, glogp = model(fc, att, am, opt={'sample_method': 'greedy'}, mode='sample')
        for k, alpha in ((4, 0.0), (1, 0.6), (1, 0.0), (31, 0.0)):
            seq, logp = model(fc, att, am, opt={'sample_method': 'contrastive', 'penalty_alpha': alpha, 'contrastive_k': k}, mode='sample')
            assert torch.equal(seq, greedy), (name, k, alpha, seq.tolist(), greedy.tolist())
            steps = torch.cat([torch.ones(1, dtype=torch.bool, device=DEV), (greedy != 0).cumprod(1).bool().any(0)[:-1]])
            np.testing.assert_allclose(logp[:, steps].cpu().numpy(), glogp[:, steps].cpu().numpy(), rtol=2e-5, atol=5e-6)


def test_trigram_blocking_and_bad_endings_come_before_the_candidates():
    ref = _check('updown', 4, 0.6, constrained=True)
    step, state, N = R.family_step('updown', _replay('updown', 4, 0.6, True)[0], *_golden('updown')[1:], _opt('updown'))
    plain = R.search(step, state, N, 31, 8, 4, 0.6)
    assert not torch.equal(plain['seq'], ref['seq'])          # on the same weights the constraints change the caption


# ------------------------------------------------------------------------------------------------ the command line
def test_eval_entrypoint_decodes_with_contrastive_search(tmp_path):
    from test_langeval_gpu import SMALL, _opts
    from imagecaptioning.pytorch_amd.tools import eval as E
    out_dir = tmp_path / 'cs'
    res = E.main(_opts(SMALL + ['--num_images', '6', '--language_eval', '1', '--split', 'val', '--eval_results_dir', str(out_dir),
                                '--sample_method', 'contrastive', '--penalty_alpha', '0.6', '--contrastive_k', '4']))
    preds = res[1]
    assert len(preds) >= 6 and all(isinstance(p['caption'], str) for p in preds)
    assert os.listdir(out_dir) == ['capmi_val.json']
    out = json.load(open(out_dir / 'capmi_val.json'))
    assert set(out) == {'overall', 'imgToEval'} and 1 <= len(out['imgToEval']) <= len(preds)
    assert all(isinstance(v['caption'], str) for v in out['imgToEval'].values())
