"""Consensus reranking (opt['rerank'], imagecaptioning/pytorch_amd/mbr.py, csrc/mbr.hip, tools/eval.py --rerank) without a GPU: the
options and every refusal, the C ABI of the two entries, the float64 restatement tests/mbr_ref64.py against oracle/ciderd.py and
rewards_ref64's BLEU-4 with one reference, and the selection rule on hand-made matrices."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import ciderd as OC

import mbr_ref64 as M
import rewards_ref64 as W
from test_att_trace_host import tiny_opt

FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')
ENTRIES = {'capmi_mbr_utility': 12, 'capmi_mbr_select': 9}

V = 12
CORPUS = OC.synthetic_corpus(30, V - 1, 3, 8, seed=11)
DF, REF_LEN = OC.build_document_frequency([[OC.tokens_of(r) for r in g] for g in CORPUS])


def _model(name):
    from imagecaptioning.pytorch_amd.captioning import models
    if name == 'ensemble':
        return models.AttEnsemble([models.setup(tiny_opt('updown')), models.setup(tiny_opt('att2in2'))])
    return models.setup(tiny_opt(name))


def test_option_defaults_and_parsing():
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    from imagecaptioning.pytorch_amd import mbr
    assert (opts.DEFAULTS['rerank'], opts.DEFAULTS['rerank_prior']) == ('', 'uniform')
    o = opts.parse_opt([])
    assert o.rerank == '' and o.rerank_prior == 'uniform'
    o = opts.parse_opt(['--rerank', 'mbr_ciderd', '--rerank_prior', 'model', '--sample_n', '10'])
    assert (o.rerank, o.rerank_prior, o.sample_n) == ('mbr_ciderd', 'model', 10)
    assert not mbr.wanted(None) and not mbr.wanted({}) and not mbr.wanted({'rerank': ''}) and mbr.wanted({'rerank': 'mbr_bleu4'})
    assert sorted(mbr.KINDS) == ['mbr_bleu4', 'mbr_ciderd'] and mbr.PRIORS == ('uniform', 'model') and mbr.NMAX == 32


@pytest.mark.parametrize('name', FAMILIES + ('ensemble',))
def test_models_start_without_a_reranking(name):
    assert _model(name).last_rerank is None


@pytest.mark.parametrize('name', ('updown', 'transformer', 'ensemble'))
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: every refusal is raised before the device check that a call without the option runs into"""
    from imagecaptioning.pytorch_amd.captioning.utils import rewards
    from imagecaptioning.pytorch_amd._lib import CapmiError
    model = _model(name).eval()
    fc, att = torch.zeros(2, 20), torch.zeros(2, 4, 20)

    def call(**opt):
        with torch.no_grad():
            return model(fc, att, None, opt=opt, mode='sample')

    ok = dict(rerank='mbr_bleu4', sample_n=3, sample_method='sample')
    with pytest.raises(ValueError, match='rerank'):
        call(**dict(ok, rerank='mbr_meteor'))
    with pytest.raises(ValueError, match='rerank_prior'):
        call(**dict(ok, rerank_prior='length'))
    for n in (1, 33):
        with pytest.raises(ValueError, match='sample_n'):
            call(**dict(ok, sample_n=n))
    with pytest.raises(ValueError, match='sample_n'):
        call(rerank='mbr_bleu4')                                          # sample_n defaults to 1
    assert rewards.CiderD_scorer is None
    with pytest.raises(ValueError, match='init_scorer'):
        call(**dict(ok, rerank='mbr_ciderd'))
    # a beam search whose sample_n is neither 1 nor beam_size // group_size fills only the first B rows
    with pytest.raises(ValueError, match='beam_size'):
        call(rerank='mbr_bleu4', sample_n=2, sample_method='beam_search', beam_size=3)
    with pytest.raises(ValueError, match='beam_size'):
        call(rerank='mbr_bleu4', sample_n=3, sample_method='greedy', beam_size=6, group_size=3)
    model.train()
    with pytest.raises(NotImplementedError, match='eval'):
        call(**ok)
    model.eval()
    assert model.last_rerank is None
    # valid options: the call goes on to the device check of a CPU tensor, which is no refusal of the option
    for opt in (ok, dict(rerank='mbr_bleu4', sample_n=3, sample_method='beam_search', beam_size=3), dict(rerank='')):
        with pytest.raises((CapmiError, RuntimeError, AssertionError)) as e:
            call(**opt)
        assert not isinstance(e.value, (NotImplementedError, ValueError)), e.value
    assert model.last_rerank is None


def test_wrappers_refuse_bad_shapes_on_the_host():
    from imagecaptioning.pytorch_amd import mbr
    seq = torch.zeros(6, 5, dtype=torch.long)
    with pytest.raises(ValueError):
        mbr.utility(seq, 3, 'mbr_unknown')
    with pytest.raises(ValueError):
        mbr.utility(seq, 3, 'mbr_bleu4')                                  # not a device tensor
    with pytest.raises(ValueError, match='rerank_prior'):
        mbr.rerank(seq, torch.zeros(6, 5, 13), 3, 'mbr_bleu4', 'length')
    sel = torch.tensor([[-1.0, -2.0, -3.0], [-0.5, -0.25, -4.0]])
    toks = torch.tensor([[3, 0, 0], [4, 5, 6]])
    assert mbr.logp_sum(toks, sel).tolist() == [-3.0, -4.75]              # the end token's step counts, the steps behind it do not
    dense = torch.zeros(2, 3, 8)
    dense.scatter_(2, toks.unsqueeze(2), sel.unsqueeze(2))
    assert torch.equal(mbr.logp_sum(toks, dense), mbr.logp_sum(toks, sel)) and mbr.logp_sum(toks, dense).dtype == torch.float64
    np.testing.assert_array_equal(M.seq_weight(sel.numpy(), toks.numpy()), [-3.0, -4.75])
    t = torch.arange(12).view(6, 2)
    assert mbr.gather_rows(t, torch.tensor([2, 0], dtype=torch.int32), 3).tolist() == [[4, 5], [6, 7]]


def test_new_entries_in_header_match_the_binding():
    from imagecaptioning.pytorch_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'capmi.h')).read(), flags=re.S)
    decl = dict((m.group(1), m.group(2).strip()) for m in
                re.finditer(r'\b(?:int|int64_t|const char \*)\s*(capmi_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    for name, nargs in ENTRIES.items():
        assert len(decl[name].split(',')) == nargs == len(_lib.SIGNATURES[name]), name
        assert decl[name].rstrip().endswith('void *stream') and hasattr(_lib.lib, name)
    assert re.search(r'#define CAPMI_MBR_CIDERD 0\b', src) and re.search(r'#define CAPMI_MBR_BLEU4 1\b', src)
    assert (_lib.MBR_CIDERD, _lib.MBR_BLEU4) == (0, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _group(seed, n, L):
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, L), dtype=np.int64)
    for r in range(n):
        ln = int(rng.integers(0, L + 1))
        rows[r, :ln] = rng.integers(1, V, size=ln)
    rows[0] = 0                                                           # the empty caption: the word 0 alone
    rows[1] = rng.integers(1, V, size=L)                                  # a full row: no end token
    if n > 3:
        rows[3] = rows[2]
    return rows


@pytest.mark.parametrize('n,L', [(2, 1), (5, 6), (6, 20)])
def test_restatement_is_the_two_scorers_with_one_reference(n, L):
    rows = _group(100 * n + L, n, L)
    sc = OC.CiderD(DF, REF_LEN)
    U = M.utility(rows, 'ciderd', DF, REF_LEN)
    Ub = M.utility(rows, 'bleu4')
    for i in range(n):
        for j in range(n):
            assert abs(U[i, j] - sc.score_one(OC.tokens_of(rows[i]), [OC.tokens_of(rows[j])])) <= 1e-12
            assert abs(Ub[i, j] - W.bleu4(rows[i], [rows[j]])) <= 1e-12
    if L > 1:
        assert abs(Ub[1, 1] - 1.0) < 1e-8 and (np.diag(U)[1:] > 1.0).all()
    if n > 3:
        assert np.array_equal(U[3], U[2]) and np.array_equal(U[:, 3], U[:, 2])
    with pytest.raises(ValueError):
        M.utility(rows, 'meteor')


def test_utility_is_not_symmetric():
    """a repeated word is clipped on the hypothesis's side only: min(h, r) * r"""
    rows = np.array([[7, 7, 7, 3, 0], [7, 3, 0, 0, 0]])
    for kind in M.KINDS:
        U = M.utility(rows, kind, DF, REF_LEN)
        assert abs(U[0, 1] - U[1, 0]) > 1e-3, kind


def test_selection_rule_on_hand_made_matrices():
    rows = np.array([[1, 2, 0], [3, 4, 0], [5, 0, 0], [3, 4, 0]])        # candidate 3 repeats candidate 1
    U = np.array([[9., 1., 2., 1.],
                  [2., 9., 4., 6.],
                  [1., 2., 9., 2.],
                  [2., 6., 4., 9.]])
    e, c = M.select(U, rows)
    np.testing.assert_allclose(e, [4 / 3, 4.0, 5 / 3, 4.0], rtol=0, atol=1e-15)      # the diagonal is not read
    assert c == 1                                                         # the duplicate ties and is never returned
    U2 = U.copy()
    U2[3] += 1.0                                                          # the duplicate ahead: still the first occurrence
    assert M.select(U2, rows)[1] == 1
    assert M.first_occurrence(rows) == [True, True, True, False]
    # a tie between distinct captions: the lowest index
    T = np.array([[0., 3., 1.], [3., 0., 1.], [1., 1., 0.]])
    assert M.select(T, rows[:3])[1] == 0
    # all zero: 0; all identical: 0
    assert M.select(np.zeros((4, 4)), rows)[1] == 0
    same = np.tile(rows[:1], (3, 1))
    e, c = M.select(np.full((3, 3), 7.0), same)
    assert c == 0 and e.tolist() == [7.0, 7.0, 7.0]
    # rows that differ only behind the end token are one caption
    assert M.first_occurrence(np.array([[2, 0, 5], [2, 0, 7], [2, 7, 0]])) == [True, False, True]
    # the model prior: w = exp(weight - max), the largest exactly 1
    wt = np.array([-1.0, -3.0, -2.0, -50.0])
    w = M.weights(wt, 4)
    assert w[0] == 1.0 and abs(w[1] - np.exp(-2.0)) < 1e-17
    e, c = M.select(U, rows, wt)
    want1 = (w[0] * 2 + w[2] * 4 + w[3] * 6) / (w[0] + w[2] + w[3])
    assert abs(e[1] - want1) <= 1e-15
    assert M.margin(e, rows) > 0 and M.margin(np.zeros(4), np.tile(rows[:1], (4, 1))) == np.inf
    # the others' weights all underflow: 0, not NaN
    e, _ = M.select(U[:2, :2], rows[:2], np.array([0.0, -1e4]))
    assert e.tolist() == [0.0, 2.0]


def test_rerank_of_the_restatement_joins_the_parts():
    rows = np.concatenate([_group(5, 5, 6), _group(6, 5, 6)])
    wt = np.random.default_rng(2).normal(size=10) * 3
    U, e, c = M.rerank(rows, 5, 'ciderd', DF, REF_LEN, wt)
    assert U.shape == (2, 5, 5) and e.shape == (2, 5) and c.shape == (2,) and c.dtype == np.int32
    for g in range(2):
        eg, cg = M.select(M.utility(rows[5 * g:5 * g + 5], 'ciderd', DF, REF_LEN), rows[5 * g:5 * g + 5], wt[5 * g:5 * g + 5])
        assert np.array_equal(e[g], eg) and c[g] == cg


# ---------------------------------------------------------------------------------------------------------------------------
# tools/eval.py --rerank: the decode options and the dump
# ---------------------------------------------------------------------------------------------------------------------------
def test_eval_rerank_options_and_dump(tmp_path):
    from imagecaptioning.pytorch_amd.tools import eval as E
    ns = argparse.Namespace
    assert E.rerank_kwargs(ns(rerank='', sample_n=5, sample_n_method='sample')) == {}
    assert E.rerank_kwargs(ns(sample_n=5, sample_n_method='sample')) == {}
    assert E.rerank_kwargs(ns(rerank='mbr_ciderd', rerank_prior='model', sample_n=5, sample_n_method='top3')) == \
        dict(rerank='mbr_ciderd', rerank_prior='model', sample_n=5, sample_method='top3', beam_size=1)
    assert E.rerank_kwargs(ns(rerank='mbr_bleu4', sample_n=4, sample_n_method='bs')) == \
        dict(rerank='mbr_bleu4', rerank_prior='uniform', sample_n=4, sample_method='beam_search', beam_size=4, group_size=1)
    for method in ('dbs', 'dsample'):
        with pytest.raises(NotImplementedError, match='sample_n_method'):
            E.rerank_kwargs(ns(rerank='mbr_bleu4', sample_n=4, sample_n_method=method))
    B, n, L = 3, 2, 4
    last = dict(choice=torch.tensor([1, 0, 1], dtype=torch.int32), expected=torch.arange(6, dtype=torch.float64).view(B, n),
                candidates=torch.arange(B * n * L).view(B * n, L))
    dump = E.RerankDump()
    dump.add_batch(last, [{'id': 'a'}, {'id': 'b'}, {'id': 'c'}], 2)          # the third image is past num_images
    dump.add_batch(last, [{'id': 'd'}, {'id': 'e'}, {'id': 'f'}], 0)
    path = dump.write(ns(eval_results_dir=str(tmp_path), id='run7'), 'val')
    assert path == os.path.join(str(tmp_path), 'run7_val_mbr.npz')
    z = np.load(path)
    assert z['image_id'].tolist() == ['a', 'b'] and z['choice'].tolist() == [1, 0] and z['choice'].dtype == np.int32
    assert np.array_equal(z['expected'], last['expected'][:2].numpy())
    assert np.array_equal(z['candidates'], last['candidates'].view(B, n, L)[:2].numpy())
