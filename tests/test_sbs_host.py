"""Stochastic beam search (opt['sample_method'] = 'sbs'; imagecaptioning/pytorch_amd/sbs.py, beam.stochastic_beam_search_steps,
csrc/sbs.hip) without a GPU: the float64 replay tests/sbs_ref64.py IS sampling without replacement -- checked by exhaustion on a
tree small enough to enumerate -- the importance weights, the option plumbing and every refusal."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import sbs_ref64 as S
from test_att_trace_host import tiny_opt

FAMILIES = ('updown', 'newfc', 'att2in2', 'adaatt', 'adaattmo', 'transformer', 'aoa')
ENTRIES = {'capmi_sbs_scratch_bytes': 4, 'capmi_sbs_select': 21, 'capmi_sbs_backtrack': 10}

# the tree of the exhaustive check: V1 = 4, L = 3 -> 40 complete sequences.  Seed and scale were chosen (on the CPU) so that the
# rarest sequence has p = 0.0039: no cell of any table below expects fewer than 50 of the 20 000 trials (asserted in the test).
V1, L, TRIALS = 4, 3, 20000
TREE = S.make_tree(V1, L, seed=7, scale=0.6)
SEQS, P = S.sequences(TREE)


def _model(name):
    from imagecaptioning.pytorch_amd.captioning import models
    if name == 'ensemble':
        return models.AttEnsemble([models.setup(tiny_opt('updown')), models.setup(tiny_opt('att2in2'))])
    return models.setup(tiny_opt(name))


def test_the_tree_is_a_distribution_over_40_sequences():
    assert SEQS.shape == (40, L) and abs(P.sum() - 1.0) < 1e-12
    assert len({tuple(s) for s in SEQS.tolist()}) == 40
    assert P.min() * TRIALS >= 50, P.min()
    # sampling without replacement with k = 1 is sampling; the inclusion probabilities of k draws sum to k
    np.testing.assert_allclose(S.inclusion_probabilities(P, 1), P, rtol=0, atol=1e-15)
    assert abs(S.inclusion_probabilities(P, 2).sum() - 2.0) < 1e-12


@pytest.mark.parametrize('k', (1, 2, 3))
def test_replay_samples_without_replacement(k):
    """20 000 searches at once (the trials are the replay's images): the first row of a search is a sample from the model, the k rows
    are k draws without replacement -- each sequence's frequencies within 5 binomial standard deviations of the exact numbers"""
    rng = np.random.default_rng(1000 + k)
    out = S.search(TREE, TRIALS, k, rng.gumbel(size=(L, TRIALS * k, V1)))
    rows = out['seq'].reshape(TRIALS, k, L)
    code = {tuple(s): i for i, s in enumerate(SEQS.tolist())}
    ids = np.array([[code[tuple(r)] for r in img] for img in rows.tolist()])             # [TRIALS, k]; a KeyError: not a sequence
    assert all(len(set(img)) == k for img in ids.tolist()), 'a search returned the same sequence twice'
    assert (np.diff(out['g'], axis=1) <= 0).all()
    np.testing.assert_allclose(out['phi'], np.log(P)[ids], rtol=0, atol=1e-12)
    inc = S.inclusion_probabilities(P, k)
    for name, prob, count in (('first', P, np.bincount(ids[:, 0], minlength=40)),
                              ('inclusion', inc, np.bincount(ids.reshape(-1), minlength=40))):
        assert (prob * TRIALS >= 50).all(), name
        sd = np.sqrt(TRIALS * prob * (1 - prob))
        z = np.abs(count - TRIALS * prob) / sd
        assert z.max() <= 5.0, (name, k, int(z.argmax()), float(z.max()))


def test_select_step_of_the_replay_by_hand():
    """one row, no noise: the root orders by log-prob; below the root the arg-max inherits g and every other child lies below it"""
    lp = np.log(np.array([[[0.1, 0.2, 0.3, 0.4]]]))
    zero = np.zeros((1, 1, 4))
    r = S.select_step(lp, [[0.0]], [[0.0]], [[True]], zero, 3, step0=True)
    assert r['token'].tolist() == [[3, 2, 1]] and r['parent'].tolist() == [[0, 0, 0]] and r['alive'].tolist() == [[True] * 3]
    np.testing.assert_allclose(r['g'], lp[0, 0, [3, 2, 1]][None], atol=1e-15)
    r = S.select_step(lp, [[-1.0]], [[5.0]], [[True]], zero, 4)
    assert r['token'].tolist() == [[3, 2, 1, 0]] and r['g'][0, 0] == 5.0 and (np.diff(r['g'][0]) < 0).all()
    assert r['alive'].tolist() == [[True, True, True, False]]
    # the truncation, written the other way: exp(-g~) = exp(-g_j) - exp(-Z) + exp(-s)
    s, Z = -1.0 + lp[0, 0], -1.0 + lp[0, 0, 3]
    np.testing.assert_allclose(np.exp(-r['g'][0]), (np.exp(-5.0) - np.exp(-Z) + np.exp(-s))[[3, 2, 1, 0]], rtol=1e-12)
    # an ended row is one candidate, bit for bit; blocked columns are never chosen; force_end ends everything
    lp2 = np.log(np.array([[[0.25] * 4, [0.1, 0.2, 0.3, 0.4]]]))
    lp2[0, 1, 3] = -np.inf
    r = S.select_step(lp2, [[-2.0, -3.0]], [[0.7, 0.3]], [[False, True]], np.zeros((1, 2, 4)), 3, force_end=True)
    assert r['parent'].tolist() == [[0, 1, 1]] and r['token'].tolist() == [[0, 2, 1]] and r['g'][0, 0] == 0.7 and r['g'][0, 1] == 0.3
    assert r['phi'][0, 0] == -2.0 and not r['alive'].any()
    # equal values: the lower flat index
    r = S.select_step(np.log(np.full((1, 1, 4), 0.25)), [[0.0]], [[0.0]], [[True]], zero, 2, step0=True)
    assert r['token'].tolist() == [[0, 1]] and r['gap'][0] == 0.0


def test_log_weights_against_the_formula():
    from imagecaptioning.pytorch_amd import sbs
    rng = np.random.default_rng(5)
    for k in (1, 2, 3, 7):
        phi = -rng.uniform(1, 30, size=(6, k))
        g = -np.sort(-(phi + rng.gumbel(size=(6, k))), axis=1)
        got = sbs.log_weights(torch.from_numpy(phi).float(), torch.from_numpy(g).float())
        assert got.dtype == torch.float64 and got.shape == (6, k)
        want = S.log_weights(phi.astype(np.float32), g.astype(np.float32))
        if k == 1:
            assert got.tolist() == [[0.0]] * 6
            continue
        assert torch.isneginf(got[:, -1]).all() and np.isneginf(want[:, -1]).all()
        np.testing.assert_allclose(got[:, :-1].numpy(), want[:, :-1], rtol=0, atol=1e-9)
        np.testing.assert_allclose(np.exp(got.numpy()).sum(1), 1.0, atol=1e-12)
    assert sbs.log_weights(torch.tensor([[-1.0, -2.0]]), torch.tensor([[0.5, -3.0]])).tolist() == [[0.0, float('-inf')]]
    # a threshold far below: q -> 1, the weights are the probabilities, renormalised
    lw = sbs.log_weights(torch.tensor([[-1.0, -2.0, -3.0]]), torch.tensor([[0.0, -1.0, -200.0]]))
    np.testing.assert_allclose(np.exp(lw[0, :2].numpy()), np.exp([-1.0, -2.0]) / np.exp([-1.0, -2.0]).sum(), rtol=1e-12)


def test_the_estimator_of_the_replay_is_consistent():
    """sum_i w_i f(y_i) over many searches approaches E_p[f] (the unnormalised estimator is unbiased): f = the length of a sequence"""
    k = 3
    rng = np.random.default_rng(77)
    out = S.search(TREE, TRIALS, k, rng.gumbel(size=(L, TRIALS * k, V1)))
    f_all = (SEQS != 0).sum(1) + 1.0
    code = {tuple(s): i for i, s in enumerate(SEQS.tolist())}
    f = np.array([f_all[code[tuple(r)]] for r in out['seq'].tolist()]).reshape(TRIALS, k)
    kappa = out['g'][:, k - 1:k]
    w = np.exp(out['phi'][:, :k - 1]) / (1.0 - np.exp(-np.exp(out['phi'][:, :k - 1] - kappa)))
    est = (w * f[:, :k - 1]).sum(1)
    truth = float((P * f_all).sum())
    assert abs(est.mean() - truth) <= 5 * est.std() / np.sqrt(TRIALS), (est.mean(), truth)


def test_backtrack_of_the_replay_by_hand():
    parent = np.array([[[0, 0]], [[1, 0]], [[0, 1]]])
    token = np.array([[[5, 0]], [[0, 7]], [[0, 9]]])
    alive = np.array([[[1, 0]], [[0, 1]], [[0, 0]]])
    seq, length, lineage = S.backtrack(parent, token, alive)
    assert seq.tolist() == [[0, 0, 0], [5, 7, 9]] and length.tolist() == [1, 3]
    assert lineage.tolist() == [[0, 0], [-1, 0], [-1, 1]]


# ---------------------------------------------------------------------------------------------------------------------------
# options, refusals, the binding
# ---------------------------------------------------------------------------------------------------------------------------
def test_eval_options():
    from imagecaptioning.pytorch_amd.tools import eval as E
    from imagecaptioning.pytorch_amd import sbs
    ns = argparse.Namespace
    assert sbs.wanted({'sample_method': 'sbs'}) and not sbs.wanted({}) and not sbs.wanted(None) and not sbs.wanted({'sample_method': 'bs'})
    assert sbs.K_MAX == 16
    for prior in ('uniform', 'model'):
        assert E.rerank_kwargs(ns(rerank='mbr_bleu4', rerank_prior=prior, sample_n=4, sample_n_method='sbs')) == \
            dict(rerank='mbr_bleu4', rerank_prior=prior, sample_n=4, sample_method='sbs', beam_size=1)
    for method in ('dbs', 'dsample', 'dsbs'):
        with pytest.raises(NotImplementedError, match='sample_n_method'):
            E.rerank_kwargs(ns(rerank='mbr_bleu4', sample_n=4, sample_n_method=method))


class _FakeModel:
    """what eval_split_n asks of a model"""
    vocab = {str(i): 'w%d' % i for i in range(1, 9)}

    def __init__(self):
        self.calls = []

    def __call__(self, fc, att, att_masks, opt=None, mode=None):
        self.calls.append(dict(opt))
        n, B = opt['sample_n'], fc.shape[0]
        seq = torch.tensor([[1 + (r % 7), 2, 0] for r in range(B * n)])
        logp = torch.full((B * n, 3, 9), -2.0)
        self.last_sbs = dict(log_w=torch.log(torch.tensor([[0.75, 0.25, 0.0]] * B, dtype=torch.float64)))
        return seq, logp


@pytest.mark.parametrize('verbose', (0, 1))
def test_eval_split_n_has_a_branch_of_its_own(verbose):
    from imagecaptioning.pytorch_amd.tools import eval as E
    model, preds = _FakeModel(), []
    opt = argparse.Namespace(sample_n=3, sample_n_method='sbs', beam_size=1, temperature=0.5, verbose_beam=verbose, group_size=1)
    data = {'infos': [{'id': 'a'}, {'id': 'b'}]}
    rows = E.eval_split_n(model, preds, torch.zeros(2, 4), torch.zeros(2, 3, 4), None, data, opt)
    assert len(model.calls) == 1
    kw = model.calls[0]
    assert (kw['sample_method'], kw['sample_n'], kw['beam_size'], kw['group_size'], kw['temperature']) == ('sbs', 3, 1, 1, 0.5)
    assert rows.shape == (2, 3, 3) and [p['image_id'] for p in preds] == ['a'] * 3 + ['b'] * 3
    assert all(abs(p['perplexity'] - 2.0) < 1e-6 for p in preds) and preds[0]['caption'] == 'w1 w2'
    if verbose:
        assert [p['log_w'] for p in preds[:3]] == [float(np.log(0.75)), float(np.log(0.25)), float('-inf')]
    else:
        assert all('log_w' not in p for p in preds)


@pytest.mark.parametrize('name', FAMILIES + ('ensemble',))
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: every refusal is raised before the device check that a valid call runs into"""
    from imagecaptioning.pytorch_amd._lib import CapmiError
    model = _model(name).eval()
    assert model.last_sbs is None
    fc, att = torch.zeros(2, 20), torch.zeros(2, 4, 20)

    def call(**opt):
        with torch.no_grad():
            return model(fc, att, None, opt=opt, mode='sample')

    ok = dict(sample_method='sbs', sample_n=3)
    if name == 'ensemble':
        with pytest.raises(NotImplementedError, match='AttEnsemble'):
            call(**ok)
        return
    with pytest.raises(NotImplementedError, match='block_trigrams'):
        call(**dict(ok, block_trigrams=1))
    with pytest.raises(NotImplementedError, match='group_size'):
        call(**dict(ok, group_size=2))
    with pytest.raises(NotImplementedError, match='output_logsoftmax'):
        call(**dict(ok, output_logsoftmax=0))
    for n in (0, 17):
        with pytest.raises(ValueError, match='sample_n'):
            call(**dict(ok, sample_n=n))
    with pytest.raises(ValueError, match='temperature'):
        call(**dict(ok, temperature=0.0))
    model.train()
    with pytest.raises(NotImplementedError, match='eval'):
        call(**ok)
    model.eval()
    # valid options go on to the device check of a CPU tensor, which is no refusal of the option
    for opt in (ok, dict(ok, sample_n=1), dict(ok, decoding_constraint=1, remove_bad_endings=1, suppress_UNK=1, temperature=0.7),
                dict(ok, rerank='mbr_bleu4', rerank_prior='model')):
        with pytest.raises((CapmiError, RuntimeError, AssertionError)) as e:
            call(**opt)
        assert not isinstance(e.value, (NotImplementedError, ValueError)), e.value
    assert model.last_sbs is None


def test_a_model_without_a_stepper_refuses():
    from imagecaptioning.pytorch_amd.captioning.models.CaptionModel import CaptionModel
    from imagecaptioning.pytorch_amd import sbs

    class Bare(CaptionModel):
        pass
    with pytest.raises(NotImplementedError, match='single-step decoder'):
        sbs.check_options(Bare().eval(), dict(sample_method='sbs', sample_n=2))


def test_new_entries_in_header_match_the_binding():
    from imagecaptioning.pytorch_amd import _lib, ops
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'capmi.h')).read(), flags=re.S)
    decl = dict((m.group(1), m.group(2).strip()) for m in
                re.finditer(r'\b(?:int|int64_t|const char \*)\s*(capmi_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    for name, nargs in ENTRIES.items():
        assert len(decl[name].split(',')) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.lib, name)
    assert _lib.lib.capmi_sbs_scratch_bytes(3, 5, 5, 9488) == 3 * 5 * 10 * 5 * 8 and _lib.lib.capmi_sbs_scratch_bytes(0, 1, 1, 1) == 0
    assert ops.SBS_BD_MAX == 16
    # the argument checks come before any launch: NULL pointers, and an image that cannot supply bd candidates
    assert _lib.lib.capmi_sbs_select(None, None, None, None, None, 0, 0, 1, 1, 1, 4, 1, 0, None, 0, None, None, None, None, None,
                                     None) == _lib.EINVAL
    assert _lib.lib.capmi_sbs_backtrack(None, None, None, 1, 1, 1, None, None, None, None) == _lib.EINVAL
    cpu = torch.zeros(2, 3)
    with pytest.raises(_lib.CapmiError):
        ops.sbs_select(cpu, cpu[:, :1], cpu[:, :1], torch.ones(2, 1, dtype=torch.uint8), 2)
