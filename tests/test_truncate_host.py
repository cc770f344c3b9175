"""Min-p, epsilon, eta and locally typical sampling -- what can be checked without a GPU: the spellings and their ranges, which
requests leave the one-call rollouts, the refusals, the float64 restatement (tests/truncate_ref64.py) against rows worked out by
hand, its input builders' margins, and the ctypes prototype of capmi_truncate_rows against the header."""
import argparse
import math
import os
import re

import pytest
import torch

from conftest import ROOT
import truncate_ref64 as R
from test_att_trace_host import tiny_opt

HEADER = os.path.join(ROOT, 'include', 'capmi.h')


# ------------------------------------------------------------------------------------------------ spellings
def test_parse_truncation_and_sample_method():
    from imagecaptioning.pytorch_amd.captioning.models.utils import parse_sample_method, parse_truncation
    assert parse_truncation('minp0.1') == ('minp', 0.1) and parse_truncation('minp1') == ('minp', 1.0)
    assert parse_truncation('eps0.0003') == ('eps', 0.0003) and parse_truncation('eps3e-4') == ('eps', 3e-4)
    assert parse_truncation('eta0.002') == ('eta', 0.002) and parse_truncation('typ0.9') == ('typ', 0.9)
    for name in ('greedy', 'sample', 'gumbel', 'top5', 'top0.9', 'sbs', 'beam_search', 'minp', 'typical', 'epsilon', 'xyz', None):
        assert parse_truncation(name) is None, name
    for name, rng in (('minp0', '0 < a <= 1'), ('minp1.5', '0 < a <= 1'), ('minp-0.1', '0 < a <= 1'), ('eps0', '0 < e < 1'),
                      ('eps1', '0 < e < 1'), ('eta1', '0 < e < 1'), ('eta0', '0 < e < 1'), ('typ1', '0 < tau < 1'), ('typ0', '0 < tau < 1'),
                      ('typ2', '0 < tau < 1')):
        with pytest.raises(ValueError, match=re.escape(rng)):
            parse_truncation(name)
        with pytest.raises(ValueError, match=re.escape(rng)):
            parse_sample_method(name, 1.0)
    # the new spellings are plain sampling for the select; every old return value stands
    for name in ('minp0.1', 'eps0.0003', 'eta0.002', 'typ0.9'):
        assert parse_sample_method(name, 0.7) == ('sample', 0.7, 0, 0.0)
    assert parse_sample_method('greedy', 0.5) == ('greedy', 0.5, 0, 0.0)
    assert parse_sample_method('sample', 1.3) == ('sample', 1.3, 0, 0.0)
    assert parse_sample_method('gumbel', 1.3) == ('sample', 1.0, 0, 0.0)
    assert parse_sample_method('top5', 2.0) == ('sample', 2.0, 5, 0.0)
    assert parse_sample_method('top0.9', 1.0) == ('sample', 1.0, 0, 0.9)
    for name in ('beam_search_xyz', 'typical', 'minp', 'epsilon0.1'):
        with pytest.raises(NotImplementedError, match='sample_method'):
            parse_sample_method(name, 1.0)


def test_wants_options():
    from imagecaptioning.pytorch_amd import decode
    for name in ('minp0.1', 'eps0.0003', 'eta0.002', 'typ0.9', 'minp1'):
        assert decode.wants_options({'sample_method': name})
        assert decode.wants_options({'sample_method': name, 'beam_size': 5, 'sample_n': 3})
        assert decode.truncation({'sample_method': name})[0] == name[:4 if name.startswith('minp') else 3]
    for opt in ({}, {'sample_method': 'greedy', 'beam_size': 5}, {'sample_method': 'sample'}, {'sample_method': 'top0.9'},
                {'sample_method': 'top5'}, {'sample_method': 'gumbel'}, {'sample_method': 'sbs'}, {'group_size': 1}):
        assert not decode.wants_options(opt), opt
        assert decode.truncation(opt) is None
    assert decode.truncation(None) is None
    assert decode.wants_options({'group_size': 2}) and decode.wants_options({'decoding_constraint': 1})
    with pytest.raises(ValueError, match='0 < tau < 1'):
        decode.wants_options({'sample_method': 'typ1.0'})


def test_eval_accepts_the_spellings():
    from imagecaptioning.pytorch_amd.tools import eval as E
    ns = argparse.Namespace
    for method in ('typ0.9', 'minp0.05', 'eps0.0003', 'eta0.002'):
        assert E.rerank_kwargs(ns(rerank='mbr_ciderd', rerank_prior='model', sample_n=5, sample_n_method=method)) == \
            dict(rerank='mbr_ciderd', rerank_prior='model', sample_n=5, sample_method=method, beam_size=1)
    with pytest.raises(NotImplementedError, match='sample_n_method'):
        E.rerank_kwargs(ns(rerank='mbr_bleu4', sample_n=4, sample_n_method='dtyp0.9'))
    with pytest.raises(ValueError, match='0 < e < 1'):
        E.rerank_kwargs(ns(rerank='mbr_bleu4', sample_n=4, sample_n_method='eta2'))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('name', ('updown', 'newfc', 'transformer'))
def test_refusals_come_before_any_device_work(name):
    """CPU tensors: a call that got past the refusals would fail in the device check or in a launch instead"""
    from imagecaptioning.pytorch_amd.captioning import models
    model = models.setup(tiny_opt(name))
    fc, att = torch.zeros(2, 20), torch.zeros(2, 3, 20)
    model.train()
    for method in ('typ0.9', 'minp0.1', 'eps0.001', 'eta0.002'):
        with pytest.raises(NotImplementedError, match='test-time option'):
            model(fc, att, None, opt={'sample_method': method, 'sample_n': 2}, mode='sample')
    model.eval()
    with pytest.raises(NotImplementedError, match='output_logsoftmax=0'):
        model(fc, att, None, opt={'sample_method': 'typ0.9', 'output_logsoftmax': 0}, mode='sample')
    with pytest.raises(ValueError, match='0 < a <= 1'):
        model(fc, att, None, opt={'sample_method': 'minp1.2'}, mode='sample')


def test_train_sample_method_is_refused():
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules.loss_wrapper import LossWrapper
    model = models.setup(tiny_opt('updown'))
    for method in ('typ0.9', 'eta0.002'):
        opt = synthetic.updown_opt(train_sample_method=method)
        with pytest.raises(NotImplementedError, match='train_sample_method'):
            LossWrapper(model, opt)
    LossWrapper(model, synthetic.updown_opt(train_sample_method='sample'))


# ------------------------------------------------------------------------------------------------ the oracle, by hand
P5 = [0.5, 0.25, 0.15, 0.07, 0.03]


def _row5(T=1.0):
    return (torch.tensor(P5, dtype=R.F64).log() * T + 1.7)[None]            # any shift; softmax(x / T) = P5


def _expect(ref, kept):
    kept = torch.tensor(kept)
    assert ref['kept'][0].tolist() == kept.tolist()
    mass = sum(p for p, k in zip(P5, kept.tolist()) if k)
    assert abs(float(ref['mass'][0]) - mass) < 1e-12 and int(ref['count'][0]) == int(kept.sum())
    for v in range(5):
        if kept[v]:
            assert abs(float(ref['q'][0, v]) - math.log(P5[v] / mass)) < 1e-12
        else:
            assert float(ref['q'][0, v]) == float('-inf')


@pytest.mark.parametrize('T', (1.0, 0.7))
def test_oracle_on_a_row_worked_out_by_hand(T):
    """p = (0.5, 0.25, 0.15, 0.07, 0.03), H = 1.2691 nats.
    minp 0.2: threshold 0.1, keeps 3; minp 0.5: 0.25 >= 0.25 is kept; minp 1: the maximum alone.
    eps 0.1: keeps 3; eps 0.6: nothing reaches it, the maximum stays.
    eta 0.04: sqrt(0.04) exp(-H) = 0.0562 > 0.04, threshold 0.04, keeps 4; eta 0.5: sqrt(0.5) exp(-H) = 0.1988 < 0.5, keeps 2.
    typ: scores |-log p - H| = 0.5759, 0.1172, 0.6281, 1.3902, 2.2375 -> order 1, 0, 2, 3, 4 with masses 0.25, 0.75, 0.90, 0.97, 1:
    tau 0.2 keeps {1}, 0.7 keeps {0, 1}, 0.8 keeps {0, 1, 2}, 0.95 keeps four."""
    x = _row5(T)
    H = -sum(p * math.log(p) for p in P5)
    assert abs(H - 1.26906) < 1e-5 and abs(float(R.stats(x, T)[2][0]) - H) < 1e-12
    _expect(R.truncate_ref(x, 'minp', 0.2, T), [1, 1, 1, 0, 0])
    _expect(R.truncate_ref(x, 'minp', 0.4999, T), [1, 1, 0, 0, 0])
    _expect(R.truncate_ref(x, 'minp', 0.51, T), [1, 0, 0, 0, 0])
    _expect(R.truncate_ref(x, 'minp', 1.0, T), [1, 0, 0, 0, 0])
    _expect(R.truncate_ref(x, 'eps', 0.1, T), [1, 1, 1, 0, 0])
    _expect(R.truncate_ref(x, 'eps', 0.6, T), [1, 0, 0, 0, 0])
    assert abs(math.sqrt(0.04) * math.exp(-H) - 0.05622) < 1e-4 and abs(math.sqrt(0.5) * math.exp(-H) - 0.19876) < 1e-4
    _expect(R.truncate_ref(x, 'eta', 0.04, T), [1, 1, 1, 1, 0])
    _expect(R.truncate_ref(x, 'eta', 0.5, T), [1, 1, 0, 0, 0])
    s = [abs(-math.log(p) - H) for p in P5]
    assert [round(v, 4) for v in s] == [0.5759, 0.1172, 0.6281, 1.3902, 2.2375]
    _expect(R.truncate_ref(x, 'typ', 0.2, T), [0, 1, 0, 0, 0])
    _expect(R.truncate_ref(x, 'typ', 0.7, T), [1, 1, 0, 0, 0])
    _expect(R.truncate_ref(x, 'typ', 0.8, T), [1, 1, 1, 0, 0])
    _expect(R.truncate_ref(x, 'typ', 0.95, T), [1, 1, 1, 1, 0])


@pytest.mark.parametrize('V1', (5, 64, 1031))
def test_oracle_on_uniform_one_hot_and_barred_rows(V1):
    s = R.special_rows(V1)
    for kind in R.KINDS:
        for param in R.PARAMS[kind] + ((1.0,) if kind == 'minp' else ()):
            for T in (1.0, 0.7):
                ref = R.truncate_ref(s, kind, param, T)
                assert ref['count'][:3].tolist() == [V1, 1, 1], (kind, param, T, ref['count'])
                assert abs(float(ref['q'][0, 0]) + math.log(V1)) < 1e-12 and float(ref['q'][1, V1 // 2]) == 0.0
                assert abs(float(ref['q'][2, V1 // 3])) < 1e-12 and abs(float(ref['mass'][2]) - 1.0) < 1e-12
                barred = torch.isneginf(s[3])
                assert bool(barred.any()) and not bool(ref['kept'][3][barred].any())
                assert bool(ref['kept'][3, 1]) and bool(torch.isneginf(ref['q'][3][~ref['kept'][3]]).all())
                assert abs(float(ref['q'][3][ref['kept'][3]].exp().sum()) - 1.0) < 1e-12


def test_typical_ties_do_not_depend_on_an_order():
    """two pairs of equal tokens: the pair at s* is kept whole although the first of them already reaches tau"""
    x = torch.tensor([[0.3, 0.3, 0.2, 0.2]], dtype=R.F64).log()
    H = float(R.stats(x, 1.0)[2][0])
    assert abs(-math.log(0.3) - H) < abs(-math.log(0.2) - H)
    assert R.truncate_ref(x, 'typ', 0.25, 1.0)['kept'][0].tolist() == [True, True, False, False]
    assert R.truncate_ref(x, 'typ', 0.7, 1.0)['kept'][0].tolist() == [True] * 4
    assert R.truncate_ref(x[:, [2, 0, 3, 1]], 'typ', 0.25, 1.0)['kept'][0].tolist() == [False, True, False, True]


def test_builders_plant_the_margins():
    for V1 in (2, 5, 65, 1031):
        for kind in R.KINDS:
            for i, param in enumerate(R.PARAMS[kind]):
                T = (1.0, 0.7)[i]
                x = R.rows_for(3, V1, kind, param, T, 10 * V1 + i)
                assert x.dtype == torch.float32 and x.shape == (3, V1)
                assert R.check_margins(x, kind, param, T) >= R.GAP
    # an unplanted row inside the margin is caught
    x = torch.tensor([[0.5, 0.0500001, 0.4499999]]).log()
    with pytest.raises(AssertionError):
        R.check_margins(x, 'minp', 0.1, 1.0)


def test_host_loop_restatement_follows_the_rule():
    """a scripted decoder: minp1 picks the arg-max whatever the noise, rows end at token 0 and stay ended"""
    V1, L, N = 7, 4, 3
    g = R.gen(3)
    table = torch.randn(L, N, V1, generator=g, dtype=R.F64) * 2
    table[1, 0, 0] = 50.0                                    # row 0 ends at step 1
    noise = torch.randn(L, N, V1, generator=g)
    seq, lps, was, gap = R.sample_loop(lambda t, it: table[t], N, N, V1, L, 'minp', 1.0, 1.0, noise)
    assert seq[:, 0].tolist() == table[0].argmax(1).tolist() and seq[0].tolist()[1:] == [0, 0, 0]
    assert was[0].tolist() == [True, True, False, False] and gap == float('inf')      # a one-token kept set has no runner-up
    assert torch.allclose(lps[:, 2], torch.log_softmax(table[2], 1))


# ------------------------------------------------------------------------------------------------ the prototype
def test_ctypes_prototype_matches_the_header():
    import ctypes as C
    from imagecaptioning.pytorch_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'\bint\s+capmi_truncate_rows\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
    assert m, 'capmi_truncate_rows is not declared in include/capmi.h'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]

    def ctype(decl):
        if '*' in decl:
            return C.c_void_p
        return {'int': C.c_int, 'float': C.c_float, 'int64_t': C.c_int64}[decl.rsplit(' ', 1)[0].replace('const ', '')]
    assert [ctype(a) for a in args] == _lib.SIGNATURES['capmi_truncate_rows'], args
    assert [a.rsplit(' ', 1)[1].lstrip('*') for a in args] == ['logp', 'ld', 'q', 'ld_q', 'N', 'V1', 'kind', 'param', 'temperature', 'kept',
                                                               'kept_mass', 'store', 'store_ld', 'unfinished', 'stream']
    for k, v in (('MINP', 0), ('EPS', 1), ('ETA', 2), ('TYP', 3), ('STREAM', 256)):
        assert int(re.search(r'#define CAPMI_TRUNCATE_%s (\d+)' % k, src).group(1)) == v == getattr(_lib, 'TRUNCATE_' + k)
    assert R.KIND_ID == {'minp': _lib.TRUNCATE_MINP, 'eps': _lib.TRUNCATE_EPS, 'eta': _lib.TRUNCATE_ETA, 'typ': _lib.TRUNCATE_TYP}
    assert R.STREAM == _lib.TRUNCATE_STREAM
    assert _lib.lib.capmi_truncate_rows.argtypes == _lib.SIGNATURES['capmi_truncate_rows']
