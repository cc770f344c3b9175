"""The float64 references of select_ref64.py, anchored outside themselves: the kept sets against torch.topk and against the reference's
nucleus lines run literally, the log-probs and the greedy token against F.log_softmax / torch.max, the sparse backward against dense
autograd, the reward criterion against the reference formula -- and the three input margins (top-k boundary, nucleus boundary,
winner) the GPU tests lean on, asserted for every case of every table.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import select_ref64 as S

F64 = torch.float64


def sample_next_word_logprobs(logprobs, top_num, temperature):
    """CaptionModel.sample_next_word's 'top...' branch (CaptionModel.py:386-404) as the reference writes it: the log-probs the
    Categorical draws from"""
    logprobs = logprobs / temperature
    if 0 < top_num < 1:
        probs = F.softmax(logprobs, dim=1)
        sorted_probs, sorted_indices = torch.sort(probs, descending=True, dim=1)
        _cumsum = sorted_probs.cumsum(1)
        mask = _cumsum < top_num
        mask = torch.cat([torch.ones_like(mask[:, :1]), mask[:, :-1]], 1)
        sorted_probs = sorted_probs * mask.to(sorted_probs)
        sorted_probs = sorted_probs / sorted_probs.sum(1, keepdim=True)
        logprobs.scatter_(1, sorted_indices, sorted_probs.log())
    else:
        the_k = int(top_num)
        tmp = torch.empty_like(logprobs).fill_(float('-inf'))
        topk, indices = torch.topk(logprobs, the_k, dim=1)
        tmp = tmp.scatter(1, indices, topk)
        logprobs = tmp
    return logprobs


@pytest.mark.parametrize('i', range(len(S.SELECT_CASES)))
def test_select_case_margins_and_reference(i):
    """every case: the three margins hold; lp is F.log_softmax of the assembled row; the kept set is the support of the
    reference's filtered distribution; the greedy token is torch.max; the bookkeeping follows AttModel.py:340-347"""
    case = S.SELECT_CASES[i]
    N, V1, splits, has_bias, offset, mode, T, top_k, top_p, step, flags, reaches = case
    d = S.select_inputs(case, i)
    ref = S.select_ref(d)
    g_topk, g_mass, g_win = S.check_margins(d, ref)
    assert g_topk >= S.TOPK_GAP and g_mass >= S.MASS_GAP and g_win >= S.WIN_GAP
    assert d['slabs'].shape == (splits, N, V1) and (d['bias'] is not None) == bool(has_bias)
    assert S.kernel_of(case) == ('register' if reaches.startswith('register') else 'streaming')
    row = d['slabs'].double().sum(0) + (d['bias'].double() if has_bias else 0.0)
    lp = F.log_softmax(row, 1)
    assert torch.equal(ref['lp'], lp)
    if top_k or top_p:
        support = torch.isfinite(sample_next_word_logprobs(lp.clone(), top_p if top_p else top_k, T))
        assert torch.equal(ref['kept'], support)
        assert ref['kept'].sum(1).tolist() == [min(top_k, V1) if top_k else {0.3: 1, 0.7: 3, 0.95: 6}[top_p]] * N
    else:
        assert bool(ref['kept'].all())
    for r in range(N):
        m = int(d['modes'][r])
        if m == 0:
            assert int(ref['chosen'][r]) == int(torch.max(row[r:r + 1], 1)[1])
        elif m == 1:
            assert bool(ref['kept'][r, ref['chosen'][r]])
        else:
            assert int(ref['chosen'][r]) == int(d['forced'][r, step])
    if 'tie0' in flags:
        assert int(ref['chosen'][N // 2]) == 1
    if (top_k or top_p) and not bool(ref['kept'].all()):
        # every other sampled row elects its LAST KEPT token, and its first dropped token carries more noise still
        for r in [r for r in range(N) if int(d['modes'][r]) == 1][::2]:
            k, xt = ref['kept'][r], ref['xt'][r]
            assert int(ref['chosen'][r]) == int(xt.masked_fill(~k, float('inf')).argmin())
            assert float(d['gumbel'][r, xt.masked_fill(k, float('-inf')).argmax()]) == 30.0
    # AttModel.py:340-347 in its own words
    it = ref['chosen'].clone()
    if step == 0 or d['no_finish_mask']:
        unfinished = it != 0
        logprobs = lp
    else:
        unfinished = d['unfinished'].bool()
        it[~unfinished] = 0
        logprobs = lp * unfinished.unsqueeze(1).to(lp)
        unfinished = unfinished & (it != 0)
    assert torch.equal(ref['token'], it)
    if not d['raw']:
        assert torch.equal(ref['dense'], logprobs)
    if not d['no_finish_mask']:
        assert torch.equal(ref['unfinished'].bool(), unfinished)
        assert ref['alive'] == int(unfinished.sum() != 0)


def test_kept_sets_against_torch_on_plain_random_rows():
    """no planting: wherever the margins happen to hold on random rows, kept_set is the reference's support"""
    g = S.gen(7)
    x = torch.log_softmax(torch.randn(64, 40, generator=g, dtype=F64) * 2, 1)
    seen = 0
    for T in (1.0, 0.7):
        for k in (1, 5, 40):
            assert torch.equal(S.kept_set(x / T, k, 0.0), torch.isfinite(sample_next_word_logprobs(x.clone(), k, T)))
        for p in (0.3, 0.7, 0.95):
            cum = torch.sort(torch.softmax(x / T, 1), 1, descending=True)[0].cumsum(1)
            ok = (cum - p).abs().min(1)[0] > 1e-9
            seen += int(ok.sum())
            assert torch.equal(S.kept_set(x / T, 0, p)[ok], torch.isfinite(sample_next_word_logprobs(x.clone(), p, T))[ok])
    assert seen > 300


@pytest.mark.parametrize('i', range(len(S.TOPK_TIE)))
def test_topk_tie_rows_hold_k_plus_one_values(i):
    V1, k = S.TOPK_TIE[i]
    row, gum, allowed = S.topk_tie_inputs(V1, k, i)
    assert torch.equal(allowed, S.kept_set(row.double(), k, 0.0))
    idx = torch.topk(row, k, 1)[1]
    assert bool(allowed.gather(1, idx).all())                 # torch.topk's choice lies inside


@pytest.mark.parametrize('i', range(len(S.TWIN_CASES)))
def test_twin_seeds_leave_no_near_tie(i):
    """the seeds of the Philox twins were chosen so that the float64 scores under the restated Philox noise show no gap below
    WIN_GAP: the GPU test may then ask for identical tokens that equal the reference's"""
    d = S.twin_inputs(i)
    S.check_margins(d)
    e, ref, gap = S.twin_philox_ref(d, i)
    assert gap >= S.WIN_GAP, gap
    g = e['gumbel']
    assert bool(torch.isfinite(g).all()) and -3.0 < float(g.min()) and 0.3 < float(g.mean()) < 0.9     # Gumbel(0, 1): mean 0.5772


def test_philox_restatement_known_answer():
    """Philox4x32-10 known-answer vectors of the Random123 distribution (counter, key -> output)"""
    def run(ctr, key):
        w = S.philox_uniform_bits(key[0] | (key[1] << 32), ctr[0] | (ctr[1] << 32), ctr[2] | (ctr[3] << 32))
        return [int(v) for v in w.reshape(4)]
    assert run((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run((0xffffffff,) * 4, (0xffffffff, 0xffffffff)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize('i', range(len(S.LOGP_CASES)))
def test_logp_case_margins_and_reference(i):
    """capmi_select_logp's cases: margins; -inf entries are never kept; sel_unmasked stores sample_next_word's sampleLogprobs"""
    case = S.LOGP_CASES[i]
    N, V1, mode, T, top_k, top_p, unmasked, step = case
    d = S.logp_inputs(case, i)
    ref = S.select_ref(d)
    S.check_margins(d, ref)
    x = d['slabs'][0].double()
    assert int(torch.isinf(x).sum()) == 3 * N
    assert not bool((ref['kept'] & torch.isinf(x)).any()) or not (top_k or top_p)
    assert bool(torch.isfinite(x[torch.arange(N), ref['chosen']]).all())
    if top_p == 0.7 and T == 1.0:            # 4th largest = the float right below the 3rd largest = the last kept token
        v = torch.sort(d['slabs'][0], 1, descending=True)[0]
        assert torch.equal(torch.nextafter(v[:, 2], torch.tensor(float('-inf'))), v[:, 3]) and bool((v[:, 3] < v[:, 2]).all())
        assert ref['kept'].sum(1).tolist() == [3] * N
    if step > 0:
        assert int(ref['token'][1]) == 0 and bool(torch.isnan(ref['dense'][1]).sum() == 3)
    else:                                                                     # step 0 ignores the flag
        assert int(ref['token'][1]) == int(ref['chosen'][1]) and not bool(torch.isnan(ref['dense']).any())
    if unmasked:
        if mode == 0:
            want = torch.max(x, 1)[0]
        elif top_k or top_p:
            want = sample_next_word_logprobs(x.clone(), top_p if top_p else top_k, T).gather(1, ref['chosen'][:, None]).squeeze(1)
        else:
            want = (x / T).gather(1, ref['chosen'][:, None]).squeeze(1)
        assert float((ref['sel_logp'] - want).abs().max()) < 1e-12
    elif step > 0:
        assert float(ref['sel_logp'][1]) == 0.0


@pytest.mark.parametrize('i', range(len(S.SPARSE_CASES)))
def test_sparse_backward_reference_is_dense_autograd(i):
    """sparse_bwd_ref == autograd through a dense gradient tensor (zero fill + scatter + row constant + dense part)"""
    case = S.SPARSE_CASES[i]
    N, V1, T, has_sel, has_sum, has_g, has_scale, raw, dead = case
    if V1 > 100:
        case = (N, 33, T, has_sel, has_sum, has_g, has_scale, raw, dead)          # the same combination, a host-sized row
    d = S.sparse_inputs(case, i)
    got = S.sparse_bwd_ref(d['logits'], d['tok'], d['g_sel'], d['g_sum'], d['g'], d['scale'], d['raw'], d['live'], T)
    x = d['logits'].clone().requires_grad_(True)
    out = x if raw else torch.log_softmax(x, 2)
    dense = torch.zeros_like(out)
    sc = float(d['scale']) if has_scale else 1.0
    if has_sel:
        dense.scatter_(2, d['tok'][:, :S.L, None], sc * d['g_sel'].double()[:, :, None])
    if has_sum:
        dense = dense + sc * d['g_sum'].double()[:, :, None]
    if has_g:
        dense = dense + d['g'].double()
    dense[:, T:] = 0
    if dead:
        dense = dense * d['live'].double()[:, :, None]
    out.backward(dense)
    assert got.shape == (T, N, case[1])
    assert float((got - x.grad[:, :T].transpose(0, 1)).abs().max()) < 1e-12
    if dead:
        assert float(got[1:, N // 2].abs().max()) == 0.0


@pytest.mark.parametrize('i', range(len(S.REWARD_CASES)))
def test_reward_criterion_reference_is_the_formula(i):
    """reward_criterion_ref == RewardCriterion.forward (losses.py:22-37) on a dense input whose gathered entries are `sel`"""
    d = S.reward_inputs(S.REWARD_CASES[i], i)
    n, Lr = d['n_used'], d['L']
    loss, gc = S.reward_criterion_ref(d['sel'].double(), d['seq'][:, :Lr], S.reward_full(d), n, d['n_all'], d['per_row'])
    seq = d['seq'][:n, :Lr]
    inp = torch.zeros(n, Lr, 9, dtype=F64).scatter_(2, seq.unsqueeze(2), d['sel'].double()[:n, :, None]).requires_grad_(True)
    reward = S.reward_full(d)
    # the reference's lines
    N, L = inp.shape[:2]
    input = inp.gather(2, seq.unsqueeze(2)).squeeze(2)
    input = input.reshape(-1)
    reward = reward.reshape(-1)
    mask = (seq > 0).to(input)
    mask = torch.cat([mask.new(mask.size(0), 1).fill_(1), mask[:, :-1]], 1).reshape(-1)
    output = - input * reward * mask
    if d['per_row']:
        output = output.view(N, L).sum(1) / mask.view(N, L).sum(1)
    else:
        output = torch.sum(output) / torch.sum(mask)
    output.sum().backward()
    assert float((loss - output.detach()).abs().max()) < 1e-12
    assert float((gc[:n] - inp.grad.gather(2, seq.unsqueeze(2)).squeeze(2)).abs().max()) < 1e-12
    assert float(gc[n:].abs().max()) == 0.0 if d['n_all'] > n else True
    assert float(mask.view(N, L).sum(1).min()) == 1.0          # a caption that ends at once still counts its first step
