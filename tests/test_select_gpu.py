"""The token-selection family of csrc/sampler.hip through the C ABI against the float64 references of select_ref64.py: one case per
dispatch arm of capmi_logsoftmax_select_partial (register-resident NQ = 1 / 2 / 3 against streaming; V1 % 4, pointer and slab-stride
alignment; the slab-assembly arms), every mode and filter, the bookkeeping flags, the next-step embedding tail; the two kernels
against each other under the in-kernel Philox; the filtered sampling distribution; capmi_select_logp on constrained rows; the sparse
log-softmax backward and the reward criterion.

Tokens and flags are compared exactly -- the case builders plant every decision 1e-3 or more clear in float64 (select_ref64.py) --
dense rows and selected log-probs by max |got - ref| < 2e-5 (the bound of test_kernels_gpu.py test_logsoftmax_select_modes), the
sparse gradient and the criterion by rel_err of test_kernels_gpu.py with 5e-6 (cell backward) and 2e-6.  Outputs are pre-filled
with NaN / sentinels, so an element a launch did not write shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import select_ref64 as S
from oracle import planes as PL

pytestmark = pytest.mark.gpu

LOGP_TOL, SPARSE_TOL, CRIT_TOL = 2e-5, 5e-6, 2e-6
SENT = -7                     # pre-fill of the integer outputs
# Twins may disagree on a token only where the float64 top-two scores are closer than TWIN_GAP, and on at most TWIN_CAP rows in
# this whole file.  The twin seeds were chosen (test_select_host.py test_twin_seeds_leave_no_near_tie) so that no row has such a
# gap: the allowance is not expected to be used, and the last twin test reports how many rows used it.
TWIN_GAP, TWIN_CAP = 1e-5, 1
twin_rows_excused = []


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def lib_mod():
    from imagecaptioning.pytorch_amd import _lib
    return _lib


def ptr(t):
    return None if t is None else t.data_ptr()


def rel_err(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def put_slabs(dev, slabs, offset):
    """the slabs in one device buffer, NaN between and behind them.  offset 'ptr': the first slab starts one float past a 16-byte
    boundary; 'stride': the slabs lie N * V1 + 1 floats apart"""
    Sn, N, V1 = slabs.shape
    stride = N * V1 + (1 if offset == 'stride' else 0)
    off = 1 if offset == 'ptr' else 0
    buf = torch.full((off + (Sn - 1) * stride + N * V1 + 4,), float('nan'), device=dev)
    assert buf.data_ptr() % 16 == 0
    for s in range(Sn):
        buf[off + s * stride: off + s * stride + N * V1] = slabs[s].reshape(-1).to(dev)
    return buf, buf.data_ptr() + 4 * off, stride


def run_select(dev, d, gumbel='given', seed=0, offset=None):
    """one capmi_logsoftmax_select_partial launch on the case `d` -> its outputs (CPU tensors)"""
    L = lib_mod()
    Sn, N, V1 = d['slabs'].shape
    step = d['step']
    hold, p_slabs, stride = put_slabs(dev, d['slabs'], d['offset'] if offset is None else offset)
    bias = None if d['bias'] is None else d['bias'].to(dev)
    gum = d['gumbel'].to(dev).contiguous() if gumbel == 'given' else None
    mix = d['mode'] == 'mix'
    row_mode = d['modes'].to(torch.uint8).to(dev) if mix else None
    forced = d['forced'].to(dev).contiguous()
    seq = torch.full((N, S.L + 1), SENT, dtype=torch.long, device=dev)            # seq_ld = L + 1
    it = torch.full((N,), SENT, dtype=torch.long, device=dev)
    it_save = torch.full((N,), SENT, dtype=torch.long, device=dev)
    unf = d['unfinished'].to(dev)
    slp = torch.full((N, S.L, V1), float('nan'), device=dev)
    sel = torch.full((N, S.L), float('nan'), device=dev)
    live = torch.full((N, S.L), 9, dtype=torch.uint8, device=dev)
    x_next = torch.full((N, S.EDIM), float('nan'), device=dev)
    alive = torch.zeros(1, dtype=torch.int32, device=dev)
    E = d['E'].to(dev)
    mask = None if d['mask'] is None else d['mask'].to(dev)
    x_pl = torch.zeros(int(L.lib.capmi_planes_bytes(S.EDIM)), dtype=torch.uint8, device=dev) if d.get('planes') else None
    ne = L.NextEmbed()
    ne.E, ne.mask, ne.x, ne.it_save, ne.Edim, ne.relu, ne.x_planes, ne.alive = (ptr(E), ptr(mask), ptr(x_next), ptr(it_save), S.EDIM,
                                                                                d['relu'], ptr(x_pl), ptr(alive))
    flt = L.SampleFilter(int(d['top_k']), float(d['top_p']))
    mode = (0 if mix else int(d['mode'])) | (S.RAW if d['raw'] else 0)
    L.check(L.lib.capmi_logsoftmax_select_partial(p_slabs, Sn, stride, ptr(bias), N, V1, step, S.L, mode, ptr(row_mode), float(d['T']),
                                                  ptr(gum), seed, ptr(forced), S.L, d['no_finish_mask'], ptr(seq), S.L + 1, ptr(it),
                                                  ptr(unf), ptr(slp), ptr(sel), ptr(live), C.byref(ne),
                                                  C.byref(flt) if (d['top_k'] or d['top_p']) else None, L.stream_ptr()),
            'capmi_logsoftmax_select_partial')
    torch.cuda.synchronize()
    del hold
    return dict(seq=seq.cpu(), it=it.cpu(), it_save=it_save.cpu(), unf=unf.cpu(), slp=slp.cpu(), sel=sel.cpu(), live=live.cpu(),
                x_next=x_next.cpu(), alive=int(alive.cpu()), planes=None if x_pl is None else x_pl.cpu())


def compare(d, ref, out, what=''):
    N, V1 = ref['row'].shape
    step = d['step']
    other = [t for t in range(S.L) if t != step]
    # exact: tokens and flags, and nothing outside this step's column
    assert torch.equal(out['seq'][:, step], ref['token']), (what, out['seq'][:, step].tolist(), ref['token'].tolist())
    assert bool((out['seq'][:, other + [S.L]] == SENT).all())
    assert torch.equal(out['it'], ref['it_next']) and torch.equal(out['it_save'], ref['token'])
    assert torch.equal(out['unf'], ref['unfinished']), (what, out['unf'].tolist(), ref['unfinished'].tolist())
    assert torch.equal(out['live'][:, step], ref['live']) and bool((out['live'][:, other] == 9).all())
    # dense row and selected log-prob
    got = out['slp'][:, step].double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isnan(out['slp'][:, other]).all())
    e_dense = float((got - ref['dense']).abs().max())
    e_sel = float((out['sel'][:, step].double() - ref['sel_logp']).abs().max())
    print('%s dense %.2e sel_logp %.2e (bound %.0e)' % (what, e_dense, e_sel, LOGP_TOL))
    assert e_dense < LOGP_TOL and e_sel < LOGP_TOL
    assert bool((got[~ref['was_unf']] == 0).all()) and bool((out['sel'][:, step][~ref['was_unf']] == 0).all())
    assert bool(torch.isnan(out['sel'][:, other]).all())
    # next-step embedding: exactly relu?(E[token]) * mask, the same values as A planes, the alive word
    assert torch.equal(out['x_next'], ref['x_next'])
    if out['planes'] is not None:
        assert np.array_equal(out['planes'].numpy(), PL.planes_from_f32(ref['x_next'].numpy()))
    assert out['alive'] == ref['alive']


# ------------------------------------------------------------------------------------------------ 1. parity, every case row
@pytest.mark.parametrize('i', range(len(S.SELECT_CASES)))
def test_select_parity(dev, i):
    """capmi_logsoftmax_select_partial on case row i of select_ref64.SELECT_CASES (its last column names the kernel and the arm)
    against select_ref: tokens, flags and the embedding exactly, log-probs within 2e-5"""
    case = S.SELECT_CASES[i]
    d = S.select_inputs(case, i)
    ref = S.select_ref(d)
    compare(d, ref, run_select(dev, d), case[-1])


@pytest.mark.parametrize('i', range(len(S.TOPK_TIE)))
def test_topk_with_an_exact_tie_at_the_kth_value(dev, i):
    """The k-th and (k+1)-th largest logits are the same float.  The reference's torch.topk (CaptionModel.py:402) keeps exactly k
    tokens and breaks such a tie BY POSITION (which of the two it keeps is an implementation detail of the sort); the kernels keep
    every token >= the k-th largest value.  So only this is asserted: the token lies among the values >= the k-th largest."""
    V1, k = S.TOPK_TIE[i]
    row, gum, allowed = S.topk_tie_inputs(V1, k, i)
    N = row.shape[0]
    d = dict(slabs=row[None], bias=None, modes=torch.ones(N, dtype=torch.long), mode=1, T=1.0, top_k=k, top_p=0.0, step=0,
             forced=torch.zeros(N, S.L, dtype=torch.long), unfinished=torch.ones(N, dtype=torch.uint8), no_finish_mask=0, raw=0,
             offset='', gumbel=gum, E=torch.zeros(V1, S.EDIM), mask=None, relu=0)
    for noise in (gum, torch.zeros_like(gum), gum.flip(1)):
        out = run_select(dev, dict(d, gumbel=noise))
        tok = out['seq'][:, 0]
        assert bool(allowed[torch.arange(N), tok].all()), (tok.tolist(), allowed.nonzero().tolist())


# ------------------------------------------------------------------------------------------------ 2. kernel twins
def twin_agree(a, b, ref, what):
    """tokens of the two kernels: identical, or -- TWIN_CAP rows in the file at most -- apart on a float64 near-tie below TWIN_GAP"""
    for r in np.nonzero((a != b).numpy())[0]:
        sa, sb = float(ref['score'][r, a[r]]), float(ref['score'][r, b[r]])
        print('%s row %d: register token %d score %.9f, streaming token %d score %.9f' % (what, r, a[r], sa, int(b[r]), sb))
        assert abs(sa - sb) < TWIN_GAP, (what, r, sa, sb)
        twin_rows_excused.append((what, int(r)))
    assert len(twin_rows_excused) <= TWIN_CAP, twin_rows_excused


@pytest.mark.parametrize('i', range(len(S.TWIN_CASES)))
def test_register_and_streaming_kernels_draw_the_same_tokens(dev, i):
    """The same aligned case (NQ = 1, 2, 3; no filter, top-k, nucleus) through the register-resident kernel and -- the logits one
    float off 16 bytes -- through the streaming kernel.  In-kernel Philox with an epoch word bound: 'identical Philox counters and
    identical samples' (sampler.hip), and both equal the float64 reference under the restated Philox noise, whose top-two gap the
    host test holds above 1e-3 for these seeds.  Then the same with injected noise."""
    L = lib_mod()
    d = S.twin_inputs(i)
    assert S.kernel_of((S.TWIN_N, S.TWIN_CASES[i][0], 2, 1, '')) == 'register'
    e, ref_p, gap = S.twin_philox_ref(d, i)
    assert gap >= S.WIN_GAP
    epoch = torch.tensor([S.TWIN_EPOCH], dtype=torch.int64, device=dev)
    prev = C.c_void_p()
    L.check(L.lib.capmi_rng_bind_epoch(epoch.data_ptr(), C.byref(prev)), 'capmi_rng_bind_epoch')
    try:
        a = run_select(dev, d, gumbel=None, seed=S.TWIN_SEED + i, offset='')
        b = run_select(dev, d, gumbel=None, seed=S.TWIN_SEED + i, offset='ptr')
    finally:
        L.check(L.lib.capmi_rng_bind_epoch(prev.value, None), 'capmi_rng_bind_epoch')
    step = d['step']
    twin_agree(a['seq'][:, step], b['seq'][:, step], ref_p, 'philox %s' % (S.TWIN_CASES[i],))
    assert torch.equal(a['seq'][:, step], ref_p['token']), (a['seq'][:, step].tolist(), ref_p['token'].tolist())
    compare(e, ref_p, a, 'philox register')
    ref = S.select_ref(d)
    a, b = run_select(dev, d, offset=''), run_select(dev, d, offset='ptr')
    twin_agree(a['seq'][:, step], b['seq'][:, step], ref, 'injected %s' % (S.TWIN_CASES[i],))
    compare(d, ref, a, 'injected register')
    compare(d, ref, b, 'injected streaming')
    if i == len(S.TWIN_CASES) - 1:
        print('twin rows that used the near-tie allowance: %d of cap %d %s' % (len(twin_rows_excused), TWIN_CAP, twin_rows_excused))


# ------------------------------------------------------------------------------------------------ 3. filtered distribution
@pytest.mark.parametrize('top_k,top_p,offset', [(5, 0.0, ''), (0, 0.7, ''), (5, 0.0, 'ptr'), (0, 0.7, 'ptr')])
def test_philox_sampling_matches_the_filtered_distribution(dev, top_k, top_p, offset):
    """test_philox_sampling_matches_distribution with a filter: V1 = 16, 4096 rows x 8 seeds = 32768 draws, T = 0.7.  Frequencies
    within 0.01 of the renormalised softmax over the kept set (3.6 sigma of the largest binomial deviation at 32768 draws, the
    bound of that test) and exactly 0 outside it; on the register kernel and (offset) the streaming kernel."""
    L = lib_mod()
    V1, N, T = 16, 4096, 0.7
    row = S.nucleus_rows(1, V1, T, S.gen(9)).float()
    lp = torch.log_softmax(row.double(), 1)
    kept = S.kept_set(lp / T, top_k, top_p)[0]
    assert int(kept.sum()) == (5 if top_k else 3)
    hold, p_slabs, stride = put_slabs(dev, row.repeat(N, 1)[None], offset)
    seq = torch.zeros(N, 1, dtype=torch.long, device=dev)
    it = torch.zeros(N, dtype=torch.long, device=dev)
    unf = torch.ones(N, dtype=torch.uint8, device=dev)
    flt = L.SampleFilter(top_k, top_p)
    counts = torch.zeros(V1)
    for s in range(8):
        L.check(L.lib.capmi_logsoftmax_select_partial(p_slabs, 1, stride, None, N, V1, 0, 1, 1, None, T, None, 1234 + s, None, 0, 0,
                                                      ptr(seq), 1, ptr(it), ptr(unf), None, None, None, None, C.byref(flt),
                                                      L.stream_ptr()), 'capmi_logsoftmax_select_partial')
        counts += torch.bincount(seq[:, 0].cpu(), minlength=V1).float()
    freq = counts / counts.sum()
    want = torch.softmax(lp[0] / T, 0) * kept
    want = (want / want.sum()).float()
    print('max |freq - want| %.4f' % float((freq - want).abs().max()))
    assert float((freq - want).abs().max()) < 0.01
    assert float(freq[~kept].max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. capmi_select_logp
@pytest.mark.parametrize('i', range(len(S.LOGP_CASES)))
def test_select_logp(dev, i):
    """capmi_select_logp on rows of constrained log-probs (three -inf entries and a penalised column per row; row 1 finished).  The
    kept set never holds a -inf entry (the token is compared exactly); the stored row of the finished row is NaN where the
    reference's -inf * 0 is and 0 elsewhere.
    sel_unmasked: decode.diverse_sample_steps passes the filter of sample_method 'top<p>' together with sel_unmasked = 1, so the
    nucleus combination is reachable, and the reference stores there the log-prob of the renormalised truncated distribution
    (CaptionModel.py:396-398, 406), not x[chosen]; under top-k and plain sampling it stores x[chosen] / temperature.  select_ref
    states those values and the kernel is held to them."""
    L = lib_mod()
    case = S.LOGP_CASES[i]
    N, V1, mode, T, top_k, top_p, unmasked, step = case
    d = S.logp_inputs(case, i)
    ref = S.select_ref(d)
    x = d['slabs'][0].to(dev).contiguous()
    gum = d['gumbel'].to(dev).contiguous()
    seq = torch.full((N, S.L), SENT, dtype=torch.long, device=dev)
    it = torch.full((N,), SENT, dtype=torch.long, device=dev)
    unf = d['unfinished'].to(dev)
    slp = torch.full((N, S.L, V1), float('nan'), device=dev)
    sel = torch.full((N, S.L), float('nan'), device=dev)
    flt = L.SampleFilter(top_k, top_p)
    L.check(L.lib.capmi_select_logp(ptr(x), N, V1, step, S.L, mode, T, ptr(gum) if mode else None, 0, ptr(seq), S.L, ptr(it), ptr(unf),
                                    ptr(slp), ptr(sel), unmasked, C.byref(flt) if (top_k or top_p) else None, L.stream_ptr()),
            'capmi_select_logp')
    torch.cuda.synchronize()
    assert torch.equal(seq[:, step].cpu(), ref['token']) and torch.equal(it.cpu(), ref['token'])
    assert torch.equal(unf.cpu(), ref['unfinished'])
    got, want = slp[:, step].cpu().double(), ref['dense']
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(got[ok], want[ok])                                       # stored as they are: float32 in, float32 out
    e = float((sel[:, step].cpu().double() - ref['sel_logp']).abs().max())
    print('sel_logp %.2e (bound %.0e)' % (e, LOGP_TOL))
    assert e < LOGP_TOL
    other = [t for t in range(S.L) if t != step]
    assert bool(torch.isnan(sel[:, other]).all()) and bool((seq[:, other] == SENT).all())


# ------------------------------------------------------------------------------------------------ 5. sparse backward, criterion
@pytest.mark.parametrize('i', range(len(S.SPARSE_CASES)))
def test_logsoftmax_bwd_sparse(dev, i):
    """capmi_logsoftmax_bwd_sparse against autograd on log_softmax in float64 (sparse_bwd_ref): rel_err < 5e-6"""
    L = lib_mod()
    case = S.SPARSE_CASES[i]
    N, V1, T = case[:3]
    d = S.sparse_inputs(case, i)
    ref = S.sparse_bwd_ref(d['logits'], d['tok'], d['g_sel'], d['g_sum'], d['g'], d['scale'], d['raw'], d['live'], T)
    t = {k: (None if d[k] is None else d[k].to(dev).contiguous()) for k in ('saved', 'tok', 'g_sel', 'g_sum', 'g', 'scale', 'live')}
    sp = L.SparseLogpGrad()
    sp.g_sel, sp.g_sum, sp.tok, sp.tok_ld, sp.raw, sp.scale = ptr(t['g_sel']), ptr(t['g_sum']), ptr(t['tok']), S.L + 1, d['raw'], ptr(t['scale'])
    out = torch.full((T, N, V1), float('nan'), device=dev)
    L.check(L.lib.capmi_logsoftmax_bwd_sparse(C.byref(sp), ptr(t['g']), ptr(t['saved']), ptr(t['live']), ptr(out), N, S.L, T, V1,
                                              L.stream_ptr()), 'capmi_logsoftmax_bwd_sparse')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    e = rel_err(out, ref)
    print('dlogits rel_err %.2e (bound %.0e)' % (e, SPARSE_TOL))
    assert e < SPARSE_TOL
    if d['live'] is not None:
        assert float(out[1:, N // 2].abs().max()) == 0.0


@pytest.mark.parametrize('i', range(len(S.REWARD_CASES)))
def test_reward_criterion(dev, i):
    """capmi_reward_criterion against losses.py:18-37 in float64 (reward_criterion_ref): loss and coefficients rel_err < 2e-6"""
    L = lib_mod()
    d = S.reward_inputs(S.REWARD_CASES[i], i)
    n, n_all, Lr = d['n_used'], d['n_all'], d['L']
    loss_ref, gc_ref = S.reward_criterion_ref(d['sel'].double(), d['seq'][:, :Lr], S.reward_full(d), n, n_all, d['per_row'])
    sel, seq, rw = d['sel'].to(dev), d['seq'].to(dev).contiguous(), d['reward'].to(dev).contiguous()
    rs, cs = (1, 0) if rw.dim() == 1 else (Lr, 1)
    loss = torch.full((n if d['per_row'] else 1,), float('nan'), device=dev)
    gc = torch.full((n_all, Lr), float('nan'), device=dev)
    L.check(L.lib.capmi_reward_criterion(ptr(sel), Lr, ptr(seq), d['seq_ld'], ptr(rw), rs, cs, n, n_all, Lr, d['per_row'], ptr(loss),
                                         ptr(gc), L.stream_ptr()), 'capmi_reward_criterion')
    torch.cuda.synchronize()
    e_loss, e_gc = rel_err(loss, loss_ref.reshape(-1)), rel_err(gc, gc_ref)
    print('loss rel_err %.2e gcoef rel_err %.2e (bound %.0e)' % (e_loss, e_gc, CRIT_TOL))
    assert e_loss < CRIT_TOL and e_gc < CRIT_TOL
    assert float(gc[n:].abs().max()) == 0.0 if n_all > n else True
