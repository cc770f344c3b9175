"""Float64 restatements, on the CPU, of the token-selection family of csrc/sampler.hip (log-softmax + top-k / nucleus filter + token
choice + rollout bookkeeping + next-step embedding, the sparse log-softmax backward, the reward criterion) plus the case tables and
input builders that test_select_host.py and test_select_gpu.py share.  Nothing of the package is imported here: the semantics are
those of include/capmi.h and of the reference lines it cites (CaptionModel.py:370-407 sample_next_word, AttModel.py:333-350 _sample,
AttModel.py:436-447 _diverse_sample, losses.py:18-37 RewardCriterion).

Every decision a case asks of the kernel is robust BY CONSTRUCTION of its inputs, so no case and no share of cases is excused:
  * top-k: the k-th and (k+1)-th largest logits of every row are at least TOPK_GAP = 1e-2 apart;
  * nucleus: the float64 cumulative masses of the tempered softmax stay at least MASS_GAP = 1e-3 away from p;
  * winner: the float64 top-two scores of the kept set are at least WIN_GAP = 1e-3 apart (injected Gumbel noise is raised until so).
These are conditions on the inputs, three orders of magnitude above the float32 error of the log-probs at these magnitudes (2e-5,
test_kernels_gpu.py test_logsoftmax_select_modes), not tolerances of the kernel.  check_margins() asserts them."""
import numpy as np
import torch

F64 = torch.float64
TOPK_GAP, MASS_GAP, WIN_GAP = 1e-2, 1e-3, 1e-3
L = 3                     # steps of every select case
EDIM = 10                 # width of the next-step embedding of every select case
RAW = 256                 # CAPMI_SELECT_RAW
ROW_MODES = (0, 1, 2, 1, 0, 2)
# tempered softmax masses planted for the nucleus cases, largest first; the other tokens of a row share what is left (0.01).
# Cumulative masses 0.40 0.65 0.80 0.90 0.94 0.97 0.99: p = 0.3 keeps 1 token, p = 0.7 keeps 3, p = 0.95 keeps 6 (two of the tail).
HEAD = (0.40, 0.25, 0.15, 0.10, 0.04, 0.03, 0.02)
# capmi_select_logp with p = 0.7 and T = 1 (the row is used as it is: tempered value == input float, bit for bit): the first dropped
# token is the float right below the last kept one, so a threshold off by ONE KEY in the radix descent changes the kept set.  The
# log-softmax entries cannot carry such a case: there the kernels subtract their own float32 logsumexp first, and whether two
# adjacent floats stay apart after that rounding (ties to even) is below the resolution the log-probs are held to.
ADJ_HEAD = (0.40, 0.25, 0.15, 0.15, 0.02, 0.01, 0.01)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the select, restated
def kept_set(xt, top_k, top_p):
    """bool [N, V1]: the tokens a mode-1 row may draw.  xt = tempered log-probs (any per-row shift).
    top-k: the k largest values (a value equal to the k-th largest is kept: an exact tie there keeps more than k).
    nucleus: token j of the descending order is kept iff the mass before it is < p; the first always is."""
    if top_k > 0:
        kth = torch.sort(xt, 1, descending=True)[0][:, min(top_k, xt.shape[1]) - 1]
        return xt >= kth[:, None]
    if top_p > 0:
        pr = torch.softmax(xt, 1)
        sp, si = torch.sort(pr, 1, descending=True)
        before = torch.cat([torch.zeros_like(sp[:, :1]), sp.cumsum(1)[:, :-1]], 1)
        keep_sorted = before < top_p
        keep_sorted[:, 0] = True
        return torch.zeros_like(keep_sorted).scatter(1, si, keep_sorted)
    return torch.ones_like(xt, dtype=torch.bool)


def assemble(slabs, bias):
    """the logits row: sum of the K-slice slabs [S, N, V1] plus the bias [V1]"""
    row = slabs.to(F64).sum(0)
    return row + bias.to(F64) if bias is not None else row


def select_ref(d):
    """d: a dict of select_inputs() / logp_inputs().  Returns the float64 statement of everything one select launch writes.
    prenorm (capmi_select_logp): the row already holds log-probabilities and is stored and gathered as it is."""
    row = assemble(d['slabs'], d['bias'])
    N, V1 = row.shape
    prenorm, raw = d.get('prenorm', 0), d.get('raw', 0)
    lp = row if prenorm else torch.log_softmax(row, 1)
    xt = lp / d['T']
    kept = kept_set(xt, d['top_k'], d['top_p'])
    modes, step = d['modes'], d['step']
    score = torch.full_like(xt, float('-inf'))
    chosen = torch.zeros(N, dtype=torch.long)
    for r in range(N):
        m = int(modes[r])
        if m == 0:
            score[r] = row[r]
            chosen[r] = int(torch.nonzero(row[r] == row[r].max())[0])          # lowest index of the maximum
        elif m == 1:
            score[r] = torch.where(kept[r], xt[r] + d['gumbel'][r].to(F64), score[r])
            chosen[r] = int(torch.nonzero(score[r] == score[r].max())[0])
        else:
            chosen[r] = int(d['forced'][r, step])
    unf_in = d['unfinished'].bool()
    was_unf = torch.ones(N, dtype=torch.bool) if (step == 0 or d['no_finish_mask']) else unf_in.clone()
    token = torch.where(was_unf, chosen, torch.zeros_like(chosen))              # pad = 0
    keep = was_unf.to(F64)
    stored = row if (raw or prenorm) else lp
    if prenorm:
        dense = torch.where(was_unf[:, None], stored, stored * 0.0)            # logprobs * unfinished: -inf * 0 = NaN
    else:
        dense = stored * keep[:, None]
    ar = torch.arange(N)
    sel = keep * stored[ar, token]
    if prenorm == 2:
        # _diverse_sample stores sampleLogprobs of sample_next_word unmasked: greedy the row's maximum, sample the tempered
        # entry, top-k the tempered entry (CaptionModel.py:401-406), nucleus the log of the RENORMALISED truncated
        # distribution (CaptionModel.py:396-398, 406)
        sel = row[ar, chosen].clone()
        for r in range(N):
            if int(modes[r]) == 1:
                sel[r] = xt[r, chosen[r]]
                if d['top_p'] > 0:
                    pr = torch.softmax(xt[r], 0)
                    sel[r] = torch.log(pr[chosen[r]] / pr[kept[r]].sum())
    goes_on = was_unf & (token != 0)
    out = dict(row=row, lp=lp, xt=xt, kept=kept, score=score, chosen=chosen, was_unf=was_unf, token=token, it_next=token,
               live=was_unf.to(torch.uint8), dense=dense, sel_logp=sel,
               unfinished=d['unfinished'].clone() if d['no_finish_mask'] else goes_on.to(torch.uint8),
               alive=int(bool(d['no_finish_mask']) or bool(goes_on.any())))
    if d.get('E') is not None:
        x = d['E'][token]                                                       # float32, exact: one relu, one multiply
        if d['relu']:
            x = x.clamp_min(0)
        out['x_next'] = x * d['mask'] if d['mask'] is not None else x
    return out


def top2_gap(v):
    s = torch.sort(v, descending=True)[0]
    return float(s[0] - s[1]) if v.numel() > 1 else float('inf')


def check_margins(d, ref=None):
    """the three margins of a select case: (top-k boundary, nucleus boundary, winner); inf where a margin does not apply"""
    ref = ref or select_ref(d)
    N, V1 = ref['row'].shape
    k, p = d['top_k'], d['top_p']
    tie = d.get('tie_rows', ())
    g_topk = g_mass = g_win = float('inf')
    for r in range(N):
        m = int(d['modes'][r])
        if m == 1 and 0 < k < V1 and r not in tie:
            s = torch.sort(ref['row'][r], descending=True)[0]
            g_topk = min(g_topk, float(s[k - 1] - s[k]))
        if m == 1 and p > 0:
            cum = torch.sort(torch.softmax(ref['xt'][r], 0), descending=True)[0].cumsum(0)
            g_mass = min(g_mass, float((cum - p).abs().min()), p)
        if m != 2 and r not in tie:
            fin = ref['score'][r][torch.isfinite(ref['score'][r])]
            g_win = min(g_win, top2_gap(fin))
    assert g_topk >= TOPK_GAP and g_mass >= MASS_GAP and g_win >= WIN_GAP, (g_topk, g_mass, g_win)
    return g_topk, g_mass, g_win


# ------------------------------------------------------------------------------------------------ Philox, restated
def philox_uniform_bits(seed, ctr_lo, ctr_hi):
    """Philox4x32-10 as csrc/capmi_common.h states it: key = (seed lo, seed hi), counter = (ctr_lo lo, hi, ctr_hi lo, hi);
    numpy uint64 arrays hold the 32-bit words.  Returns [..., 4] uint32 words."""
    M32 = np.uint64(0xffffffff)
    ctr_lo, ctr_hi = np.broadcast_arrays(np.asarray(ctr_lo, np.uint64), np.asarray(ctr_hi, np.uint64))
    c = [ctr_lo & M32, ctr_lo >> np.uint64(32), ctr_hi & M32, ctr_hi >> np.uint64(32)]
    a, b = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ a, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ b, p0 & M32]
        a = (a + np.uint64(0x9E3779B9)) & M32
        b = (b + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, -1).astype(np.uint32)


def philox_gumbel(seed, epoch, step, N, V1):
    """the Gumbel noise [N, V1] (float64) both select kernels draw for `seed` (+ 0x9E3779B97F4A7C15 * epoch when an epoch word is
    bound): vocabulary quad q of row r is Philox(counter = (step << 32 | r, q)), u = ((word >> 8) + 0.5) / 2^24, g = -log(-log u)"""
    if epoch is not None:
        seed = (seed + 0x9E3779B97F4A7C15 * epoch) & 0xFFFFFFFFFFFFFFFF
    nq = (V1 + 3) // 4
    r = np.arange(N, dtype=np.uint64)[:, None]
    q = np.arange(nq, dtype=np.uint64)[None, :]
    w = philox_uniform_bits(seed, (np.uint64(step) << np.uint64(32)) | r, q)            # [N, nq, 4]
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) / 16777216.0
    return torch.from_numpy(-np.log(-np.log(u)).reshape(N, nq * 4)[:, :V1].copy())


# ------------------------------------------------------------------------------------------------ input builders
def nucleus_rows(N, V1, T, g, head=HEAD):
    """target logits [N, V1] whose tempered softmax has the HEAD masses at random positions above a random tail"""
    assert V1 >= len(head)
    rows = torch.empty(N, V1, dtype=F64)
    for r in range(N):
        m = torch.tensor(head, dtype=F64) + (torch.rand(len(head), generator=g, dtype=F64) - 0.5) * 1e-3
        rest = V1 - len(head)
        if rest:
            tail = torch.rand(rest, generator=g, dtype=F64) + 0.1
            mass = torch.cat([m, tail * (1.0 - m.sum()) / tail.sum()])
        else:
            m[-1] += 1.0 - m.sum()
            mass = m
        perm = torch.randperm(V1, generator=g)
        rows[r, perm] = T * torch.log(mass) + 3.0 * torch.randn((), generator=g, dtype=F64)
    return rows


def split_row(target, S, has_bias, g):
    """float32 slabs [S, N, V1] and bias whose float64 sum is `target` up to one float32 rounding of the last slab"""
    N, V1 = target.shape
    bias = (torch.randn(V1, generator=g) * 0.5) if has_bias else None
    others = torch.randn(S - 1, N, V1, generator=g) * 0.7
    last = target - others.to(F64).sum(0) - (bias.to(F64) if has_bias else 0.0)
    return torch.cat([others, last.float()[None]], 0), bias


def adjacent_rows(N, V1, g):
    """float32 log-probs [N, V1] with the ADJ_HEAD masses; the 4th largest entry is the float right below the 3rd largest"""
    x = torch.log_softmax(nucleus_rows(N, V1, 1.0, g, ADJ_HEAD), 1).float()
    order = torch.sort(x, 1, descending=True)[1]
    for r in range(N):
        x[r, order[r, 3]] = torch.nextafter(x[r, order[r, 2]], torch.tensor(float('-inf')))
        assert -2.0 < float(x[r, order[r, 3]]) < float(x[r, order[r, 2]]) < -1.0
    return x


def boost_boundary(d):
    """every other sampled row of a filtered case: the LAST KEPT token gets noise 20 and the FIRST DROPPED token noise 30, so the
    last kept token wins, a kept set one token too large elects the dropped one and a set one token too small another one"""
    if not (d['top_k'] or d['top_p']):
        return
    ref = select_ref(d)
    for r in [r for r in range(len(d['modes'])) if int(d['modes'][r]) == 1][::2]:
        k, xt = ref['kept'][r], ref['xt'][r]
        if bool(k.all()):
            continue
        d['gumbel'][r, xt.masked_fill(~k, float('inf')).argmin()] = 20.0
        d['gumbel'][r, xt.masked_fill(k, float('-inf')).argmax()] = 30.0


def plant_noise(d, modes):
    """Gumbel noise [N, V1] float32 with the winner of every mode-1 row WIN_GAP clear of the runner-up"""
    for _ in range(64):
        ref = select_ref(d)
        low = [r for r in range(len(modes)) if int(modes[r]) == 1 and
               top2_gap(ref['score'][r][torch.isfinite(ref['score'][r])]) < WIN_GAP]
        if not low:
            return
        for r in low:
            d['gumbel'][r, ref['chosen'][r]] += 2 * WIN_GAP
    raise AssertionError('winner margin not reached')


def select_inputs(case, seed):
    N, V1, S, has_bias, offset, mode, T, top_k, top_p, step, flags, _ = case
    fl = set(flags.split())
    g = gen(1000 + seed)
    modes = torch.tensor(ROW_MODES[:N] if mode == 'mix' else [mode] * N)
    if top_p > 0:
        target = nucleus_rows(N, V1, T, g)
    else:
        target = torch.randn(N, V1, generator=g, dtype=F64) * 2.0
        if 0 < top_k < V1:                        # the k largest of every row move up: the boundary gap is at least 2 * TOPK_GAP
            idx = torch.topk(target, top_k, 1)[1]
            target.scatter_add_(1, idx, torch.full(idx.shape, 2 * TOPK_GAP, dtype=F64))
    for r in range(N):                            # greedy rows: the maximum stands clear
        if int(modes[r]) == 0 and top2_gap(target[r]) < 10 * WIN_GAP:
            target[r, target[r].argmax()] += 10 * WIN_GAP
    tie_rows = ()
    if 'tie0' in fl:                              # exact tie of the maximum: the lowest index wins (torch.max on the CPU)
        assert S == 1 and not has_bias and mode == 0
        target[N // 2, V1 - 2] = target[N // 2, 1] = 50.0
        tie_rows = (N // 2,)
    slabs, bias = split_row(target, S, has_bias, g)
    forced = torch.randint(1, V1, (N, L), generator=g)
    if 'allend' in fl:
        forced.zero_()
    elif N > 1:
        forced[N - 1, step] = 0                   # a forced row that ends here
    unf = torch.ones(N, dtype=torch.uint8)
    if 'fin' in fl:
        unf[1 % N] = 0
    if 'nofinish' in fl:
        unf[:] = torch.tensor(([0, 1] * N)[:N], dtype=torch.uint8)
    E = torch.randn(V1, EDIM, generator=g)
    d = dict(slabs=slabs, bias=bias, modes=modes, mode=mode, T=T, top_k=top_k, top_p=top_p, step=step, forced=forced,
             unfinished=unf, no_finish_mask=int('nofinish' in fl), raw=int('raw' in fl), offset=offset, tie_rows=tie_rows,
             gumbel=-torch.log(-torch.log(torch.rand(N, V1, generator=g).clamp_min(1e-20))),
             E=E, mask=None if 'nomask' in fl else (torch.rand(N, EDIM, generator=g) < 0.5).float() * 2, relu=int('relu' in fl),
             planes='planes' in fl)
    boost_boundary(d)
    plant_noise(d, modes)
    check_margins(d)
    return d


_F = [(0, 0.0), (1, 0.0), (7, 0.0), (-1, 0.0), (0, 0.3), (0, 0.7), (0, 0.95)]       # top_k = -1 stands for top_k = V1


def _cases():
    c = [
        # N, V1, splits, bias, offset, mode, T, top_k, top_p, step, flags, kernel and arm the row is meant to reach
        (3, 7, 1, 0, '', 1, 1.0, 0, 0.0, 1, 'relu', 'streaming: V1 % 4 != 0, last Philox quad partly past V1'),
        (3, 7, 2, 1, '', 1, 0.7, 7, 0.0, 1, 'fin', 'streaming: V1 % 4 != 0, top-k = V1'),
        (3, 4099, 3, 1, '', 1, 0.7, 7, 0.0, 1, 'fin relu planes', 'streaming: V1 % 4 != 0, more than one pass of 1024 threads'),
        (2, 4099, 2, 0, '', 1, 1.0, 0, 0.95, 2, '', 'streaming: V1 % 4 != 0, nucleus into the tail'),
        (2, 12292, 2, 1, '', 1, 1.0, 0, 0.7, 1, 'relu', 'streaming: V1 % 4 == 0, aligned, one quad past NQ = 3'),
        (2, 12292, 1, 0, '', 1, 0.7, 7, 0.0, 0, 'fin', 'streaming: past NQ = 3, top-k'),
        (3, 8, 1, 0, '', 1, 1.0, 0, 0.0, 1, 'relu planes', 'register NQ = 1: two live threads'),
        (3, 8, 2, 1, '', 1, 0.7, 7, 0.0, 1, 'fin', 'register NQ = 1: top-k one below V1'),
        (2, 4096, 2, 1, '', 1, 0.7, 0, 0.7, 1, 'fin', 'register NQ = 1 at its limit: every thread one quad'),
        (2, 4096, 1, 0, '', 1, 1.0, 7, 0.0, 2, 'relu', 'register NQ = 1 at its limit, top-k'),
        (2, 4100, 2, 1, '', 1, 1.0, 0, 0.95, 1, '', 'register NQ = 2, one quad past NQ = 1: 1023 clamped padding quads'),
        (2, 8192, 2, 0, '', 1, 0.7, 7, 0.0, 1, 'fin relu', 'register NQ = 2 at its limit'),
        (2, 8192, 3, 1, '', 1, 1.0, 0, 0.3, 0, '', 'register NQ = 2 at its limit, nucleus keeps one token'),
        (2, 8196, 2, 1, '', 1, 0.7, 0, 0.7, 1, 'relu', 'register NQ = 3, one quad past NQ = 2'),
        (2, 12288, 2, 1, '', 1, 1.0, 7, 0.0, 1, 'fin', 'register NQ = 3 at its limit'),
        (2, 12288, 1, 0, '', 1, 0.7, 0, 0.95, 2, 'relu planes', 'register NQ = 3 at its limit, nucleus into the tail'),
        (3, 8, 2, 1, 'ptr', 1, 0.7, 7, 0.0, 1, 'fin', 'streaming: aligned V1, logits one float off 16 bytes'),
        (2, 4096, 3, 1, 'ptr', 1, 1.0, 0, 0.7, 1, 'relu', 'streaming: aligned V1, logits one float off 16 bytes'),
        (3, 8, 2, 1, 'stride', 1, 1.0, 0, 0.7, 1, '', 'streaming: aligned V1 and pointers, slab_stride % 4 != 0'),
        (2, 4096, 5, 0, 'stride', 1, 0.7, 7, 0.0, 1, 'fin', 'streaming: aligned V1 and pointers, slab_stride % 4 != 0'),
    ]
    # the slab assembly: first-four arm alone (1, 4), first s0 group with one (5) or three (7) live slabs, second s0 group with
    # one live slab (8) -- register kernel NQ = 2 (V1 = 4100), and the streaming kernel's plain loop (V1 = 4099)
    arm = {1: 'first four, three multiplied away', 4: 'first four all live', 5: 'first s0 group, one live slab',
           7: 'first s0 group, three live slabs', 8: 'second s0 group, one live slab'}
    for V1, kern in ((4100, 'register NQ = 2'), (4099, 'streaming')):
        for S in (1, 4, 5, 7, 8):
            for b in (0, 1):
                c.append((2, V1, S, b, '', 1, 1.0, 7 if b else 0, 0.0, 1, 'relu' if S & 1 else '',
                          '%s: splits = %d (%s), %s bias' % (kern, S, arm[S], 'with' if b else 'no')))
    # every filter at both temperatures, mode 1, on both kernels
    for V1, kern in ((4100, 'register NQ = 2'), (4099, 'streaming')):
        for T in (1.0, 0.7):
            for k, p in _F:
                c.append((3, V1, 2, 1, '', 1, T, V1 if k < 0 else k, p, 1, 'fin',
                          '%s: mode 1, top_k = %s, top_p = %s, T = %s' % (kern, 'V1' if k < 0 else k, p, T)))
    # modes 0 and 2 never look at the filter or the temperature
    for V1, kern in ((4100, 'register NQ = 2'), (4099, 'streaming')):
        for mode in (0, 2):
            for T, (k, p) in ((1.0, (0, 0.0)), (0.7, (1, 0.0)), (0.7, (7, 0.0)), (1.0, (-1, 0.0)), (1.0, (0, 0.3)), (0.7, (0, 0.7)),
                              (1.0, (0, 0.95))):
                c.append((3, V1, 2, 1, '', mode, T, V1 if k < 0 else k, p, 1, 'fin relu',
                          '%s: mode %d ignores top_k = %s, top_p = %s, T = %s' % (kern, mode, 'V1' if k < 0 else k, p, T)))
    for V1, kern in ((4100, 'register NQ = 2'), (4099, 'streaming'), (8, 'register NQ = 1'), (7, 'streaming')):
        c += [
            (6, V1, 3, 1, '', 'mix', 0.7, 7 if V1 > 8 else 3, 0.0, 1, 'fin relu planes', kern + ': row_mode mixes modes 0, 1, 2; finished row'),
            (6, V1, 3, 1, '', 'mix', 0.7, 0, 0.7, 0, 'fin', kern + ': the same flags at step 0, where they are ignored'),
            (4, V1, 2, 1, '', 1, 1.0, 0, 0.0, 1, 'nofinish', kern + ': no_finish_mask, flags neither read nor written'),
            (4, V1, 2, 0, '', 2, 1.0, 0, 0.0, 1, 'nofinish relu', kern + ': teacher forcing with no_finish_mask'),
            (4, V1, 2, 1, '', 1, 0.7, 3, 0.0, 1, 'raw fin', kern + ': CAPMI_SELECT_RAW, sampled'),
            (4, V1, 1, 0, '', 0, 1.0, 0, 0.0, 1, 'raw fin relu', kern + ': CAPMI_SELECT_RAW, greedy'),
            (3, V1, 1, 0, '', 0, 1.0, 0, 0.0, 1, 'tie0', kern + ': exact tie of the maximum, lowest index wins'),
            (3, V1, 2, 1, '', 2, 1.0, 0, 0.0, 1, 'allend nomask', kern + ': every row ends, alive stays 0; no mask'),
        ]
    return c


SELECT_CASES = _cases()


def kernel_of(case):
    """which kernel capmi_logsoftmax_select_partial's conditions give the case (the comment column says the same in words)"""
    N, V1, S, has_bias, offset = case[:5]
    return 'register' if (offset == '' and V1 % 4 == 0 and V1 <= 12288) else 'streaming'


# a top-k row with an exact tie AT the k-th value: (V1, k).  torch.topk (CaptionModel.py:402) keeps k tokens and breaks the tie by
# position, the kernels keep every token >= the k-th largest; only membership in that set can be asked of either.
TOPK_TIE = [(4100, 7), (4099, 7), (8, 3), (7, 3)]


def topk_tie_inputs(V1, k, seed):
    N = 3
    g = gen(2000 + seed)
    row = (torch.randn(N, V1, generator=g) * 2.0)
    order = torch.sort(row, 1, descending=True)[1]
    for r in range(N):
        row[r, order[r, :k - 1]] += 1.0
        row[r, order[r, k]] = row[r, order[r, k - 1]]                      # k-th == (k+1)-th, bit for bit
        row[r, order[r, k + 1:]] -= 1.0
    gum = -torch.log(-torch.log(torch.rand(N, V1, generator=g).clamp_min(1e-20)))
    allowed = row >= torch.sort(row, 1, descending=True)[0][:, k - 1:k]
    assert allowed.sum(1).tolist() == [k + 1] * N
    return row, gum, allowed


# twins: the same aligned case through both kernels (the second time one float off 16 bytes), in-kernel Philox
# (V1, top_k, top_p); N = 6, splits = 2 with a bias, T = 0.7, step = 1, epoch word bound
TWIN_CASES = [(V1, k, p) for V1 in (4096, 8192, 12288) for k, p in ((0, 0.0), (7, 0.0), (0, 0.7))]
TWIN_SEED, TWIN_EPOCH, TWIN_STEP, TWIN_N, TWIN_T = 77, 5, 1, 6, 0.7


def twin_inputs(i):
    V1, k, p = TWIN_CASES[i]
    d = select_inputs((TWIN_N, V1, 2, 1, '', 1, TWIN_T, k, p, TWIN_STEP, '', 'twin'), 500 + i)
    return d


def twin_philox_ref(d, i):
    """the case with the noise the kernels draw themselves: reference and its winner gap (not planted: it is what it is)"""
    N, V1 = d['gumbel'].shape
    e = dict(d, gumbel=philox_gumbel(TWIN_SEED + i, TWIN_EPOCH, TWIN_STEP, N, V1))
    ref = select_ref(e)
    gap = min(top2_gap(ref['score'][r][torch.isfinite(ref['score'][r])]) for r in range(N))
    return e, ref, gap


# ------------------------------------------------------------------------------------------------ capmi_select_logp
# (N, V1, mode, T, top_k, top_p, sel_unmasked, step): rows of log-probs as the constrained decoders leave them (penalised columns,
# -inf entries, not renormalised); row 1 has finished
LOGP_CASES = [
    (4, 50, 0, 1.0, 0, 0.0, 0, 1), (4, 50, 0, 1.0, 0, 0.0, 1, 1), (4, 50, 1, 1.0, 0, 0.0, 0, 1), (4, 50, 1, 1.0, 0, 0.0, 1, 1),
    (4, 50, 1, 1.0, 5, 0.0, 0, 1), (4, 50, 1, 1.0, 5, 0.0, 1, 1), (4, 50, 1, 1.0, 0, 0.7, 0, 1), (4, 50, 1, 1.0, 0, 0.7, 1, 1),
    (4, 4099, 1, 1.0, 0, 0.7, 1, 2), (4, 4100, 1, 1.0, 5, 0.0, 1, 0), (4, 50, 1, 0.7, 0, 0.7, 1, 1), (4, 50, 1, 0.7, 5, 0.0, 1, 1),
]


def logp_inputs(case, seed):
    N, V1, mode, T, top_k, top_p, unmasked, step = case
    g = gen(3000 + seed)
    if top_p == 0.7 and T == 1.0:                          # the first dropped token one float below the last kept (see ADJ_HEAD)
        x = adjacent_rows(N, V1, g).to(F64)
    elif top_p > 0:
        x = torch.log_softmax(nucleus_rows(N, V1, T, g), 1)
    else:
        x = torch.log_softmax(torch.randn(N, V1, generator=g, dtype=F64) * 2.0, 1)
        if top_k:
            idx = torch.topk(x, top_k, 1)[1]
            x.scatter_add_(1, idx, torch.full(idx.shape, 2 * TOPK_GAP, dtype=F64))
    low = torch.sort(torch.cat([torch.full((N, 1), float('inf'), dtype=F64), x[:, 1:]], 1), 1)[1]       # never the pad column
    for r in range(N):
        x[r, low[r, :3]] = float('-inf')                   # a decoding constraint: the three least likely tokens are barred
        x[r, low[r, 3]] -= 0.5                             # a diversity penalty
    if mode == 0:
        for r in range(N):
            if top2_gap(x[r]) < 10 * WIN_GAP:
                x[r, x[r].argmax()] += 10 * WIN_GAP
    unf = torch.ones(N, dtype=torch.uint8)
    unf[1] = 0
    d = dict(slabs=x.float()[None], bias=None, modes=torch.tensor([mode] * N), mode=mode, T=T, top_k=top_k, top_p=top_p, step=step,
             forced=None, unfinished=unf, no_finish_mask=0, prenorm=2 if unmasked else 1, E=None,
             gumbel=-torch.log(-torch.log(torch.rand(N, V1, generator=g).clamp_min(1e-20))))
    boost_boundary(d)
    plant_noise(d, d['modes'])
    check_margins(d)
    return d


# ------------------------------------------------------------------------------------------------ sparse log-softmax backward
def sparse_bwd_ref(lp_src, tok, g_sel, g_sum, g, scale, raw, live, T):
    """d loss / d logits [T, N, V1] (time-major, as the kernel writes it) by autograd, for
    loss = scale * (sum g_sel * out[tok] + sum g_sum * out.sum(-1)) + sum g * out, out = log_softmax(logits) (raw: the logits
    themselves) over the live (row, step) pairs of the first T steps.  lp_src [N, L, V1] float64 logits."""
    x = lp_src.detach().clone().requires_grad_(True)
    out = x if raw else torch.log_softmax(x, 2)
    N, Lx, V1 = x.shape
    w = live.to(F64)[:, :T] if live is not None else torch.ones(N, T, dtype=F64)
    loss = torch.zeros((), dtype=F64)
    sc = 1.0 if scale is None else float(scale)
    if g_sel is not None:
        loss = loss + sc * (g_sel.to(F64)[:, :T] * w * out[:, :T].gather(2, tok[:, :T, None]).squeeze(2)).sum()
    if g_sum is not None:
        loss = loss + sc * (g_sum.to(F64)[:, :T] * w * out[:, :T].sum(2)).sum()
    if g is not None:
        loss = loss + (g.to(F64)[:, :T] * w[:, :, None] * out[:, :T]).sum()
    loss.backward()
    return x.grad[:, :T].transpose(0, 1).contiguous()


# (N, V1, T, g_sel, g_sum, dense g, scale, raw, dead live row)
SPARSE_CASES = [
    (1, 7, 2, 1, 0, 0, 0, 0, 0), (6, 7, 2, 0, 1, 0, 0, 0, 1), (6, 9488, 2, 1, 1, 1, 1, 0, 1), (1, 9488, 1, 1, 1, 1, 0, 0, 0),
    (6, 7, 2, 1, 1, 1, 1, 1, 1), (6, 9488, 2, 1, 0, 0, 1, 1, 0), (6, 7, 1, 1, 1, 0, 1, 0, 0),
]


def sparse_inputs(case, seed):
    N, V1, T, has_sel, has_sum, has_g, has_scale, raw, dead = case
    g = gen(4000 + seed)
    logits = torch.randn(N, L, V1, generator=g) * 2.0
    saved = logits.clone() if raw else torch.log_softmax(logits.double(), 2).float()     # what the rollout stored
    live = torch.ones(N, L, dtype=torch.uint8)
    if dead:
        live[N // 2, 1:] = 0
    return dict(logits=logits.double() if raw else saved.double(), saved=saved, tok=torch.randint(0, V1, (N, L + 1), generator=g),
                g_sel=torch.randn(N, L, generator=g) if has_sel else None, g_sum=torch.randn(N, L, generator=g) * 0.01 if has_sum else None,
                g=torch.randn(N, L, V1, generator=g) * 0.01 if has_g else None,
                scale=torch.tensor([0.37]) if has_scale else None, raw=raw, live=live if dead else None, T=T)


# ------------------------------------------------------------------------------------------------ reward criterion
def reward_criterion_ref(sel, seq, reward, n_used, n_all, per_row):
    """losses.py:18-37 on the already gathered log-probs: sel [n_all, L], seq [n_all, L], reward [n_used, L] (float64).
    Returns (loss: scalar or [n_used], gcoef [n_all, L] = d sum(loss) / d sel, zero for the rows past n_used)."""
    s = sel[:n_used].detach().clone().requires_grad_(True)
    mask = (seq[:n_used] > 0).to(F64)
    mask = torch.cat([torch.ones(n_used, 1, dtype=F64), mask[:, :-1]], 1)
    out = -s * reward * mask
    loss = out.sum(1) / mask.sum(1) if per_row else out.sum() / mask.sum()
    loss.sum().backward()
    gc = torch.zeros(n_all, sel.shape[1], dtype=F64)
    gc[:n_used] = s.grad
    return loss.detach(), gc


# (N_used, N_all, per_row, reward shape: 'row' = [N] over time through column stride 0 / 'full' = [N, L], seq_ld - L)
REWARD_CASES = [(3, 5, 0, 'row', 0), (5, 5, 0, 'full', 2), (3, 5, 1, 'full', 0), (5, 5, 1, 'row', 2), (3, 5, 0, 'full', 2)]
REWARD_L = 7


def reward_inputs(case, seed):
    n_used, n_all, per_row, shape, pad = case
    g = gen(5000 + seed)
    Lr = REWARD_L
    seq = torch.randint(1, 9, (n_all, Lr + pad), generator=g)
    seq[0, 2:] = 0                                   # a caption that ends early
    seq[1, 0:] = 0                                   # one that ends at once: only the first step counts
    sel = -torch.rand(n_all, Lr, generator=g) * 5
    reward = torch.randn(n_all, generator=g) if shape == 'row' else torch.randn(n_all, Lr, generator=g)
    return dict(sel=sel, seq=seq, reward=reward, n_used=n_used, n_all=n_all, per_row=per_row, L=Lr, seq_ld=Lr + pad)


def reward_full(d):
    """the reward as [n_used, L] float64"""
    r = d['reward'].to(F64)[:d['n_used']]
    return r[:, None].expand(-1, d['L']) if r.dim() == 1 else r
