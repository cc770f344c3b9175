"""Float64 restatements, on the CPU, of the truncation samplers of csrc/truncate.hip (min-p, epsilon, eta and locally typical
sampling; include/capmi.h capmi_truncate_rows) and of the two host loops that call them (decode.sample_steps,
decode.diverse_sample_steps), plus the input builders test_truncate_host.py and test_truncate_gpu.py share.  Nothing of the
package is imported here.

The rules, in exact arithmetic: x a row of log-probabilities, p = softmax(x / T), H = -sum p log p (0 log 0 = 0), p_max = max p.
    minp<a>   keep p_v >= a p_max
    eps<e>    keep p_v >= e, and every token with p_v == p_max
    eta<e>    keep p_v >= min(e, sqrt(e) exp(-H)), and every token with p_v == p_max
    typ<tau>  s_v = |-log p_v - H|, s* the smallest score with mass{s_v <= s*} >= tau, keep s_v <= s* (ties at s* all kept)
Entries at -inf have p = 0 and are never kept.  q_v = log(p_v / sum_kept p) on the kept set, -inf elsewhere.

Every decision a case asks of the kernel is robust BY CONSTRUCTION of its inputs (the float32 rows the kernel is handed, judged in
float64), so no row and no token is excused:
  * minp / eps / eta: the log-probability of every token other than the row maximum is at least GAP = 1e-3 away from the log of the
    threshold (1e-3 relative in p: MASS_GAP of select_ref64.py);
  * typ: the score of every token not tied with s* is at least GAP away from s*, the mass strictly below s* is at most tau (1 - GAP)
    and the mass up to s* at least tau (1 + GAP) -- or the whole row is kept.
A float32 log-probability at these magnitudes is good to 2e-5 (select_ref64.py), fifty times below.  plant() moves tokens until the
margins hold and puts one token right behind each side of the boundary (3 GAP off), so that a threshold that is off by more than a
few GAP changes the kept set; check_margins() asserts the margins, on the final float32 rows."""
import math

import torch

F64 = torch.float64
GAP = 1e-3
KINDS = ('minp', 'eps', 'eta', 'typ')
KIND_ID = {'minp': 0, 'eps': 1, 'eta': 2, 'typ': 3}            # CAPMI_TRUNCATE_*
STREAM = 256                                                   # CAPMI_TRUNCATE_STREAM
# two parameters per rule
PARAMS = {'minp': (0.1, 0.5), 'eps': (3e-4, 0.01), 'eta': (2e-3, 0.05), 'typ': (0.9, 0.3)}
NEG_INF = float('-inf')


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the rules, restated
def stats(x, T):
    """log p [N, V1], p, H [N] of float64 rows x"""
    lp = torch.log_softmax(x.to(F64) / T, 1)
    p = lp.exp()
    H = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(1)
    return lp, p, H


def log_threshold(kind, param, lp, H):
    """minp / eps / eta: the log of the probability a token other than the maximum must reach, [N]"""
    if kind == 'minp':
        return math.log(param) + lp.max(1)[0]
    if kind == 'eps':
        return torch.full_like(H, math.log(param))
    return torch.minimum(torch.full_like(H, math.log(param)), 0.5 * math.log(param) - H)


def typical_cut(s, p, tau):
    """one row: (s*, mass strictly below s*, mass up to s*); scores of p = 0 tokens are +inf and carry no mass"""
    order = torch.argsort(s)
    ss, cs = s[order], p[order].cumsum(0)
    le = cs[torch.searchsorted(ss, ss, right=True) - 1]                    # mass{s_v <= ss[i]}
    hit = torch.nonzero(le >= tau)
    if hit.numel() == 0:                                                   # rounding left the whole mass short of tau: keep all
        fin = torch.isfinite(ss)
        return float(ss[fin][-1]), 0.0, float(cs[-1])
    i = int(hit[0])
    first = int(torch.searchsorted(ss, ss[i:i + 1], right=False))
    return float(ss[i]), float(cs[first - 1]) if first > 0 else 0.0, float(le[i])


def truncate_ref(x, kind, param, T=1.0):
    """x [N, V1] -> dict(kept bool [N, V1], count [N], mass [N], q [N, V1], lp, H), all float64"""
    lp, p, H = stats(x, T)
    N, V1 = lp.shape
    if kind == 'typ':
        s = (-lp - H[:, None]).abs()
        kept = torch.zeros(N, V1, dtype=torch.bool)
        for r in range(N):
            cut, _, _ = typical_cut(s[r], p[r], param)
            kept[r] = (s[r] <= cut) & (p[r] > 0)
    else:
        kept = (lp >= log_threshold(kind, param, lp, H)[:, None]) & (p > 0)
        if kind == 'minp':
            kept = (p >= param * p.max(1, keepdim=True)[0]) & (p > 0)
        else:
            kept |= p == p.max(1, keepdim=True)[0]
    mass = torch.where(kept, p, torch.zeros_like(p)).sum(1)
    q = torch.where(kept, lp - mass.log()[:, None], torch.full_like(lp, NEG_INF))
    return dict(kept=kept, count=kept.sum(1), mass=mass, q=q, lp=lp, H=H)


def check_margins(x, kind, param, T=1.0):
    """asserts the decision margins of the module docstring on float32 rows x; returns the smallest one seen (inf: none applies)"""
    lp, p, H = stats(x, T)
    worst = float('inf')
    for r in range(lp.shape[0]):
        live = p[r] > 0
        if kind == 'typ':
            s = (-lp[r] - H[r]).abs()
            cut, below, upto = typical_cut(s, p[r], param)
            if bool(((s <= cut) | ~live).all()) and upto < param:
                continue
            others = live & (s != cut)
            m = [float((s[others] - cut).abs().min())] if bool(others.any()) else []
            m += [(param - below) / param, (upto - param) / param]
        else:
            others = live & (p[r] != p[r].max())
            if not bool(others.any()):
                continue
            m = [float((lp[r][others] - log_threshold(kind, param, lp[r:r + 1], H[r:r + 1])[0]).abs().min())]
        worst = min([worst] + m)
        assert min(m) >= GAP, (kind, param, T, r, m)
    return worst


# ------------------------------------------------------------------------------------------------ input builders
def _raw_rows(N, V1, g, scale):
    """scale * randn rows with a peaked head: the maximum holds between a fifth and two thirds of the mass"""
    x = torch.randn(N, V1, generator=g, dtype=F64) * scale
    for r in range(N):
        i = int(x[r].argmax())
        rest = torch.logsumexp(torch.cat([x[r, :i], x[r, i + 1:]]), 0) if V1 > 1 else torch.tensor(0.0, dtype=F64)
        share = 0.2 + 0.45 * float(torch.rand((), generator=g))
        x[r, i] = rest + math.log(share / (1 - share))
    return x


def plant(x, kind, param, T, g):
    """float32 rows whose every decision under (kind, param, T) has its margin; x float64 [N, V1] is the starting point.
    Row by row: tokens inside 2 GAP of the boundary are pushed 4 GAP further out, and where the row has room one token is put 3 GAP
    inside and one 3 GAP outside of the boundary; all of it on the float32 values, until nothing moves."""
    x = x.float().to(F64)
    N, V1 = x.shape
    for r in range(N):
        perm = torch.randperm(V1, generator=g)
        for turn in range(200):
            push = (4 * GAP if turn < 20 else 0.1) * T            # a short row may need more than a nudge: every move shifts H
            row = x[r:r + 1]
            lp, p, H = stats(row, T)
            lp, p = lp[0], p[0]
            top = int(p.argmax())
            pick = perm[(perm != top) & (p[perm] > 0)][:2].tolist()
            moved = False
            if kind == 'typ':
                s = (-lp - H[0]).abs()
                cut, below, upto = typical_cut(s, p, param)
                if abs(below - param) < 2 * GAP * param or abs(upto - param) < 2 * GAP * param:
                    x[r, top] += 0.05 * T                                   # shifts every cumulative mass
                    moved = True
                else:
                    # the designated pair: less probable than typical (-log p = H + s), on both sides of s*, if that is a light token
                    placed = []
                    for v, off in zip(pick, (-3 * GAP, 3 * GAP)):
                        want = -(float(H[0]) + cut + off)
                        if V1 >= 8 and want < math.log(0.02) and cut + off > 0 and s[v] != cut:
                            placed.append(v)
                            if abs(float(lp[v]) - want) > GAP / 4:
                                x[r, v] += T * (want - float(lp[v]))
                                moved = True
                    if not moved:
                        near = (p > 0) & (s != cut) & ((s - cut).abs() < 2 * GAP)
                        for v in torch.nonzero(near).flatten().tolist():
                            if v in placed:
                                continue
                            # away from s*: the score grows when a token less probable than typical loses mass, and the other way round
                            grow = s[v] > cut
                            less = -lp[v] > H[0]
                            x[r, v] += (-1 if grow == less else 1) * push
                            moved = True
            else:
                lt = float(log_threshold(kind, param, lp[None], H)[0])
                placed = []
                for v, off in zip(pick, (3 * GAP, -3 * GAP)):
                    if lt + off < float(lp[top]) - 10 * GAP:
                        placed.append(v)
                        if abs(float(lp[v]) - (lt + off)) > GAP / 4:
                            x[r, v] += T * (lt + off - float(lp[v]))
                            moved = True
                if not moved:
                    near = (p > 0) & ((lp - lt).abs() < 2 * GAP)
                    near[top] = False
                    for v in torch.nonzero(near).flatten().tolist():
                        if v not in placed:
                            x[r, v] += (1 if lp[v] >= lt else -1) * push
                            moved = True
            x[r] = x[r].float().to(F64)
            if not moved:
                break
        else:
            raise AssertionError('margins not reached: %s %s T %s row %d' % (kind, param, T, r))
    out = x.float()
    check_margins(out, kind, param, T)
    return out


def rows_for(N, V1, kind, param, T, seed, scale=2.5):
    """the float32 case rows [N, V1] of a shape and rule: log-probabilities with a constraint's -inf entries on the odd rows"""
    g = gen(seed)
    x = torch.log_softmax(_raw_rows(N, V1, g, scale), 1)
    for r in range(1, N, 2):
        if V1 >= 5:
            low = torch.argsort(x[r])[:2]
            x[r, low] = NEG_INF
    return plant(x, kind, param, T, g)


def special_rows(V1):
    """float32 [4, V1]: uniform, one-hot with -inf elsewhere, one-hot above a far tail, a row with -inf entries"""
    x = torch.zeros(4, V1)
    x[0] = -math.log(V1)
    x[1] = NEG_INF
    x[1, V1 // 2] = 0.0
    x[2] = -60.0
    x[2, V1 // 3] = 0.0
    x[3] = torch.log_softmax(torch.randn(V1, generator=gen(V1)) * 2.0, 0)
    x[3, ::3] = NEG_INF
    if V1 > 1:
        x[3, 1] = 0.5
    return x


# ------------------------------------------------------------------------------------------------ the host loops, restated
def _pick(q, gumbel):
    """argmax(q + g), the lowest index on a tie"""
    return torch.max(q + gumbel.to(F64), 1)[1]


def sample_loop(step, N, B, V1, L, kind, param, T, gumbel, bad_endings=(), decoding_constraint=0, remove_bad_endings=0,
                block_trigrams=0):
    """decode.sample_steps with a truncation rule: step(t, it [N] int64) -> logits [N, V1] (any float type).  gumbel [L, N, V1].
    Returns seq [N, L], the constrained log-probabilities lp [N, L, V1] of every step (before the unfinished flag is applied),
    was_unfinished [N, L] and the smallest winner gap of the live rows."""
    from oracle.decode_opts import _constrain, _trigram_penalty
    seq = torch.zeros(N, L, dtype=torch.long)
    lps = torch.zeros(N, L, V1, dtype=F64)
    was = torch.zeros(N, L, dtype=torch.bool)
    it = torch.zeros(N, dtype=torch.long)
    unf = torch.ones(N, dtype=torch.bool)
    gap = float('inf')
    for t in range(L):
        lp = torch.log_softmax(step(t, it).to(F64), 1)
        lp = _constrain(lp, seq, t, bad_endings, bool(decoding_constraint), bool(remove_bad_endings))
        if block_trigrams:
            lp = _trigram_penalty(lp, seq, t, B)
        q = truncate_ref(lp, kind, param, T)['q']
        score = q + gumbel[t].to(F64)
        tok = torch.max(score, 1)[1]
        top2 = torch.sort(score, 1, descending=True)[0][:, :2]
        live = unf if t > 0 else torch.ones_like(unf)
        if V1 > 1 and bool(live.any()):
            gap = min(gap, float((top2[:, 0] - top2[:, 1])[live].min()))
        tok = torch.where(live, tok, torch.zeros_like(tok))
        was[:, t] = live
        lps[:, t] = lp
        seq[:, t] = tok
        unf = live & (tok != 0)
        it = tok
    return seq, lps, was, gap


def diverse_loop(step, B, G, V1, L, kind, param, temperature, lam, gumbel):
    """decode.diverse_sample_steps with a truncation rule: step(t, it [B * G] image-major) -> logits [B * G, V1].
    gumbel [L, G, B, V1].  Returns (seq [B * G, L], sel_logp [B * G, L] = q[token], unmasked; smallest winner gap)."""
    seq = torch.zeros(G, B, L, dtype=torch.long)
    slp = torch.zeros(G, B, L, dtype=F64)
    it = torch.zeros(G, B, dtype=torch.long)
    unf = torch.ones(G, B, dtype=torch.bool)
    gap = float('inf')
    for t in range(L):
        logits = step(t, it.t().reshape(B * G)).to(F64)
        lp_all = torch.log_softmax(logits / temperature, 1).view(B, G, V1).transpose(0, 1).clone()
        for g in range(G):
            lp = lp_all[g]
            for pg in range(g):
                cols = torch.unique(seq[pg][:, t])
                lp[:, cols] = lp[:, cols] - lam
            q = truncate_ref(lp, kind, param, 1.0)['q']
            score = q + gumbel[t, g].to(F64)
            tok = torch.max(score, 1)[1]
            top2 = torch.sort(score, 1, descending=True)[0][:, :2]
            gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
            slp[g][:, t] = q[torch.arange(B), tok]
            live = unf[g] if t > 0 else torch.ones_like(unf[g])
            tok = torch.where(live, tok, torch.zeros_like(tok))
            seq[g][:, t] = tok
            unf[g] = live & (tok != 0)
            it[g] = tok
    return seq.transpose(0, 1).reshape(B * G, L), slp.transpose(0, 1).reshape(B * G, L), gap
