"""float64 restatement of contrastive search (Su et al. 2022) as decode.contrastive_steps runs it -- a test helper in plain torch.

    search(step, state, N, V1, L, k, alpha, ...)       the decode loop over a single-step callable
    select(tok, lp, g, hist, alpha, unf)               one scoring step (what capmi_contrastive_select computes), numpy

step(it [rows] int64, state) -> (logits [rows, V1], hidden [rows, R], state'): `hidden` is the row the vocabulary projection reads,
`state` a tuple of tensors with the rows in front, so that tuple(s[idx] for s in state) reorders it.

Definition.  h_s[i]: the hidden row of caption i after input token s (s = 0: BOS).  At output position t the k largest entries of the
constrained log-softmax row are the candidates v_0..v_{k-1} (ties: the lower id), p_j = exp(logp[v_j]); the decoder is stepped on the
N * k candidate rows, which gives g_j; score_j = (1 - alpha) p_j - alpha max_{s <= t} cos(g_j, h_s) with
cos(a, b) = a.b / max(|a| |b|, 1e-8); a candidate at -inf scores -inf; the winner is the lowest j of the largest score.  The winner's
hidden row joins the history, its state and logits are the next step's.
"""
import numpy as np
import torch

F64 = torch.float64


def topk_ids(lp, k):
    """the k largest entries of every row, descending, equal values by ascending id (-inf entries included): ids [N, k]"""
    return torch.sort(lp, dim=1, descending=True, stable=True)[1][:, :k]


def cosines(g, hist):
    """g [N, k, R], hist [N, S, R] -> cos [N, k, S] with cosine_similarity's clamp"""
    dots = torch.einsum('nkr,nsr->nks', g, hist)
    den = (g.norm(dim=2).unsqueeze(2) * hist.norm(dim=2).unsqueeze(1)).clamp_min(1e-8)
    return dots / den


def scores(lp_k, g, hist, alpha):
    """lp_k [N, k] candidate log-probs, g [N, k, R], hist [N, S, R] (S >= 1) -> score [N, k]"""
    pen = cosines(g, hist).max(2)[0]
    s = (1.0 - alpha) * lp_k.exp() - alpha * pen
    return torch.where(torch.isneginf(lp_k), torch.full_like(s, float('-inf')), s)


def choose(score):
    """(arg-max with the lowest index on ties [N], best minus second best [N] (inf for k = 1; nan where both are -inf))"""
    c = torch.max(score, 1)[1]
    if score.shape[1] == 1:
        return c, torch.full((score.shape[0],), float('inf'), dtype=F64)
    top2 = torch.sort(score, 1, descending=True)[0][:, :2]
    return c, top2[:, 0] - top2[:, 1]


def search(step, state, N, V1, L, k, alpha, bad_endings=(), decoding_constraint=0, remove_bad_endings=0, block_trigrams=0):
    """Returns a dict: seq [N, L], lps [N, L, V1] (the constrained log-probabilities of every step, before the unfinished flag),
    was_unfinished [N, L], choice [N, L], score_gap (the smallest best-minus-second-best score over the live rows and steps) and
    topk_gap (the smallest logp[v_{k-1}] - logp[v_k] over the live rows and steps: how far the candidate set is from changing)."""
    from oracle.decode_opts import _constrain, _trigram_penalty
    seq = torch.zeros(N, L, dtype=torch.long)
    lps = torch.zeros(N, L, V1, dtype=F64)
    was = torch.zeros(N, L, dtype=torch.bool)
    choice = torch.zeros(N, L, dtype=torch.long)
    unf = torch.ones(N, dtype=torch.bool)
    score_gap = topk_gap = float('inf')
    logits, h, state = step(torch.zeros(N, dtype=torch.long), state)
    hist = h.to(F64).unsqueeze(1)                                                  # [N, 1, R]
    logits = logits.to(F64)
    rows = torch.arange(N)
    for t in range(L):
        lp = torch.log_softmax(logits, 1)
        lp = _constrain(lp, seq, t, bad_endings, bool(decoding_constraint), bool(remove_bad_endings))
        if block_trigrams:
            lp = _trigram_penalty(lp, seq, t, N)
        srt, ids = torch.sort(lp, dim=1, descending=True, stable=True)
        tok, lp_k = ids[:, :k], srt[:, :k]
        fan = rows.repeat_interleave(k)
        logits_k, g, state_k = step(tok.reshape(-1), tuple(s[fan] for s in state))
        g = g.to(F64).view(N, k, -1)
        sc = scores(lp_k, g, hist, alpha)
        c, gap = choose(sc)
        if bool(unf.any()):
            if k > 1:
                score_gap = min(score_gap, float(gap[unf].min()))
            if k < V1:
                edge = (srt[:, k - 1] - srt[:, k])[unf]
                edge = edge[~torch.isnan(edge)]                                    # -inf minus -inf: both outside any finite margin
                if edge.numel():
                    topk_gap = min(topk_gap, float(edge.min()))
        pick = rows * k + c
        new = tok[rows, c]
        new = torch.where(unf, new, torch.zeros_like(new))
        was[:, t], lps[:, t], seq[:, t], choice[:, t] = unf, lp, new, c
        unf = unf & (new != 0)
        hist = torch.cat([hist, g[rows, c].unsqueeze(1)], 1)
        state = tuple(s[pick] for s in state_k)
        logits = logits_k.to(F64)[pick]
    return dict(seq=seq, lps=lps, was_unfinished=was, choice=choice, score_gap=score_gap, topk_gap=topk_gap)


def select(tok, lp, g, hist, alpha, unf):
    """One launch of capmi_contrastive_select in float64 numpy.  tok, lp [N, k]; g [N, k, R]; hist [N, S, R] (S may be 0); unf [N]
    bool.  Returns choice, parent, token (0 where finished), the new flags, the appended row and its inverse norm, and the smallest
    score gap of every row (inf for k = 1 or when the runner-up is -inf)."""
    N, k, R = g.shape
    g, hist, lp = g.astype(np.float64), hist.astype(np.float64), lp.astype(np.float64)
    gn = np.sqrt((g * g).sum(2))
    if hist.shape[1]:
        hn = np.sqrt((hist * hist).sum(2))
        dots = np.einsum('nkr,nsr->nks', g, hist)
        pen = (dots / np.maximum(gn[:, :, None] * hn[:, None, :], 1e-8)).max(2)
    else:
        pen = np.zeros((N, k))
    with np.errstate(divide='ignore', invalid='ignore'):
        score = np.where(np.isneginf(lp), -np.inf, (1.0 - alpha) * np.exp(lp) - alpha * pen)
        choice = np.argmax(score, 1)                                               # the first of equal maxima
        rows = np.arange(N)
        srt = -np.sort(-score, 1)
        gap = np.full(N, np.inf) if k == 1 else np.where(np.isneginf(srt[:, 1]), np.inf, srt[:, 0] - srt[:, 1])
        token = np.where(unf, tok[rows, choice], 0)
        return dict(choice=choice, parent=rows * k + choice, token=token, unfinished=unf & (token != 0), row=g[rows, choice],
                    inv=1.0 / gn[rows, choice], gap=gap, score=score)


# ------------------------------------------------------------------------------------------------ the families' float64 single steps
def family_step(name, P, fc, att, att_masks, opt=None):
    """(step, state0, N) for search(): the float64 single step of a family -- tests/att2in2_ref64.py, tests/adaatt_ref64.py,
    tests/aoa_variants_ref64.py (opt: the model's options, out_res 0), and for updown / newfc the oracle's step (oracle/att_lstm.py)
    on float64 tensors.  P: the state_dict (any float type)."""
    P = {k: v.to(F64) for k, v in P.items()}
    B = att.shape[0] if fc is None else fc.shape[0]
    if name == 'aoa':
        import aoa_variants_ref64 as A
        assert not getattr(opt, 'out_res', 0)                     # with out_res the logit reads output + h_att, not the carried row
        heads = opt.num_heads
        mean, p_att, am = A.prepare(P, opt, heads, None if fc is None else fc.to(F64), att.to(F64),
                                    None if att_masks is None else att_masks.to(F64))
        R = mean.shape[1]

        def step(it, state):
            n = it.shape[0] // B
            rep = lambda x: None if x is None else x.repeat_interleave(n, 0)      # noqa: E731
            h_att, out, c_att, c_logic = state
            logp, (hs, cs) = A.step(P, opt, heads, it, rep(mean), rep(p_att), rep(am),
                                    (torch.stack([h_att, out]), torch.stack([c_att, c_logic])))
            return logp, hs[1], (hs[0], hs[1], cs[0], cs[1])      # a normalised row: search()'s log_softmax leaves it as it is
        return step, tuple(torch.zeros(B, R, dtype=F64) for _ in range(4)), B
    if name == 'att2in2':
        import att2in2_ref64 as A
        a, p_att, am = A.prefill(P, att, att_masks)
        R = P['core.h2h.weight'].shape[1]

        def step(it, state):
            logits, h, c = A.step(P, it, state[0], state[1], a, p_att, am, it.shape[0] // B)
            return logits, h, (h, c)
        return step, (torch.zeros(B, R, dtype=F64), torch.zeros(B, R, dtype=F64)), B
    if name in ('adaatt', 'adaattmo'):
        import adaatt_ref64 as A
        f, a, p_att, am = A.prefill(P, fc, att, att_masks)
        R = P['logit.weight'].shape[1]
        W, b = P['logit.weight'], P['logit.bias']
        assert int(torch.linalg.matrix_rank(W)) == R              # logit is injective: its operand is the solution of W x = logits - b

        def step(it, state):
            logits, h, c = A.step(P, it, state[0], state[1], f, a, p_att, am, it.shape[0] // B)
            out = torch.linalg.lstsq(W, (logits - b).t()).solution.t()
            assert float((out @ W.t() + b - logits).abs().max()) < 1e-12
            return logits, out, (h, c)
        return step, (torch.zeros(B, R, dtype=F64), torch.zeros(B, R, dtype=F64)), B
    from oracle import att_lstm as O
    if name == 'updown':
        f, a, p_att, am = O.prepare_feature(P, fc.to(F64), att.to(F64), att_masks)
        R = P['logit.weight'].shape[1]

        def step(it, state):
            n = it.shape[0] // B
            fr, ar, pr, mr = O.repeat_rows(n, f, a, p_att, am)
            h_att, h_lang, c_att, c_lang = state
            logits, (h, c) = O.updown_step(P, it, fr, ar, pr, mr, (torch.stack([h_att, h_lang]), torch.stack([c_att, c_lang])),
                                           want_logsoftmax=False)
            return logits, h[1], (h[0], h[1], c[0], c[1])
        return step, tuple(torch.zeros(B, R, dtype=F64) for _ in range(4)), B
    if name == 'newfc':
        f = fc.to(F64) @ P['fc_embed.weight'].t() + P['fc_embed.bias']
        R = P['logit.weight'].shape[1]

        def step(it, state):
            fr, = O.repeat_rows(it.shape[0] // B, f)
            logits, (h, c) = O.newfc_step(P, it, fr, (state[0].unsqueeze(0), state[1].unsqueeze(0)), want_logsoftmax=False)
            return logits, h[0], (h[0], c[0])
        return step, (torch.zeros(B, R, dtype=F64), torch.zeros(B, R, dtype=F64)), B
    raise KeyError(name)
