"""Float64 restatement of discriminative decoding (imagecaptioning/pytorch_amd/disc.py, csrc/disc.hip), written from the formulas of
its contract; it imports nothing of the package.

combine: per hypothesis the decoder's logits under the target image (slot 0) and under up to 7 distractor images (slots 1 ..) ->
the row the search sees.  With lt / l_i the log-softmax of slot 0 / slot i, P the present distractor slots, D' = |P|:

    suppress   u = lt - (1 - lam) (logsumexp_{i in P} l_i - log D')
    listener   u = lt + (1 - lam) (lt - logsumexp_{i in P + {0}} l_i)
    D' = 0 or lam = 1: u = lt;  lt = -inf gives -inf whatever the distractors say

beam_search: the beam search of the package's beam driver over a decoder given as a function of the prefix: per image and step the
bd best (row, token) by sums[row] + logp[row, token], ties to the lower flat index; a kept candidate with token 0 -- every one at the
last step -- has ended, is recorded with its score and goes on 1000 lower.  The caption is the recorded candidate with the highest
score (the earlier step, then the lower slot, on a tie); its log-probability rows are those along its lineage.
"""
import math

import torch

MODES = ('suppress', 'listener')


def combine(logits, present, lam, mode):
    """logits [B, D1, cur, V1] (any float dtype), present [B, D1] (column 0 the target) -> u float64 [B, cur, V1]"""
    assert mode in MODES
    x = torch.as_tensor(logits).double()
    B, D1, cur, V1 = x.shape
    present = torch.as_tensor(present).bool().clone()
    present[:, 0] = True
    w = 1.0 - float(lam)
    lp = torch.log_softmax(x, dim=-1)
    out = torch.empty(B, cur, V1, dtype=torch.float64)
    for b in range(B):
        lt = lp[b, 0]
        ds = [i for i in range(1, D1) if present[b, i]]
        if not ds or w == 0.0:
            out[b] = lt
            continue
        if mode == 'suppress':
            u = lt - w * (torch.logsumexp(lp[b, ds], dim=0) - math.log(len(ds)))
        else:
            u = lt + w * (lt - torch.logsumexp(lp[b, [0] + ds], dim=0))
        out[b] = torch.where(torch.isneginf(lt), lt, u)
    return out


def beam_search(decoder, B, V1, L, bd):
    """decoder(k, prefix tuple) -> float64 log-probabilities [V1] of image k's next token (a normalised row).  Returns a dict: seq
    [B, L] int64, logp [B, L, V1] float64 (zero rows behind the caption's end), score [B], length [B], and the two margins of the
    replay: step_gap [L, B] the last kept score minus the first dropped one, final_gap [B] the caption's score minus the best other
    recorded candidate's (inf where there is none)."""
    out = dict(seq=torch.zeros(B, L, dtype=torch.long), logp=torch.zeros(B, L, V1, dtype=torch.float64),
               score=torch.zeros(B, dtype=torch.float64), length=torch.zeros(B, dtype=torch.long),
               step_gap=torch.full((L, B), float('inf'), dtype=torch.float64), final_gap=torch.full((B,), float('inf'), dtype=torch.float64))
    for k in range(B):
        hyps = [((), 0.0, [])]                                   # (prefix, sum, the rows along the lineage)
        done = []                                                # (score, t, slot, prefix, rows)
        for t in range(L):
            rows = [decoder(k, h[0]).double() for h in hyps]
            cand = torch.stack([h[1] + r for h, r in zip(hyps, rows)]).reshape(-1)
            order = sorted(range(cand.numel()), key=lambda f: (-float(cand[f]), f))
            keep = order[:bd]
            if len(order) > bd:
                out['step_gap'][t, k] = float(cand[keep[-1]]) - float(cand[order[bd]])
            nxt = []
            for j, f in enumerate(keep):
                r, v = divmod(f, V1)
                prefix, lineage, s = hyps[r][0] + (v,), hyps[r][2] + [rows[r]], float(cand[f])
                ended = v == 0 or t == L - 1
                if ended:
                    done.append((s, t, j, prefix, lineage))
                nxt.append((prefix, s - 1000.0 if ended else s, lineage))
            hyps = nxt
        done.sort(key=lambda d: (-d[0], d[1], d[2]))
        s, t, _, prefix, lineage = done[0]
        if len(done) > 1:
            out['final_gap'][k] = s - done[1][0]
        out['seq'][k, :t + 1] = torch.tensor(prefix)
        out['logp'][k, :t + 1] = torch.stack(lineage)
        out['score'][k], out['length'][k] = s, t + 1
    return out
