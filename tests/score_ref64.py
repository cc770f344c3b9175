"""Float64 restatements of the caption-scoring arithmetic (csrc/score.hip, imagecaptioning/pytorch_amd/score.py); numpy only, no
device code.

  score_step      one step of capmi_score_step: log_softmax of logits * inv_temperature in float64, the given token gathered, the
                  live rule (a live row is scored; token 0 is scored and then the row is dead; dead rows are untouched)
  score_caption   a whole caption from per-step logits
  retrieval       ranks and log-posterior of a score matrix; ties go to the lower image index
"""
import numpy as np


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def score_step(logits, tok, live, acc, cnt, inv_temperature=1.0, unk_col=-1):
    """logits [rows, V1], tok [rows], live bool [rows], acc float64 [rows], cnt int [rows] -> (lp, live', acc', cnt'); lp is NaN
    for dead rows.  The UNK column is normalised with the others and then pushed down by 1000 (capmi_beam_logsoftmax)."""
    logits, tok, live = np.asarray(logits, np.float64), np.asarray(tok, np.int64), np.asarray(live, bool)
    lsm = log_softmax(logits * float(inv_temperature))
    if unk_col >= 0:
        lsm[:, unk_col] -= 1000.0
    lp = np.where(live, lsm[np.arange(len(tok)), tok], np.nan)
    acc2 = np.where(live, np.asarray(acc, np.float64) + np.where(live, lp, 0.0), acc)
    cnt2 = np.where(live, np.asarray(cnt) + 1, cnt)
    return lp, live & (tok != 0), acc2, cnt2


def score_caption(step_logits, seq, inv_temperature=1.0, unk_col=-1):
    """step_logits [T', V1] (row t: the distribution of word t), seq [L] padded with 0 -> (logp, len, tok_logp [L], 0 behind the
    scored part): every word up to and including the first 0, at most L of them"""
    seq = np.asarray(seq, np.int64)
    tok_logp = np.zeros(len(seq))
    total, n = 0.0, 0
    for t, v in enumerate(seq):
        lp, _, _, _ = score_step(np.asarray(step_logits[t])[None], [v], [True], [0.0], [0], inv_temperature, unk_col)
        tok_logp[t] = lp[0]
        total += lp[0]
        n += 1
        if v == 0:
            break
    return total, n, tok_logp


def retrieval(S, target):
    """S [C, I], target [C] -> (rank int [C], log_post float64 [C])"""
    S = np.asarray(S, np.float64)
    C, I = S.shape
    rank, post = np.zeros(C, np.int64), np.zeros(C)
    for c in range(C):
        t = int(target[c])
        st = S[c, t]
        rank[c] = 1 + int((S[c] > st).sum()) + int((S[c, :t] == st).sum())
        post[c] = log_softmax(S[c])[t]
    return rank, post


def summary(ranks):
    """R@1/5/10, median, mean, MRR of a list of ranks, by their definitions"""
    r = np.sort(np.asarray(ranks, np.float64))
    return {'R@1': float((r <= 1).mean()), 'R@5': float((r <= 5).mean()), 'R@10': float((r <= 10).mean()),
            'median_rank': float(np.median(r)), 'mean_rank': float(r.mean()), 'MRR': float((1.0 / r).mean())}
