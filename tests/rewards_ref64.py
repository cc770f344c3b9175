"""Float64 restatement of the training rewards beside CIDEr-D -- Bleu(4)'s per-sentence BLEU-4 (reference rewards.py:68-74,
105-112) and Cider.my_self_cider + get_div (rewards.py:116-136) -- and of the call-site arithmetic that mixes them
(rewards.py:74-77, losses.py:175-187).  The yardstick of tests/test_reward_mix_host.py and tests/test_reward_mix_gpu.py.  Not a test.

PARITY UNPINNED for the two scorers: coco-caption and the cider submodule are empty directories in the reference checkout, so
they are written from the published formulas, on the helpers of langeval_ref64.py / diveval_ref64.py.  The call-site arithmetic
IS pinned: tests/golden/reward_mix.npz was recorded from the reference's own rewards.py and losses.py.

Token convention: array_to_str (rewards.py:33-39) -- a row is cut AFTER its first 0, so the 0 is a word; a row without 0 is taken
whole.  The evaluation helpers cut BEFORE the first 0; they are given the words shifted up by one, which holds no 0.

One deviation from the reference: self-CIDEr is 0.0 where sum sqrt(lambda) = 0 (numpy gives NaN), as in diveval_ref64.
"""
import math

import numpy as np

import diveval_ref64 as D
import langeval_ref64 as R


def tokens_of(row):
    """array_to_str: ids up to and INCLUDING the first 0"""
    out = []
    for t in row:
        out.append(int(t))
        if int(t) == 0:
            break
    return out


def _shift(row):
    return [t + 1 for t in tokens_of(row)]


def bleu_stats(hyp, refs):
    """guess [4], correct [4], testlen, reflen ('closest', ties to the shorter) of one hypothesis against its references"""
    return R.bleu_stats_image(_shift(hyp), [_shift(r) for r in refs])


def bleu4(hyp, refs):
    """Bleu(4).compute_score(gts, res)[1][3] for one hypothesis"""
    return R.bleu_corpus(*bleu_stats(hyp, refs))[3]


def _shift_df(df):
    return {tuple(int(t) + 1 for t in g): float(v) for g, v in df.items()}


def self_cider_parts(group, df, ref_len, shifted_df=None):
    """(K [n,n], ascending eigenvalues of K/10, score) of the n rows of one image; weight of an n-gram = tf * (log(ref_len) -
    log(max(1, df)))"""
    sdf = shifted_df if shifted_df is not None else _shift_df(df)
    K = D.self_cider_matrix([_shift(r) for r in group], sdf, math.log(float(ref_len)))
    eig = np.linalg.eigvalsh(K / 10)
    return K, eig, D.self_cider_of(eig)


def self_cider_scores(rows, n, df, ref_len):
    """get_self_cider_scores: [B] from rows [B * n, L]"""
    sdf = _shift_df(df)
    return np.array([self_cider_parts(rows[i:i + n], df, ref_len, sdf)[2] for i in range(0, len(rows), n)])


# ---- call site ---------------------------------------------------------------------------------------------------------------
def mix(cw, bw, cider, bleu):
    """rewards.py:74 / :112; a scorer whose weight is 0 is not called and counts as the scalar 0"""
    return cw * (cider if cw > 0 else 0) + bw * (bleu if bw > 0 else 0)


def self_critical_reward(cw, bw, cider, bleu, B, L):
    """rewards.py:74-79 from the scores of the N sampled then B greedy rows: [N, L]"""
    s = mix(cw, bw, cider, bleu)
    N = len(s) - B
    adv = s[:N].reshape(B, N // B) - s[N:][:, None]
    return np.repeat(adv.reshape(N)[:, None], L, 1)


def nsc_weights(scores, n, self_cider=None, sw=0.0):
    """losses.py:175-182: leave-one-out advantage [B, n], plus sw * self_cider[image] on each of its rows"""
    s = np.asarray(scores, dtype=np.float64).reshape(-1, n)
    w = s - (s.sum(1, keepdims=True) - s) / (n - 1)
    if sw > 0:
        w = w + sw * np.asarray(self_cider, dtype=np.float64).reshape(-1, 1)
    return w


def nsc_loss(logp_sel, seq, weights, reduction='mean'):
    """losses.py:183-187 on the selected log-probs [N, L]: mask = position 0 on, then (seq > 0) shifted right"""
    seq = np.asarray(seq)
    mask = np.concatenate([np.ones((seq.shape[0], 1)), (seq[:, :-1] > 0).astype(np.float64)], 1)
    out = -np.asarray(logp_sel, dtype=np.float64) * mask * np.asarray(weights, dtype=np.float64).reshape(-1, 1)
    return out.sum(1) / mask.sum(1) if reduction == 'none' else out.sum() / mask.sum()
