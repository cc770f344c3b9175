"""Float64 restatement of the consensus (minimum-Bayes-risk) reranking of csrc/mbr.hip / imagecaptioning/pytorch_amd/mbr.py, built on
oracle/ciderd.py (CIDEr-D) and tests/rewards_ref64.py (sentence BLEU-4).  The yardstick of tests/test_mbr_host.py and
tests/test_mbr_gpu.py.  Not a test.

    utility(group, kind, df, ref_len)   U [n, n]: candidate i as the hypothesis against candidate j as its ONLY reference
    seq_weight(logp_sel, seq)           the model prior: the sum of a candidate's selected log-probs over its kept steps
    select(U, group, weight)            (expected [n], choice)
    rerank(rows, n, kind, ...)          (U [B,n,n], expected [B,n], choice [B]) of rows [B * n, L]

Token convention: the training rewards' (array_to_str) -- a row is cut AFTER its first 0, which is a word; a row without 0 is taken
whole, on either side of a pair.

The selection rule.  expected[i] = sum_{j != i} w_j U[i][j] / sum_{j != i} w_j (j ascending; 0 where the denominator is 0), w_j = 1
or exp(weight_j - max weight), the largest exactly 1.  A candidate whose caption repeats an earlier candidate's is never chosen (it
still counts as a reference); the choice is the lowest index with the largest expected value among the first occurrences, so 0
when all expected values are 0.
"""
import math

import numpy as np

from oracle import ciderd as OC

import rewards_ref64 as W

KINDS = ('ciderd', 'bleu4')


def utility(group, kind, df=None, ref_len=None):
    """U [n, n] of the n rows of one image; every candidate is cooked once (CiderD._vec of its n-gram counts)"""
    toks = [OC.tokens_of(r) for r in group]
    n = len(toks)
    U = np.zeros((n, n))
    if kind == 'ciderd':
        sc = OC.CiderD(df, ref_len)
        cooked = [sc._vec(OC.precook(t)) for t in toks]
        for i, (vh, nh, lh) in enumerate(cooked):
            for j, (vr, nr, lr) in enumerate(cooked):
                U[i, j] = float(np.mean(sc._sim(vh, vr, nh, nr, lh, lr)) / 1 * 10.0)        # score_one with one reference
    elif kind == 'bleu4':
        for i in range(n):
            for j in range(n):
                U[i, j] = W.bleu4(group[i], [group[j]])
    else:
        raise ValueError(kind)
    return U


def seq_weight(logp_sel, seq):
    """[N] from the selected log-probs [N, L] and the tokens [N, L]: the steps of losses._shifted_mask (position 0, then every
    step behind a non-zero token: the end token's step counts)"""
    seq = np.asarray(seq)
    mask = np.concatenate([np.ones((seq.shape[0], 1)), (seq[:, :-1] > 0).astype(np.float64)], 1)
    return (np.asarray(logp_sel, dtype=np.float64) * mask).sum(1)


def weights(weight, n):
    if weight is None:
        return np.ones(n)
    weight = np.asarray(weight, dtype=np.float64)
    mx = weight.max()
    return np.array([1.0 if x == mx else math.exp(x - mx) for x in weight])


def first_occurrence(group):
    toks = [tuple(OC.tokens_of(r)) for r in group]
    return [toks[i] not in toks[:i] for i in range(len(toks))]


def select(U, group, weight=None):
    U = np.asarray(U, dtype=np.float64)
    n = U.shape[0]
    w = weights(weight, n)
    expected = np.zeros(n)
    for i in range(n):
        num = den = 0.0
        for j in range(n):
            if j != i:
                num += w[j] * U[i, j]
                den += w[j]
        expected[i] = num / den if den > 0 else 0.0
    first = first_occurrence(group)
    best = 0
    for i in range(1, n):
        if first[i] and expected[i] > expected[best]:
            best = i
    return expected, best


def margin(expected, group):
    """the gap between the two largest expected values among the first occurrences (inf with fewer than two of them)"""
    first = first_occurrence(group)
    e = sorted((expected[i] for i in range(len(first)) if first[i]), reverse=True)
    return e[0] - e[1] if len(e) > 1 else math.inf


def rerank(rows, n, kind, df=None, ref_len=None, weight=None):
    rows = np.asarray(rows)
    B = rows.shape[0] // n
    U = np.stack([utility(rows[g * n:(g + 1) * n], kind, df, ref_len) for g in range(B)])
    out = [select(U[g], rows[g * n:(g + 1) * n], None if weight is None else np.asarray(weight)[g * n:(g + 1) * n])
           for g in range(B)]
    return U, np.stack([e for e, _ in out]), np.array([c for _, c in out], dtype=np.int32)
