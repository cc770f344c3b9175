"""Float64 restatement of the reference's diversity evaluation (captioning/utils/eval_multi.py) over token ids -- the yardstick of
tests/test_diveval_host.py and tests/test_diveval_gpu.py.  Not a test.

Div1 / Div2 / gDiv1 restate captioning/utils/div_utils.py, which IS part of the reference checkout: tests/golden/diveval_ref.npz
pins them (tests/golden/make_diveval.py ran the reference's functions).  PARITY UNPINNED for the rest: coco-caption's Bleu and
the cider submodule's my_self_cider are not in the checkout, so mBLEU and self-CIDEr are written from the published formulas
(bleu_scorer.py; Wang & Chan 2019, "Describing like humans: on diversity in image captioning") on langeval_ref64's helpers.

    refs: list (per image) of lists of rows;  groups: list (per image) of n rows, or None for an image without captions

One deviation from eval_self_cider: an image whose captions are all empty has sum sqrt(lambda) = 0, numpy makes that NaN; here
it scores 0.0.
"""
import math

import numpy as np

import langeval_ref64 as R

ORACLE_KEYS = ('CIDEr', 'Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L')


def distinct(group, k):
    """div_utils.compute_div_n's set for one image: the distinct k-grams over its captions"""
    out = set()
    for row in group:
        w = R.caption(row)
        out.update(tuple(w[i:i + k]) for i in range(len(w) - k + 1))
    return out


def div_n(groups, k):
    """compute_div_n: (mean, per image); the denominator is the token count for every k"""
    per = np.array([float(len(distinct(g, k))) / (1e-6 + float(sum(len(R.caption(r)) for r in g))) for g in groups])
    return per.mean(), per


def global_div_1(groups):
    """compute_global_div_n with n = 1: the number of distinct unigrams over all captions, as a float"""
    out = set()
    for g in groups:
        out |= distinct(g, 1)
    return float(len(out))


def self_cider_matrix(group, df, log_n):
    """K[i][j] = 10 * (1/4) sum_k cos_k: plain CIDEr between the captions (no clipping, no length term); an order with a zero
    norm contributes 0; i <= j computed, mirrored"""
    vecs = [R._vec(R.ngrams(R.caption(row)), df, log_n) for row in group]
    n = len(group)
    K = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            (vi, ni), (vj, nj) = vecs[i], vecs[j]
            total = 0.0
            for k in range(R.NG):
                dot = 0.0
                for g, x in vi[k].items():
                    dot += x * vj[k].get(g, 0.0)
                if ni[k] != 0 and nj[k] != 0:
                    total += dot / (ni[k] * nj[k])
            K[i, j] = K[j, i] = total / R.NG * 10.0
    return K


def self_cider_of(eig):
    """eval_self_cider.get_div on ascending eigenvalues of K/10; 0.0 where numpy would give NaN"""
    lam = np.clip(np.asarray(eig, dtype=np.float64), 0, None)
    s = np.sqrt(lam).sum()
    if s == 0:
        return 0.0
    return float(-np.log(np.sqrt(lam[-1]) / s) / np.log(len(lam)))


def evaluate(refs, groups, oracle=False):
    """-> dict: 'overall' {Div1, Div2, gDiv1, mBLeu_1..4, self_cider [, oracle_X, avg_X]}; per image (index = position in
    `refs`, rows of images without a group hold zeros, 'seen' tells): 'distinct' [n_img, 2], 'tokens' [n_img], 'mbleu_stats'
    [n_img, n, 10] (guess 1..4, correct 1..4, testlen, reflen), 'sent_bleu2' [n_img, n], 'K', 'eig', 'self_cider', 'scores'
    [n_img, n, 6]; 'totals' [n, 10]; 'gdiv_tokens' the distinct unigrams."""
    df = R.document_frequency(refs)
    log_n = math.log(float(len(refs)))
    n = len(next(g for g in groups if g is not None))
    m = len(refs)
    out = {'seen': np.array([g is not None for g in groups]), 'distinct': np.zeros((m, 2), dtype=np.int64),
           'tokens': np.zeros(m, dtype=np.int64), 'mbleu_stats': np.zeros((m, n, 10), dtype=np.int64),
           'sent_bleu2': np.zeros((m, n)), 'K': np.zeros((m, n, n)), 'eig': np.zeros((m, n)), 'self_cider': np.zeros(m),
           'scores': np.zeros((m, n, 6))}
    for i, g in enumerate(groups):
        if g is None:
            continue
        out['distinct'][i] = [len(distinct(g, 1)), len(distinct(g, 2))]
        out['tokens'][i] = sum(len(R.caption(r)) for r in g)
        for s in range(n):
            gs, c, tl, rl = R.bleu_stats_image(g[s], [g[o] for o in range(n) if o != s])
            out['mbleu_stats'][i, s] = gs + c + [tl, rl]
            out['sent_bleu2'][i, s] = R.bleu_corpus(gs, c, tl, rl)[1]
            if oracle:
                og, oc, otl, orl = R.bleu_stats_image(g[s], refs[i])
                out['scores'][i, s] = ([R.cider_image(g[s], refs[i], df, log_n)] + R.bleu_corpus(og, oc, otl, orl) +
                                       [R.rouge_image(g[s], refs[i])[0]])
        out['K'][i] = self_cider_matrix(g, df, log_n)
        out['eig'][i] = np.linalg.eigvalsh(out['K'][i] / 10)
        out['self_cider'][i] = self_cider_of(out['eig'][i])
    seen = out['seen']
    kept = [g for g in groups if g is not None]
    out['totals'] = out['mbleu_stats'][seen].sum(axis=0)
    slot_bleu = np.array([R.bleu_corpus(t[:4], t[4:8], int(t[8]), int(t[9])) for t in out['totals']])
    overall = {'Div1': float(div_n(kept, 1)[0]), 'Div2': float(div_n(kept, 2)[0]), 'gDiv1': global_div_1(kept),
               'self_cider': float(out['self_cider'][seen].mean())}
    overall.update(('mBLeu_%d' % (k + 1), float(slot_bleu[:, k].mean())) for k in range(R.NG))
    if oracle:
        for x, key in enumerate(ORACLE_KEYS):
            overall['oracle_' + key] = float(out['scores'][seen][:, :, x].max(axis=1).mean())
            overall['avg_' + key] = float(out['scores'][seen][:, :, x].mean(axis=1).mean())
    out['overall'] = overall
    return out
