"""Float64 restatement of coco-caption's Cider, Bleu (option 'closest') and Rouge over token ids -- the yardstick of
tests/test_langeval_host.py and tests/test_langeval_gpu.py.  Not a test.

PARITY UNPINNED: coco-caption is not part of the reference checkout (its submodule directory is empty), so this file is
written from the published formulas of pycocoevalcap (cider/cider_scorer.py, bleu/bleu_scorer.py, rouge/rouge.py), not checked
against their code.  The PTB tokenizer is not reproduced: a caption is the ids of its row before the first 0 (the whole row
when it holds none), compared as integers.

    refs: list (per image) of lists of rows;  hyps: list (per image) of one row, or None for an image without a hypothesis
"""
import math
from collections import Counter

import numpy as np

NG = 4
BETA = 1.2
TINY, SMALL = 1e-15, 1e-9          # bleu_scorer.py


def caption(row):
    out = []
    for t in row:
        if int(t) == 0:
            break
        out.append(int(t))
    return out


def ngrams(words, n=NG):
    """cook: Counter {n-gram tuple -> count} over the orders 1..n"""
    c = Counter()
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            c[tuple(words[i:i + k])] += 1
    return c


def document_frequency(refs):
    """cider_scorer.compute_doc_freq: every n-gram counts once per image"""
    df = Counter()
    for image in refs:
        for g in set(g for row in image for g in ngrams(caption(row))):
            df[g] += 1
    return df


def _vec(counts, df, log_n):
    vec = [dict() for _ in range(NG)]
    norm = [0.0] * NG
    for g, tf in counts.items():
        k = len(g) - 1
        vec[k][g] = float(tf) * (log_n - math.log(max(1.0, float(df.get(g, 0)))))
        norm[k] += vec[k][g] ** 2
    return vec, [math.sqrt(x) for x in norm]


def cider_image(hyp, image_refs, df, log_n):
    """cider_scorer.compute_cider for one image: 10 * mean_n mean_ref cosine (no clipping, no length penalty)"""
    vh, nh = _vec(ngrams(caption(hyp)), df, log_n)
    score = np.zeros(NG)
    for row in image_refs:
        vr, nr = _vec(ngrams(caption(row)), df, log_n)
        for k in range(NG):
            val = 0.0
            for g, x in vh[k].items():
                val += x * vr[k].get(g, 0.0)
            if nh[k] != 0 and nr[k] != 0:
                val /= nh[k] * nr[k]
            score[k] += val
    if not image_refs:
        return 0.0
    return float(np.mean(score)) / len(image_refs) * 10.0


def bleu_stats_image(hyp, image_refs):
    """bleu_scorer.cook_refs / cook_test: guess [4], correct [4], testlen, reflen ('closest', ties to the shorter)"""
    h = caption(hyp)
    counts = ngrams(h)
    maxcounts = Counter()
    lens = []
    for row in image_refs:
        r = caption(row)
        lens.append(len(r))
        for g, c in ngrams(r).items():
            maxcounts[g] = max(maxcounts[g], c)
    guess = [max(0, len(h) - k) for k in range(NG)]
    correct = [0] * NG
    for g, c in counts.items():
        correct[len(g) - 1] += min(maxcounts.get(g, 0), c)
    reflen = min((abs(l - len(h)), l) for l in lens)[1] if lens else 0
    return guess, correct, len(h), reflen


def bleu_corpus(guess, correct, testlen, reflen):
    """bleu_scorer.compute_score on the summed statistics"""
    bleus, b = [], 1.0
    for k in range(NG):
        b *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        bleus.append(b ** (1.0 / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        bleus = [x * math.exp(1 - 1 / ratio) for x in bleus]
    return bleus


def lcs(a, b):
    t = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            t[i][j] = t[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(t[i - 1][j], t[i][j - 1])
    return t[len(a)][len(b)]


def rouge_image(hyp, image_refs):
    """rouge.calc_score: (F, [lcs per reference]).  An empty caption on either side gives precision / recall 0."""
    h = caption(hyp)
    prec, rec, ls = [0.0], [0.0], []
    for row in image_refs:
        r = caption(row)
        x = lcs(r, h)
        ls.append(x)
        if h:
            prec.append(x / float(len(h)))
        if r:
            rec.append(x / float(len(r)))
    p, q = max(prec), max(rec)
    f = (1 + BETA ** 2) * p * q / float(q + BETA ** 2 * p) if p != 0 and q != 0 else 0.0
    return f, ls


def evaluate(refs, hyps):
    """-> dict: the six corpus scores, 'cider_img' / 'rouge_img' (NaN where hyps[i] is None), 'totals' (guess 1..4, correct 1..4,
    testlen, reflen), 'stats' per image, 'lcs' per image, 'df'.  The document frequency covers ALL images of `refs`."""
    df = document_frequency(refs)
    log_n = math.log(float(len(refs)))
    cider = np.full(len(refs), np.nan)
    rouge = np.full(len(refs), np.nan)
    totals = np.zeros(10, dtype=np.int64)
    stats, lcss = {}, {}
    for i, (image, hyp) in enumerate(zip(refs, hyps)):
        if hyp is None:
            continue
        cider[i] = cider_image(hyp, image, df, log_n)
        rouge[i], lcss[i] = rouge_image(hyp, image)
        g, c, tl, rl = bleu_stats_image(hyp, image)
        stats[i] = (g, c, tl, rl)
        totals += np.array(g + c + [tl, rl], dtype=np.int64)
    bleus = bleu_corpus(totals[:4], totals[4:8], int(totals[8]), int(totals[9]))
    out = {'Bleu_%d' % (k + 1): float(bleus[k]) for k in range(NG)}
    seen = ~np.isnan(cider)
    out['ROUGE_L'] = float(rouge[seen].mean()) if seen.any() else 0.0
    out['CIDEr'] = float(cider[seen].mean()) if seen.any() else 0.0
    out.update(cider_img=cider, rouge_img=rouge, totals=totals, stats=stats, lcs=lcss, df=df)
    return out
