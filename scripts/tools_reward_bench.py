"""Times the reward launches of one SCST / new_self_critical step at the headline size: H = 60 rows (10 images x 5 sampled + 10
greedy), L = 20, 5 references of width <= 20 per image, the synthetic corpus of oracle.ciderd.synthetic_corpus.

    python scripts/tools_reward_bench.py [--iters 50]

Device events around each call, one warm-up, the median of --iters (>= 20).  Prints one JSON line: microseconds of the CIDEr-D
launch (the yardstick), the BLEU-4 + mix launch, and the two self-CIDEr launches."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_us(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    args = ap.parse_args()
    iters = max(20, args.iters)
    from oracle import ciderd as OC
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD
    dev = torch.device('cuda:0')
    B, n, L, vocab = 10, 5, 20, 9487
    corpus = OC.synthetic_corpus(2000, vocab, 5, L, seed=1234)
    df, ref_len = OC.build_document_frequency([[OC.tokens_of(r) for r in g] for g in corpus])
    sc = DeviceCiderD(df, ref_len, dev)
    gts = corpus[:B]
    packed = sc.pack_refs(gts)
    refs, n_refs = packed
    rng = np.random.default_rng(0)
    rows = np.zeros((B * n + B, L), dtype=np.int64)
    for r in range(B * n + B):                                 # a reference of the image with 30 % of its words replaced
        g = gts[r // n if r < B * n else r - B * n]
        row = g[int(rng.integers(0, len(g)))].astype(np.int64).copy()
        words = int((row > 0).sum())
        flip = rng.random(words) < 0.3
        row[:words][flip] = rng.integers(1, vocab + 1, size=int(flip.sum()))
        rows[r] = row
    hyp = torch.from_numpy(rows).to(dev)
    img = torch.cat([torch.arange(B * n, device=dev) // n, torch.arange(B, device=dev)]).to(torch.int32)
    scores = sc.score(hyp, img, refs, n_refs, packed.cooked)
    sampled = hyp[:B * n].contiguous()
    out = {'H': B * n + B, 'L': L, 'n': n, 'iters': iters,
           'ciderd_us': median_us(lambda: sc.score(hyp, img, refs, n_refs, packed.cooked), iters),
           'bleu4_mix_us': median_us(lambda: sc.bleu4(hyp, img, packed, 1.0, 0.5, base=scores), iters),
           'self_cider_us': median_us(lambda: sc.self_cider(sampled, n), iters)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
