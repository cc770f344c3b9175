"""Times the consensus reranking (capmi_mbr_utility + capmi_mbr_select, imagecaptioning/pytorch_amd/mbr.py) at B = 50 images,
n in {5, 10, 32} candidates, L = 20, against the only way to get the same CIDEr-D matrix without it: n calls of
capmi_ciderd_score, call j with candidate j of every image as that image's single reference (their int32 reference arrays are
built outside the timed window).

    python scripts/tools_mbr_bench.py [--iters 30] [--reps 20]

The candidates are references of the synthetic corpus of oracle.ciderd.synthetic_corpus with 30 % of their words replaced, so they
share n-grams as the samples of one image do.  Both sides are warmed up, then timed alternately in the same process: a window is
--reps back-to-back calls between two device events, ending in the second event's synchronise; the figure is the median over
--iters windows of the time per call.  The two matrices are compared at every size timed.  Prints one JSON line per n."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    iters, reps = max(10, args.iters), max(1, args.reps)
    from oracle import ciderd as OC
    from imagecaptioning.pytorch_amd import mbr
    from imagecaptioning.pytorch_amd.ciderd import DeviceCiderD
    if not torch.cuda.is_available():
        raise SystemExit('tools_mbr_bench.py measures on the GPU: none is visible')
    dev = torch.device('cuda:0')
    B, L, vocab = 50, 20, 9487
    corpus = OC.synthetic_corpus(2000, vocab, 5, L, seed=1234)
    df, ref_len = OC.build_document_frequency([[OC.tokens_of(r) for r in g] for g in corpus])
    sc = DeviceCiderD(df, ref_len, dev)
    for n in (5, 10, 32):
        rng = np.random.default_rng(n)
        rows = np.zeros((B * n, L), dtype=np.int64)
        for r in range(B * n):
            g = corpus[r // n]
            row = g[int(rng.integers(0, len(g)))].astype(np.int64).copy()
            words = int((row > 0).sum())
            flip = rng.random(words) < 0.3
            row[:words][flip] = rng.integers(1, vocab + 1, size=int(flip.sum()))
            rows[r] = row
        seq = torch.from_numpy(rows).to(dev)
        img = (torch.arange(B * n, device=dev) // n).to(torch.int32)
        n_refs = torch.ones(B, dtype=torch.int32, device=dev)
        refs = []
        for j in range(n):
            a = np.full((B, 1, L + 1), -1, dtype=np.int32)
            a[:, 0, :L] = rows[j::n]
            refs.append(torch.from_numpy(a).to(dev))

        def rerank():
            U = mbr.utility(seq, n, 'mbr_ciderd', sc)
            return U, mbr.select(U, seq, n)

        def columns():
            return [sc.score(seq, img, refs[j], n_refs) for j in range(n)]

        U, (expected, choice) = rerank()
        cols = torch.stack(columns(), 1).view(B, n, n)
        torch.cuda.synchronize()
        diff = float((U - cols).abs().max())
        for _ in range(3):                                     # warm both sides at this shape
            window_us(rerank, reps)
            window_us(columns, reps)
        t_mbr, t_cols = [], []
        for _ in range(iters):                                 # alternately: whatever else the machine does hits both alike
            t_mbr.append(window_us(rerank, reps))
            t_cols.append(window_us(columns, reps))
        q = lambda t, p: float(np.percentile(t, p))            # noqa: E731
        print(json.dumps({'B': B, 'n': n, 'L': L, 'iters': iters, 'reps': reps, 'max_abs_diff': diff,
                          'mbr_us': q(t_mbr, 50), 'mbr_us_p10_p90': [q(t_mbr, 10), q(t_mbr, 90)],
                          'ciderd_columns_us': q(t_cols, 50), 'ciderd_columns_us_p10_p90': [q(t_cols, 10), q(t_cols, 90)]}),
              flush=True)


if __name__ == '__main__':
    main()
