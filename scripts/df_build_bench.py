#!/usr/bin/env python3
"""Times the device half of tools/prepro_ngrams.py (ciderd.build_df_image: upload, capmi_df_count, the one host read,
capmi_df_finalize, download) on a COCO-sized synthetic corpus against the dict checker tests/df_ref.py on the CPU.

    python scripts/df_build_bench.py [--images 113287] [--reps 5] [--no_cpu]

Corpus: --images images x 5 captions, lengths 8..20 plus the <eos>, Zipfian ids over a vocabulary of 9487.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def corpus(n_img, n_caps=5, lo=8, hi=20, vocab=9487, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n_img * n_caps) + 1                 # + the <eos>
    cap_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    p = np.arange(1, vocab + 1, dtype=np.float64) ** -1.2
    tok = (rng.choice(vocab, size=int(cap_off[-1]), p=p / p.sum()) + 1).astype(np.int32)
    tok[cap_off[1:] - 1] = 0
    return tok, cap_off, np.arange(0, n_img * n_caps + 1, n_caps, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=113287)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no_cpu', action='store_true')
    args = ap.parse_args()
    import torch
    from imagecaptioning.pytorch_amd import ciderd as D
    import df_ref
    tok, cap_off, img_off = corpus(args.images)
    D.build_df_image(*corpus(100), device='cuda:0')                          # warm-up: library, allocator, kernels
    whole, launches = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keys, vals, ref_len = D.build_df_image(tok, cap_off, img_off, device='cuda:0')
        whole.append(time.perf_counter() - t0)
        dev = [torch.from_numpy(a).to('cuda:0') for a in (tok, cap_off, img_off)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D._df_tables(*dev, device='cuda:0')
        torch.cuda.synchronize()
        launches.append(time.perf_counter() - t0)
    out = {'images': args.images, 'tokens': int(len(tok)), 'distinct_ngrams': int(np.count_nonzero(keys)), 'cap': int(keys.shape[0]),
           'device_half_s': sorted(whole), 'device_half_median_s': float(np.median(whole)),
           'resident_corpus_median_s': float(np.median(launches))}
    print(json.dumps(out), flush=True)
    if not args.no_cpu:
        images = [[tok[cap_off[c]:cap_off[c + 1]].tolist() for c in range(img_off[i], img_off[i + 1])] for i in range(args.images)]
        t0 = time.perf_counter()
        df, _ = df_ref.doc_freq(images)
        out['cpu_checker_s'] = time.perf_counter() - t0
        print(json.dumps({'cpu_checker_s': out['cpu_checker_s']}), flush=True)
        t0 = time.perf_counter()
        wk, wv = D.build_table(df)
        out['cpu_build_table_s'] = time.perf_counter() - t0
        out['equal'] = df_ref.pairs(keys, vals) == df_ref.pairs(wk, wv) and keys.shape[0] == wk.shape[0]
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
