#!/usr/bin/env python3
"""Timing of the caption scoring (csrc/score.hip, imagecaptioning/pytorch_amd/score.py), on the device, with device events:

  * one capmi_score_step at rows x V1 = 8000 x 9488 beside the ATen composition of the same step (log_softmax + gather + masked
    add), alternating in one run; the logits (304 MB) are larger than the 256 MB Infinity Cache, so both stream them from HBM;
  * a pool-1000 self-retrieval -- 1000 captions against 1000 images, 10^6 pairs -- of the UpDown model at its configured size on
    synthetic features: score.score_captions with pairing 'cross', then capmi_retrieval_rank; wall-clock around a device
    synchronise, after a warm-up call on a small pool.

    python scripts/tools_score_bench.py [--reps 100] [--pool 1000] [--out FILE.json] [--no_retrieval]

Prints one JSON line per measurement.  Nothing here is a pass/fail threshold."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.sbs_bench import timed      # noqa: E402


def score_steps(rows, V1, reps):
    from imagecaptioning.pytorch_amd import ops
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(rows + V1)
    logits = torch.randn(rows, V1, device=dev, generator=g) * 3
    tok = torch.randint(1, V1, (rows,), device=dev, generator=g)
    live = torch.ones(rows, dtype=torch.uint8, device=dev)
    acc = torch.zeros(rows, device=dev)
    cnt = torch.zeros(rows, dtype=torch.int32, device=dev)
    tl = torch.zeros(rows, device=dev)
    live_b, acc_a, cnt_a = live.bool(), torch.zeros(rows, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)

    def native():
        ops.score_step(logits, tok, live, acc, cnt, tl)

    def aten():
        lp = torch.log_softmax(logits, 1).gather(1, tok.unsqueeze(1)).squeeze(1)
        acc_a.add_(torch.where(live_b, lp, lp.new_zeros(())))
        cnt_a.add_(live_b.int())
    res = {}
    for _ in range(2):                                                       # alternate the two
        for name, fn in (('score_step_us', native), ('aten_us', aten)):
            med, lo = timed(fn, reps)
            res[name] = min(res.get(name, med), med)
            res[name + '_min'] = min(res.get(name + '_min', lo), lo)
    nbytes = rows * V1 * 4
    res.update(rows=rows, V1=V1, logits_mb=nbytes / 1e6, score_step_tb_s=nbytes / res['score_step_us'] / 1e6,
               aten_over_native=res['aten_us'] / res['score_step_us'],
               max_abs_diff=float((acc / cnt.float() - acc_a / cnt_a.float()).abs().max()))
    return res


def self_retrieval(pool, L=20):
    from imagecaptioning.pytorch_amd import ops, score, synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    dev = 'cuda'
    torch.manual_seed(7)
    model = models.setup(synthetic.updown_opt()).to(dev).eval()
    V1 = model.vocab_size + 1
    fc, att = synthetic.batch(pool, seed=5, device=dev)
    g = torch.Generator().manual_seed(3)
    seqs = torch.randint(1, V1, (pool, L), generator=g)
    for k in range(pool):                                                    # lengths 8 .. 16 words, as COCO captions run
        seqs[k, int(torch.randint(8, 17, (1,), generator=g)):] = 0
    seqs = seqs.to(dev)
    target = torch.arange(pool)
    score.score_captions(model, fc[:8], att[:8], None, seqs[:8], {'pairing': 'cross'})         # warm-up
    res = dict(what='self_retrieval', pool=pool, L=L, V1=V1, score_rows=score.default_rows(V1, model.rnn_size))
    best = None
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S = score.score_captions(model, fc, att, None, seqs, {'pairing': 'cross'})
        rank, post = ops.retrieval_rank(S, target)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        if dt > 60:
            break
    steps = int(model.last_score['len'].max())
    res.update(seconds=best, pairs=pool * pool, steps=steps, logit_bytes_read=float(pool) * pool * steps * V1 * 4,
               us_per_pair=best * 1e6 / (pool * pool), median_rank=float(rank.float().median()))
    t, lo = timed(lambda: ops.retrieval_rank(S, target), 50)
    res.update(retrieval_rank_us=t, retrieval_rank_us_min=lo)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--pool', type=int, default=1000)
    ap.add_argument('--out', default='')
    ap.add_argument('--no_retrieval', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the device'
    lines = [dict(what='score_step', **score_steps(8000, 9488, a.reps))]
    print(json.dumps(lines[-1]), flush=True)
    if not a.no_retrieval:
        lines.append(self_retrieval(a.pool))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == '__main__':
    main()
