#!/usr/bin/env python3
"""capmi_region_rows_build (csrc/region_rows.hip) at the COCO shape -- 64 newly drawn images of 36 x 2048 fp32 regions per launch --
against the host path it replaces for the resident store (numpy: norm_att_feat, the box columns, norm_box_feat, the append and
Python's sorted over the rows, captioning/data/feature_loader.py).  Device events around `reps` launches, warm, the variants
alternating round by round; median and spread over the rounds.  Bytes: every raw row read once, every store row written once.
    python scripts/region_rows_bench.py [rounds] [reps]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd'))
from imagecaptioning.pytorch_amd import ops                                              # noqa: E402
from captioning.data.feature_loader import append_boxes                                   # noqa: E402

N_IMG, K, D = 64, 36, 2048
HBM_TBS = 8.0                       # MI355X peak HBM3E bandwidth, TB/s


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    assert torch.cuda.is_available(), 'needs a HIP device: a CPU run measures nothing'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    att = np.clip(rng.standard_normal((N_IMG * K, D)), 0, None).astype(np.float32) + np.float32(0.01)
    x1, y1 = rng.uniform(0, 300, N_IMG * K), rng.uniform(0, 200, N_IMG * K)
    box = np.stack([x1, y1, x1 + rng.uniform(20, 300, N_IMG * K), y1 + rng.uniform(20, 250, N_IMG * K)], 1).astype(np.float32)
    table = np.zeros((N_IMG, 4), dtype=np.int32)
    table[:, 0], table[:, 1], table[:, 2], table[:, 3] = np.arange(N_IMG) * K, K, 480, 640
    src, bx, tab = torch.from_numpy(att).to(dev), torch.from_numpy(box).to(dev), torch.from_numpy(table).to(dev)
    variants = {'norm_att only (use_box 0)': (1, 0, 0), 'use_box + norm_box': (0, 1, 1), 'norm_att + use_box + norm_box': (1, 1, 1)}
    dst = {name: torch.zeros(N_IMG * K + 1, D + 5 * f[1], device=dev)[1:] for name, f in variants.items()}     # store rows start at row 1
    times = {name: [] for name in variants}
    for rnd in range(rounds + 1):                                  # round 0 warms every variant up
        for name, (na, ub, nb) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.region_rows_build(src, bx if ub else None, table, tab, dst[name], na, ub, nb)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) * 1e3 / reps)            # us per launch
    for name, (na, ub, nb) in variants.items():
        t = times[name]
        med = statistics.median(t)
        nbytes = N_IMG * K * 4 * (D + (4 if ub else 0) + D + 5 * ub)
        print('kernel  %-30s %7.2f us per launch of %d images (min %.2f, max %.2f over %d rounds x %d) = %.3f us per image, '
              '%.2f TB/s of %.1f MB moved (floor at %.0f TB/s: %.2f us)'
              % (name, med, N_IMG, min(t), max(t), rounds, reps, med / N_IMG, nbytes / med / 1e6, nbytes / 1e6, HBM_TBS,
                 nbytes / HBM_TBS / 1e6), flush=True)
    # the host path, one image at a time as the decode pool runs it (single thread)
    host = {name: [] for name in variants}
    for rnd in range(rounds + 1):
        for name, (na, ub, nb) in variants.items():
            t0 = time.perf_counter()
            for i in range(N_IMG):
                a = att[i * K:(i + 1) * K]
                if na:
                    a = a / np.linalg.norm(a, 2, 1, keepdims=True)
                if ub:
                    a = append_boxes(a, box[i * K:(i + 1) * K], 480, 640, nb)
            if rnd:
                host[name].append((time.perf_counter() - t0) * 1e6 / N_IMG)
    for name in variants:
        t = host[name]
        print('host    %-30s %7.1f us per image, one CPU thread (min %.1f, max %.1f over %d rounds)'
              % (name, statistics.median(t), min(t), max(t), rounds), flush=True)


if __name__ == '__main__':
    main()
