#!/usr/bin/env python3
"""The compact resident store (csrc/resident.hip) at the COCO shape.

  assembly: one batch out of a warm store of 4096 x 36 rows of 2048 features, B = 10 and B = 50, every K = 36.  `parent` is the batch
            assembly the store used before capmi_resident_gather (a [B, kmax] int64 index built in numpy, uploaded, index_select);
            `fp32` / `bf16` / `fp16` upload one pinned [B, 2] table and launch the gather.  The variants alternate inside every
            round; per variant the device time per batch (events around REPS batches) and the host time per batch (wall clock of
            the enqueueing loop, no synchronise inside) are medians over the rounds, the spread is (max - min) / median.
  narrow:   capmi_rows_narrow over 64 Ki rows x 2048 (512 MiB read, 256 MiB written), bytes moved over the event time.

    python scripts/resident_bench.py [rounds] [reps]          -> one JSON line"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from imagecaptioning.pytorch_amd import ops                         # noqa: E402

HBM_MEASURED = 6.29e12          # bytes/s, float4 copy


def parent_assembly(rows, firsts, K):
    B = len(firsts)
    gather = np.zeros((B, K), dtype=np.int64)
    for b, r0 in enumerate(firsts):
        gather[b, :K] = np.arange(r0, r0 + K)
    return rows.index_select(0, torch.from_numpy(gather.reshape(-1)).to(rows.device)).view(B, K, rows.shape[1])


def gather_assembly(rows, firsts, K):
    pinned = torch.zeros(len(firsts), 2, dtype=torch.int32, pin_memory=True)
    table = pinned.numpy()
    for b, r0 in enumerate(firsts):
        table[b] = (r0, K)
    return ops.resident_gather(rows, table, pinned.to(rows.device, non_blocking=True), K)[0]


def main():
    assert torch.cuda.is_available(), 'a measurement needs the device'
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    dev = torch.device('cuda:0')
    n_img, K, F = 4096, 36, 2048
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.relu(torch.randn(1 + n_img * K, F, device=dev, generator=g))
    base[0] = 0
    stores = {'parent': base, 'fp32': base, 'bf16': base.to(torch.bfloat16), 'fp16': base.to(torch.float16)}
    rng = np.random.default_rng(0)
    out = {'shape': {'images': n_img, 'K': K, 'F': F}, 'rounds': rounds, 'reps': reps, 'assembly': {}}
    for B in (10, 50):
        draws = [[1 + K * int(i) for i in rng.integers(0, n_img, B)] for _ in range(reps)]
        want = parent_assembly(base, draws[0], K)
        for name, rows in stores.items():                          # the outputs first: equal to the parent's, rounded once
            got = (parent_assembly if name == 'parent' else gather_assembly)(rows, draws[0], K)
            assert torch.equal(got, want if rows.dtype == torch.float32 else want.to(rows.dtype).float()), name
        dev_us = {n: [] for n in stores}
        host_us = {n: [] for n in stores}
        for rnd in range(rounds + 1):                              # round 0 warms every variant up
            for name, rows in stores.items():
                fn = parent_assembly if name == 'parent' else gather_assembly
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for firsts in draws:
                    fn(rows, firsts, K)
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                if rnd:
                    dev_us[name].append(e0.elapsed_time(e1) * 1e3 / reps)
                    host_us[name].append((t1 - t0) * 1e6 / reps)
        res = {}
        for name in stores:
            d, h = np.array(dev_us[name]), np.array(host_us[name])
            res[name] = {'device_us_per_batch': float(np.median(d)), 'device_spread': float((d.max() - d.min()) / np.median(d)),
                         'host_us_per_batch': float(np.median(h)), 'host_spread': float((h.max() - h.min()) / np.median(h))}
        out['assembly']['B%d' % B] = res
    del stores
    count = (64 << 10) * F
    src = torch.relu(torch.randn(count, device=dev, generator=g))
    out['narrow'] = {'elements': count, 'hbm_measured_bytes_per_s': HBM_MEASURED}
    for name, dt in (('bf16', torch.bfloat16), ('fp16', torch.float16)):
        dst = torch.empty(count, dtype=dt, device=dev)
        ts = []
        for rnd in range(rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                ops.rows_narrow(src, dst)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                ts.append(e0.elapsed_time(e1) * 1e-3 / 10)
        assert torch.equal(dst.view(torch.int16), src.to(dt).view(torch.int16))
        t = float(np.median(ts))
        out['narrow'][name] = {'seconds': t, 'bytes_per_s': 6 * count / t, 'share_of_measured_hbm': 6 * count / t / HBM_MEASURED,
                               'spread': float((max(ts) - min(ts)) / t)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
