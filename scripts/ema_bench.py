#!/usr/bin/env python3
"""Time of the moving-average pass (capmi_ema_step) beside the fused Adam step (capmi_adam_step) on a flat buffer of UpDown's size,
the way the optimizer table of DESIGN.md (Optimizers) was taken: device events around `--launches` back-to-back launches of one
kernel, `--rounds` rounds with the kernels alternating, mean and spread per kernel.  Bytes are what the algorithm needs: Adam 28 per
element (p, m, v read and written, g read), the average 12 (ema read and written, p read).

    python scripts/ema_bench.py [--n 52000000] [--launches 40] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=52000000)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device: a time taken elsewhere says nothing'
    from imagecaptioning.pytorch_amd import ops
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(a.n, device=dev, generator=g)
    grad = torch.randn(a.n, device=dev, generator=g) * 0.01
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    kernels = {
        'adam': (28, lambda t: ops.adam_step(p, grad, m, v, 5e-4, 0.9, 0.999, 1e-8, 0.0, 0.1, 1.0, t)),
        'ema': (12, lambda t: ops.ema_step(ema, p, 0.999, 1, t)),
    }
    for _, fn in kernels.values():          # code objects loaded, buffers touched
        for t in range(1, 6):
            fn(t)
    torch.cuda.synchronize()
    times = {k: [] for k in kernels}
    for _ in range(a.rounds):
        for name, (_, fn) in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t in range(a.launches):
                fn(6 + t)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    out = {'n': a.n, 'launches': a.launches, 'rounds': a.rounds}
    for name, (bytes_per, _) in kernels.items():
        us = sum(times[name]) / len(times[name])
        out[name] = {'us': round(us, 2), 'us_rounds': [round(x, 2) for x in times[name]], 'bytes_per_element': bytes_per,
                     'TBps': round(bytes_per * a.n / us * 1e-6, 3)}
    out['ema_over_adam_TBps'] = round(out['ema']['TBps'] / out['adam']['TBps'], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
