#!/usr/bin/env python3
"""Forward + backward of the distillation loss: the fused route (capmi_distill_loss_fwd / _bwd) against DistillCriterion.generic
(plain torch on the device) in the same run, at the XE shape (N = 320, T = 17, V1 = 9488) and the SCST-batch shape (N = 50).
Device events around `--launches` back-to-back forward+backward pairs, `--rounds` rounds with the routes alternating; mean and
spread (max - min over the rounds) per route.  Bytes are what the algorithm needs: two row reads forward, two reads and one write
backward = 5 * N * T * V1 * 4 (masked positions are not subtracted: the bench masks none).  The moving-average kernel
(capmi_ema_step, 12 bytes per element) is timed in the same rounds as the yardstick of a streaming kernel on this chip.

    python scripts/tools_distill_bench.py [--launches 20] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'imagecaptioning', 'pytorch_amd'))

SHAPES = {'xe': (320, 17, 9488), 'scst_batch': (50, 17, 9488)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--lam', type=float, default=0.7)
    ap.add_argument('--tau', type=float, default=2.0)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device: a time taken elsewhere says nothing'
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd.captioning.modules.losses import DistillCriterion
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(0)
    crit = DistillCriterion(a.lam, a.tau)
    n_ema = 52000000
    p, ema = torch.randn(n_ema, device=dev, generator=g), torch.zeros(n_ema, device=dev)
    out = {'launches': a.launches, 'rounds': a.rounds, 'lambda': a.lam, 'tau': a.tau}
    for tag, (N, T, V1) in SHAPES.items():
        lt = torch.log_softmax(2 * torch.randn(N, T, V1, device=dev, generator=g), 2)
        ls = torch.log_softmax(lt + 0.5 * torch.randn(N, T, V1, device=dev, generator=g), 2).requires_grad_(True)
        tok = torch.randint(0, V1, (N, T), device=dev, generator=g)
        mask = torch.ones(N, T, device=dev)
        one = torch.ones((), device=dev)

        def fused():
            ls.grad = None
            crit(ls, lt, tok, mask)['loss'].backward(one)

        def generic():
            ls.grad = None
            crit.generic(ls, lt, tok, mask)['loss'].backward(one)

        routes = {'fused': fused, 'generic': generic, 'ema': lambda: ops.ema_step(ema, p, 0.999, 1, 10)}
        for fn in routes.values():              # code objects loaded, allocator warmed
            for _ in range(3):
                fn()
        fused()
        g_f = ls.grad.clone()
        generic()
        same = float((g_f - ls.grad).abs().max() / ls.grad.abs().max())
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for name, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        floor_bytes = 5 * N * T * V1 * 4
        res = {'N': N, 'T': T, 'V1': V1, 'floor_bytes': floor_bytes, 'grad_rel_diff_fused_vs_generic': same}
        for name in routes:
            ts = times[name]
            us = sum(ts) / len(ts)
            nbytes = 12 * n_ema if name == 'ema' else floor_bytes
            res[name] = {'us': round(us, 1), 'us_rounds': [round(x, 1) for x in ts], 'spread_us': round(max(ts) - min(ts), 1),
                         'TBps_of_floor_bytes': round(nbytes / us * 1e-6, 3)}
        res['generic_over_fused'] = round(res['generic']['us'] / res['fused']['us'], 2)
        out[tag] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
