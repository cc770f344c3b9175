"""use_bn on one MI355X: the region statistics against ATen's batch_norm on the same tensors.

stats:  ops.bn_stats (capmi_bn_stats + capmi_bn_finalize: batch mean / rstd over the valid rows, running buffers updated) and
        ops.bn_stats + ops.bn_apply (the normalised rows too) at [360, 2048] (the SCST prefill, bs 10 x 36 regions) and [6400, 2048]
        (an XE batch), against torch.nn.functional.batch_norm(training=True), which does both.  Bytes/s counts the least traffic:
        one read of x for the statistics, one read and one write more for the apply.

    python scripts/tools_bn_bench.py [--iters 200]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_cuda(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters       # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    args = ap.parse_args()
    from imagecaptioning.pytorch_amd import ops
    dev = 'cuda:0'
    for rows, D in ((360, 2048), (6400, 2048), (360, 2053), (6400, 2053)):
        x = torch.randn(rows, D, device=dev).clamp_min(0)
        g, b = torch.rand(D, device=dev) + 0.5, torch.randn(D, device=dev)
        rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
        nbt = torch.zeros((), dtype=torch.long, device=dev)
        y = torch.empty_like(x)

        def both():
            st = ops.bn_stats(x, None, True, rm, rv, nbt)
            ops.bn_apply(x, None, st[3], st[1], g, b, out=y)
        t_s = time_cuda(lambda: ops.bn_stats(x, None, True, rm, rv, nbt), args.iters)
        t_b = time_cuda(both, args.iters)
        rm2, rv2 = torch.zeros(D, device=dev), torch.ones(D, device=dev)
        t_a = time_cuda(lambda: torch.nn.functional.batch_norm(x, rm2, rv2, g, b, True, 0.1, 1e-5), args.iters)
        nb = rows * D * 4
        print('[%d, %d]: stats %.4f ms (%.2f TB/s)  stats+apply %.4f ms (%.2f TB/s)  aten batch_norm %.4f ms (%.2f TB/s)'
              % (rows, D, t_s, nb / (t_s * 1e-3) / 1e12, t_b, 3 * nb / (t_b * 1e-3) / 1e12, t_a, 3 * nb / (t_a * 1e-3) / 1e12),
              flush=True)


if __name__ == '__main__':
    main()
