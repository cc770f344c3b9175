"""ms per XE step (forward + backward of the model, no optimizer) of NewFC and AoA with and without scheduled sampling, at the sizes
bench.py builds for --config newfc_xe and --config aoa_nsc: bs 10 x 5 captions, T = 16, 36 x 2048 features, train mode with the
configs' dropout.  ss_prob 0 and 0.25 are timed in the same process, alternating in blocks; each step ends in a device
synchronise and the figure is the median over all timed steps of a setting.

    python scripts/tools_ss_bench.py [--steps 40] [--warmup 10] [--blocks 4] [--families newfc,aoa] [--probs 0,0.25]

A tree without scheduled sampling for a family prints `n/a` for its ss_prob 0.25 line (the ss_prob 0 line is what is compared
between two trees; time it with `--probs 0` in both, so that both processes do the same work).
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40, help='timed steps per setting and block')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=4)
    ap.add_argument('--families', default='newfc,aoa')
    ap.add_argument('--probs', default='0,0.25', help='the ss_prob settings to alternate')
    a = ap.parse_args()
    import bench
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    dev = 'cuda:0'
    B, n, K, T = 10, 5, 36, 16
    for fam in a.families.split(','):
        torch.manual_seed(0)
        opt = bench._opt({'newfc': 'newfc', 'aoa': 'aoa_nsc'}[fam])
        model = models.setup(opt).to(dev)
        model.flatten_parameters_()
        model.train()
        V1 = opt.vocab_size + 1
        fc = torch.randn(B, 2048, device=dev).clamp_min(0)
        att = torch.randn(B, K, 2048, device=dev).clamp_min(0)
        am = torch.ones(B, K, device=dev)
        am[:, 30:] = 0
        am[0] = 1
        labels = torch.randint(1, V1, (B, n, T + 2), device=dev)
        labels[..., 0] = 0
        labels[..., T + 1:] = 0
        masks = torch.ones(B, n, T + 2, device=dev)
        crit = LanguageModelCriterion()

        def step():
            logp = model(fc, att, labels[..., :-1], am)
            crit(logp, labels[..., 1:], masks[..., 1:]).backward()

        times = {float(p): [] for p in a.probs.split(',')}
        for p in times:                       # warm up every shape and path the timed window uses
            model.ss_prob = p
            try:
                for _ in range(a.warmup):
                    step()
            except NotImplementedError:
                times[p] = None
        torch.cuda.synchronize()
        for _ in range(a.blocks):
            for p, ts in times.items():
                if ts is None:
                    continue
                model.ss_prob = p
                for _ in range(a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
        for p, ts in times.items():
            if ts is None:
                print('%s xe bs10x5 T16 ss_prob %.2f: n/a (not implemented in this tree)' % (fam, p), flush=True)
                continue
            q = statistics.quantiles(ts, n=10)
            print('%s xe bs10x5 T16 ss_prob %.2f: median %.3f ms per step (p10 %.3f, p90 %.3f, %d steps)'
                  % (fam, p, statistics.median(ts), q[0], q[-1], len(ts)), flush=True)


if __name__ == '__main__':
    main()
