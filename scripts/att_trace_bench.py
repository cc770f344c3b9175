#!/usr/bin/env python3
"""Time the decode call of tools/eval.py's eval_split (UpDown at the command line's default sizes: 10 images x 36 x 2048, L = 20,
vocabulary 9487) with return_attention off and, where the tree has it, on; and the three trace kernels alone.

    python scripts/att_trace_bench.py [--tree DIR] [--windows 7] [--kernels 1]

--tree DIR: measure the package of another checkout (DIR/imagecaptioning/...) with this harness -- a parent commit beside the
working tree; run one process per tree and alternate them ("Per-word region attention").  A process warms every setting
for --warm_s seconds, then times --windows windows of about --window_s seconds each per setting, the settings alternating inside
a round; a window is a host clock around calls that end in a device synchronise.  Prints one JSON line: per setting the window
times in ms per call.
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--windows', type=int, default=7)
ap.add_argument('--window_s', type=float, default=0.6)
ap.add_argument('--warm_s', type=float, default=1.0)
ap.add_argument('--kernels', type=int, default=0)
ap.add_argument('--tag', default='')
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, 'imagecaptioning', 'pytorch_amd'))

import torch      # noqa: E402
from captioning.utils import opts      # noqa: E402
from captioning import models          # noqa: E402

dev = 'cuda:0'
opt = opts.parse_opt(['--caption_model', 'updown'])
opt.vocab = {str(i): 'w%d' % i for i in range(1, opt.vocab_size + 1)}
torch.manual_seed(1234)
model = models.setup(opt).to(dev).eval()
has_trace = hasattr(model, 'last_attention')
B, K, L = 10, 36, opt.max_length
fc = torch.randn(B, opt.fc_feat_size, device=dev).clamp_min(0)
att = torch.randn(B, K, opt.att_feat_size, device=dev).clamp_min(0)

settings = {}
for name, kw in (('greedy', dict(sample_method='greedy', beam_size=1, sample_n=1)),
                 ('beam5', dict(sample_method='greedy', beam_size=5, sample_n=1))):
    settings[name + '_off'] = kw
    if has_trace:
        settings[name + '_on'] = dict(kw, return_attention=1)


def calls(kw, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        model(fc, att, None, opt=dict(kw), mode='sample')
    torch.cuda.synchronize()
    return time.perf_counter() - t0


res = {'tree': tree, 'tag': args.tag, 'trace': has_trace, 'ms_per_call': {k: [] for k in settings}}
per_window = {}
with torch.no_grad():
    for k, kw in settings.items():
        calls(kw, 5)
        t, n = 0.0, 0
        while t < args.warm_s:                     # warm: code objects loaded, clocks up
            t += calls(kw, 20)
            n += 20
        per_window[k] = max(20, int(args.window_s / (t / n)))
    for _ in range(args.windows):
        for k, kw in settings.items():
            res['ms_per_call'][k].append(round(calls(kw, per_window[k]) / per_window[k] * 1e3, 4))
res['calls_per_window'] = per_window

if args.kernels and has_trace:
    from imagecaptioning.pytorch_amd import att_trace

    def kernel_us(fn, iters=2000, reps=5):
        out = []
        for _ in range(200):
            fn()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(round(e0.elapsed_time(e1) / iters * 1e3, 3))
        return out

    # 10 rows x 20 steps x 36 regions, as the decode above; the figure spans the wrapper's output allocation and enqueue as well
    # (back-to-back calls between two device events): an upper bound of the kernel's own time
    alpha = torch.rand(L, B, K, device=dev)
    seq = torch.randint(1, 100, (B, L), device=dev)
    rows = torch.rand(L, B * 5, K, device=dev)
    lineage = torch.randint(0, B * 5, (L, B), device=dev).to(torch.int32)
    length = torch.full((B,), L, dtype=torch.int32, device=dev)
    a = att_trace.rollout(alpha, seq, K)
    res['kernel_us'] = dict(rollout=kernel_us(lambda: att_trace.rollout(alpha, seq, K)),
                            beam=kernel_us(lambda: att_trace.beam(rows, lineage, length, K)),
                            ground=kernel_us(lambda: att_trace.ground(a)))
print(json.dumps(res))
