#!/usr/bin/env python3
"""Timing of the constrained beam search (csrc/cbs.hip, beam.constrained_beam_search_steps), on the device, with device events:

  * one capmi_cbs_select step at 16 rows per image, (C, b) = (2, 4) and (3, 2), beside one capmi_beam_select step at cur = bd = 16 on
    the same rows, alternating in one run (both stream the same logp bytes);
  * one tools/eval.py pass (updown, 100 synthetic images): constrained at (C, b) = (2, 4), plain at --beam_size 4 and --beam_size 16
    (the equal-row comparison), wall-clock after a warm-up pass.

    python scripts/cbs_bench.py [--reps 200] [--out FILE.json] [--no_eval]

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.sbs_bench import timed      # noqa: E402


def select_steps(B, C, b, V1, reps):
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import lib, ptr, check, stream_ptr
    dev = 'cuda'
    S = 1 << C
    SB = S * b
    g = torch.Generator(device=dev).manual_seed(B * 100 + SB)
    logp = torch.log_softmax(torch.randn(B * SB, V1, device=dev, generator=g) * 3, 1).contiguous()
    sums = -torch.rand(B, SB, device=dev, generator=g) * 20
    words = torch.full((B, 4, 8), -1, dtype=torch.int32)
    words[:, :C, :2] = torch.randint(1, V1, (B, C, 2), dtype=torch.int32)
    tables = ops.cbs_tables(words, torch.full((B,), C, dtype=torch.int32), V1, S, dev)
    out = ops.cbs_select(logp, sums, tables, b, S)
    bo = (torch.empty(B, SB, dtype=torch.int32, device=dev), torch.empty(B, SB, dtype=torch.long, device=dev),
          torch.empty(B, SB, device=dev), torch.empty(B, SB, device=dev), torch.empty(B, SB, dtype=torch.uint8, device=dev))
    st = stream_ptr()

    def cbs():
        ops.cbs_select(logp, sums, tables, b, S, out=out)

    def beam():
        check(lib.capmi_beam_select(ptr(logp), ptr(sums), B, SB, SB, V1, 0, *[ptr(t) for t in bo], st), 'beam_select')
    res = {}
    for _ in range(2):                                                       # alternate the two
        for name, fn in (('cbs_select_us', cbs), ('beam_select_us', beam)):
            med, lo = timed(fn, reps)
            res[name] = min(res.get(name, med), med)
            res[name + '_min'] = min(res.get(name + '_min', lo), lo)
    res.update(B=B, C=C, b=b, rows_per_image=SB, V1=V1, ratio=res['cbs_select_us'] / res['beam_select_us'],
               logp_mib=logp.numel() * 4 / 2 ** 20)
    return res


def eval_passes(images=100):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'imagecaptioning', 'pytorch_amd')
    sys.path.insert(0, pkg)
    from captioning.utils import opts
    from imagecaptioning.pytorch_amd.tools import eval as E
    tmp = tempfile.mkdtemp()
    base = ['--caption_model', 'updown', '--num_images', str(images), '--synthetic_images', str(2 * images), '--split', 'val',
            '--batch_size', '50', '--eval_results_dir', tmp]
    _, vocab = E.build_loader(opts.parse_opt(base), torch.device('cuda'))
    first = E.main(opts.parse_opt(base + ['--beam_size', '4']))              # warm-up; its ids name the constrained images
    ids = [p['image_id'] for p in first[1]]
    spec = {str(i): [[vocab[str(100 + (k % 50))], vocab[str(200 + (k % 50))]], [vocab[str(300 + (k % 70))]]] for k, i in enumerate(ids)}
    path = os.path.join(tmp, 'constraints.json')
    with open(path, 'w') as f:
        json.dump(spec, f)
    res = dict(what='eval_pass', images=images)
    for name, extra in (('cbs_C2_b4_s', ['--beam_size', '4', '--constraints_json', path]), ('beam4_s', ['--beam_size', '4']),
                        ('beam16_s', ['--beam_size', '16'])):
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = E.main(opts.parse_opt(base + extra))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        res[name] = best
        if 'cbs' in name:
            res['fully_satisfied'] = sum(p['constraints_satisfied'] == p['constraints_total'] for p in out[1]) / len(out[1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default='')
    ap.add_argument('--no_eval', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the device'
    lines = []
    for C, b in ((2, 4), (3, 2)):
        lines.append(dict(what='select_step', **select_steps(50, C, b, 9488, a.reps)))
        print(json.dumps(lines[-1]), flush=True)
    if not a.no_eval:
        lines.append(eval_passes())
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == '__main__':
    main()
