#!/usr/bin/env python3
"""Timing of the stochastic beam search (csrc/sbs.hip, beam.stochastic_beam_search_steps) beside the deterministic beam search, on
the device, with device events:

  * one capmi_sbs_select step (in-kernel Philox noise) beside one capmi_beam_select step at the same shape, alternating in one run;
  * a whole sample_method='sbs' decode of an UpDown model beside its host-stepped and its one-call beam search at equal k.

    python scripts/sbs_bench.py [--reps 200] [--out FILE.json]

Shapes: B = 10, 50 images, bd = 5, 10, V1 = 9488 (the evaluation shapes).  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=20):
    """median and min microseconds per call over `reps` calls in 10 event-timed windows"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per, out = max(reps // 10, 1), []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / per)
    out.sort()
    return out[len(out) // 2], out[0]


def select_steps(B, bd, V1, reps):
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import lib, ptr, check, stream_ptr
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(B * 100 + bd)
    logp = torch.log_softmax(torch.randn(B * bd, V1, device=dev, generator=g) * 3, 1).contiguous()
    phi = -torch.rand(B, bd, device=dev, generator=g) * 20
    gg = phi + 1.0
    alive = torch.ones(B, bd, dtype=torch.uint8, device=dev)
    out = ops.sbs_select(logp, phi, gg, alive, bd, seed=1, offset=1)
    bo = (torch.empty(B, bd, dtype=torch.int32, device=dev), torch.empty(B, bd, dtype=torch.long, device=dev),
          torch.empty(B, bd, device=dev), torch.empty(B, bd, device=dev), torch.empty(B, bd, dtype=torch.uint8, device=dev))
    st = stream_ptr()

    def sbs():
        ops.sbs_select(logp, phi, gg, alive, bd, seed=1, offset=1, out=out)

    def beam():
        check(lib.capmi_beam_select(ptr(logp), ptr(phi), B, bd, bd, V1, 0, *[ptr(t) for t in bo], st), 'beam_select')
    res = {}
    for _ in range(2):                                                       # alternate the two
        for name, fn in (('sbs_select_us', sbs), ('beam_select_us', beam)):
            med, lo = timed(fn, reps)
            res[name] = min(res.get(name, med), med)
            res[name + '_min'] = min(res.get(name + '_min', lo), lo)
    res.update(B=B, bd=bd, V1=V1, ratio=res['sbs_select_us'] / res['beam_select_us'], logp_mib=logp.numel() * 4 / 2 ** 20)
    return res


def decodes(B, k, V1, reps):
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    torch.manual_seed(1)
    opt = opts.parse_opt(['--caption_model', 'updown'])
    opt.vocab_size = V1 - 1
    opt.vocab = {str(i): 'w%d' % i for i in range(1, V1)}
    model = models.setup(opt).cuda().eval()
    fc = torch.randn(B, opt.fc_feat_size, device='cuda')
    att = torch.randn(B, 36, opt.att_feat_size, device='cuda')

    def run(**o):
        def fn():
            with torch.no_grad():
                model(fc, att, None, opt=dict(o), mode='sample')
        return fn
    res = dict(B=B, k=k, V1=V1, L=model.seq_length)
    for name, o in (('sbs_ms', dict(sample_method='sbs', sample_n=k)),
                    ('bs_hoststepped_ms', dict(sample_method='beam_search', beam_size=k, sample_n=k, decoding_constraint=1)),
                    ('bs_onecall_ms', dict(sample_method='beam_search', beam_size=k, sample_n=k)),
                    ('sample_n_ms', dict(sample_method='sample', sample_n=k))):
        med, lo = timed(run(**o), max(reps // 10, 10), warmup=3)
        res[name], res[name + '_min'] = med / 1e3, lo / 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the device'
    lines = []
    for B in (10, 50):
        for bd in (5, 10):
            lines.append(dict(what='select_step', **select_steps(B, bd, 9488, a.reps)))
            print(json.dumps(lines[-1]), flush=True)
    for B in (10, 50):
        for k in (5, 10):
            lines.append(dict(what='decode', **decodes(B, k, 9488, a.reps)))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == '__main__':
    main()
