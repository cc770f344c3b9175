#!/usr/bin/env python3
"""The numbers of DESIGN.md's section on discriminative decoding (imagecaptioning/pytorch_amd/disc.py, csrc/disc.hip).

Kernel: capmi_disc_combine at `--images` x `--beam` hypotheses, V1 = `--v1`, D = 1 and D = 5, both modes, beside the torch
composition of the same result (log_softmax per slot, logsumexp over the distractor slots, the arithmetic) -- the yardstick.  Device
events around `--launches` back-to-back launches, `--rounds` rounds with the candidates alternating, mean per candidate.  GB/s counts
what the algorithm needs: (1 + D) rows read once and one row written per hypothesis.

--eval 1: seconds per batch of a beam search of the UpDown model at the configuration sizes (R = E = 1000, A = 512, 36 x 2048 region
features, V1 = `--v1`, random weights) on `--images` images with beam `--beam`: without the option, with D = 1 and with D = 5 nearest
distractors, and the prefill of the B (1 + D) feature slots alone (its share of the call).

    python scripts/tools_disc_bench.py [--images 50] [--beam 5] [--v1 9488] [--launches 40] [--rounds 3] [--eval 1] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches           # us per launch


def torch_composition(x, w, mode, B, D1, cur):
    """the same rows with ATen: every slot normalised, the distractor slots mixed, the arithmetic (every slot present)"""
    lp = torch.log_softmax(x.view(B, D1, cur, -1), -1)
    lt = lp[:, 0]
    if mode == 'suppress':
        return lt - w * (torch.logsumexp(lp[:, 1:], 1) - math.log(D1 - 1))
    return lt + w * (lt - torch.logsumexp(lp, 1))


def kernel_numbers(a, dev):
    from imagecaptioning.pytorch_amd import ops
    out = {}
    B, cur, V1 = a.images, a.beam, a.v1
    for D in (1, 5):
        D1 = 1 + D
        x = torch.randn(B * D1 * cur, V1, device=dev, generator=torch.Generator(device=dev).manual_seed(D)) * 3.0
        present = torch.ones(B, D1, dtype=torch.uint8, device=dev)
        res = torch.empty(B * cur, V1, device=dev)
        nbytes = 4 * V1 * B * cur * (D1 + 1)
        cands = {}
        for mode in ('suppress', 'listener'):
            cands['capmi_' + mode] = (lambda mode=mode: ops.disc_combine(x, present, 0.5, mode, B, D1, cur, res))
            cands['torch_' + mode] = (lambda mode=mode: torch_composition(x, 0.5, mode, B, D1, cur))
        for mode in ('suppress', 'listener'):             # the two must agree before their times are compared
            err = float((cands['capmi_' + mode]() - cands['torch_' + mode]().view(B * cur, V1)).abs().max())
            assert err < 1e-4, (mode, err)
        for fn in cands.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cands}
        for _ in range(a.rounds):
            for k, fn in cands.items():
                times[k].append(timed(fn, a.launches))
        for k, ts in times.items():
            us = sum(ts) / len(ts)
            out['D%d_%s' % (D, k)] = {'us': round(us, 2), 'us_rounds': [round(t, 2) for t in ts], 'GBps': round(nbytes / us * 1e-3, 1)}
        out['D%d_bytes' % D] = nbytes
    return out


def eval_numbers(a, dev):
    import argparse as ap
    from imagecaptioning.pytorch_amd import disc
    from imagecaptioning.pytorch_amd.captioning import models
    V = a.v1 - 1
    o = ap.Namespace(caption_model='updown', vocab_size=V, input_encoding_size=1000, rnn_size=1000, num_layers=2, drop_prob_lm=0.5,
                     seq_length=20, max_length=20, fc_feat_size=2048, att_feat_size=2048, att_hid_size=512, use_bn=0, logit_layers=1,
                     vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    torch.manual_seed(1234)
    model = models.setup(o).to(dev).eval()
    B = a.images
    gen = torch.Generator(device=dev).manual_seed(7)
    fc = torch.randn(B, 2048, device=dev, generator=gen)
    att = torch.randn(B, 36, 2048, device=dev, generator=gen)
    base = {'beam_size': a.beam, 'sample_n': 1, 'sample_method': 'greedy'}
    calls = {'plain': dict(base)}
    for D in (1, 5):
        calls['D%d' % D] = dict(base, distractors=disc.pick_nearest(att, None, D), disc_lambda=0.5)
    # the stepper-driven search without the option (decoding_constraint routes the plain call off the one-call native search)
    calls['plain_stepped'] = dict(base, decoding_constraint=1)

    def prefill(D):
        idx = torch.arange(B * (1 + D), device=dev) % B
        return lambda: model._decode_stepper(fc[idx], att[idx], None, 20)

    def run(opt):
        def fn():
            with torch.no_grad():
                model(fc, att, None, opt=dict(opt), mode='sample')
        return fn
    cands = {k: run(v) for k, v in calls.items()}
    cands.update({'prefill_D%d' % D: prefill(D) for D in (0, 1, 5)})
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, 2) * 1e-6)
    return {k: {'s_per_batch': round(sum(ts) / len(ts), 4), 's_rounds': [round(t, 4) for t in ts]} for k, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=50)
    ap.add_argument('--beam', type=int, default=5)
    ap.add_argument('--v1', type=int, default=9488)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--eval', type=int, default=0)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device: a time taken elsewhere says nothing'
    dev = torch.device('cuda', 0)
    out = {'images': a.images, 'beam': a.beam, 'V1': a.v1, 'launches': a.launches, 'rounds': a.rounds, 'kernel': kernel_numbers(a, dev)}
    if a.eval:
        out['eval'] = eval_numbers(a, dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
