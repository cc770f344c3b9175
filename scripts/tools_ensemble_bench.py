"""Test-time ensembles on one MI355X.

kernel: capmi_ensemble_logprobs against the ATen composition it replaces (AttEnsemble.py:52, softmax x M + stack + mul + div + sum
        + log) at V1 = 9488, rows in {50, 250, 1000}, M in {2, 4}.  Bytes/s counts the least traffic, (M reads + 1 write) x rows x V1
        x 4 B, over the kernel time; the device copy rate of a 1 GiB buffer is measured in the same run for comparison.
e2e:    one eval batch as eval_split runs it (teacher-forced loss + beam 5 decode, bs 10, UpDown configs size, L 20) for ensembles
        of M = 1..4 UpDown models, against the single model with its host-stepped beam search (the same driver, its own stepper)
        and with its one-call native beam search.

    python scripts/tools_ensemble_bench.py [--iters 200] [--batches 5]
"""
import argparse
import os
import sys
import time

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


def kernel(iters):
    from imagecaptioning.pytorch_amd import ops
    dev = 'cuda:0'
    V1 = 9488
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev)     # 1 GiB
    dst = torch.empty_like(src)
    ms = time_cuda(lambda: dst.copy_(src), 20, 3)
    copy_rate = 2 * src.numel() * 4 / (ms * 1e-3)
    print('device copy rate (1 GiB): %.2f TB/s' % (copy_rate / 1e12), flush=True)
    del src, dst
    for M in (2, 4):
        for rows in (50, 250, 1000):
            xs = [torch.randn(rows, V1, device=dev) * 4 for _ in range(M)]
            w = torch.tensor([1.0 + i for i in range(M)], device=dev)
            wl = (w / w.sum()).tolist()
            out = torch.empty(rows, V1, device=dev)
            t_k = time_cuda(lambda: ops.ensemble_logprobs(xs, wl, out=out), iters)
            t_a = time_cuda(lambda: torch.stack([torch.softmax(x, 1) for x in xs], 2).mul(w).div(w.sum()).sum(-1).log(), iters)
            ref = torch.stack([torch.softmax(x.double(), 1) for x in xs], 2).mul(w.double()).div(w.sum().double()).sum(-1).log()
            err = float((out.double() - ref).abs().max())
            nbytes = (M + 1) * rows * V1 * 4
            print('kernel M=%d rows=%4d V1=%d: capmi %.4f ms (%.2f TB/s, %.0f%% of copy)  aten %.4f ms  speed-up %.2fx  max|err| %.1e'
                  % (M, rows, V1, t_k, nbytes / (t_k * 1e-3) / 1e12, 100 * nbytes / (t_k * 1e-3) / copy_rate, t_a, t_a / t_k, err),
                  flush=True)


def e2e(batches):
    from imagecaptioning.pytorch_amd import beam
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.models import AttEnsemble
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion
    from imagecaptioning.pytorch_amd.captioning.utils import opts
    dev = 'cuda:0'
    torch.manual_seed(0)
    opt = opts.parse_opt(['--caption_model', 'updown'])
    opt.vocab = {str(i): 'w%d' % i for i in range(1, opt.vocab_size + 1)}
    members = []
    for i in range(4):
        m = models.setup(opt).to(dev).eval()
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.02 * torch.randn_like(p))
        members.append(m)
    B, n, K, V = 10, 5, 36, opt.vocab_size
    fc = torch.randn(B, opt.fc_feat_size, device=dev).clamp_min(0)
    att = torch.randn(B, K, opt.att_feat_size, device=dev).clamp_min(0)
    labels = torch.randint(1, V + 1, (B, n, 18), device=dev)
    labels[..., 0] = 0
    labels[..., 17:] = 0
    masks = torch.ones(B, n, 18, device=dev)
    bopt = {'sample_method': 'beam_search', 'beam_size': 5, 'sample_n': 1}
    crit = LanguageModelCriterion()

    def batch(model, decode):
        with torch.no_grad():
            crit(model(fc, att, labels[..., :-1], None), labels[..., 1:], masks[..., 1:]).item()
            decode(model)
        torch.cuda.synchronize()

    def own_beam(model):
        model(fc, att, None, opt=dict(bopt), mode='sample')

    def host_beam(model):
        beam.beam_search_steps(model, model._decode_stepper(fc, att, None, model.seq_length), B, V + 1, model.seq_length, dict(bopt), dev)

    def run(label, model, decode):
        batch(model, decode)
        t0 = time.perf_counter()
        for _ in range(batches):
            batch(model, decode)
        print('e2e %-34s %.2f ms per eval batch' % (label, (time.perf_counter() - t0) * 1e3 / batches), flush=True)

    run('single, native one-call beam', members[0], own_beam)
    run('single, host-stepped beam', members[0], host_beam)
    for M in range(1, 5):
        run('ensemble M=%d' % M, AttEnsemble(members[:M]).eval(), own_beam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--batches', type=int, default=5)
    ap.add_argument('--part', choices=('all', 'kernel', 'e2e'), default='all')
    a = ap.parse_args()
    if a.part in ('all', 'kernel'):
        kernel(a.iters)
    if a.part in ('all', 'e2e'):
        e2e(a.batches)


if __name__ == '__main__':
    main()
