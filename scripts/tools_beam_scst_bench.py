"""ms per beam-search SCST step (train_sample_method greedy, train_beam_size 5 = train_sample_n 5) at the size of BASELINE
configs[2] (B = 10, L = 20, V1 9488, dropout 0.5) for UpDown and NewFC, split by events into search / finalise + mask gather /
replay forward / backward, with the sampled SCST step of the same build beside it and the host assembly
(beam.assemble_done_beams on the same tables) that capmi_beam_finalize replaces.  Forward + RewardCriterion + backward of the
model only (no reward computation, no optimizer); the variants alternate in one process, every step is synchronised.

    python scripts/tools_beam_scst_bench.py [--steps 30] [--warmup 5] [--once updown|newfc]

--once runs two beam-search steps of one model and nothing else: the process to put behind a kernel trace.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(t):
    t = sorted(t)
    return '%.3f ms (p10 %.3f, p90 %.3f)' % (t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--once', choices=('updown', 'newfc'), default=None)
    a = ap.parse_args()
    from imagecaptioning.pytorch_amd import beam, synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules.losses import RewardCriterion
    torch.manual_seed(0)
    dev = 'cuda:0'
    B, n, L = 10, 5, 20
    fc, att = synthetic.batch(B, device=dev)
    reward = torch.randn(B * n, L, device=dev)

    def build(name):
        m = models.setup(synthetic.updown_opt(caption_model=name)).to(dev)
        m.flatten_parameters_()
        m.train()
        return m

    def step(model, o):
        seq, slp = model(fc, att, None, opt=o, mode='sample')
        RewardCriterion()(slp, seq, reward).backward()

    beam_o = {'sample_method': 'greedy', 'beam_size': n, 'sample_n': n}
    samp_o = {'sample_method': 'sample', 'sample_n': n}
    if a.once:
        model = build(a.once)
        for _ in range(2):
            step(model, beam_o)
        torch.cuda.synchronize()
        return
    built = {k: build(k) for k in ('updown', 'newfc')}
    total = {(k, v): [] for k in built for v in ('beam', 'sample')}
    parts = {(k, ph): [] for k in built for ph in ('search', 'finalize', 'replay', 'backward')}
    host = {k: [] for k in built}
    for i in range(a.warmup + a.steps):
        for k, model in built.items():
            for v, o in (('beam', beam_o), ('sample', samp_o)):
                beam.marks = [] if v == 'beam' else None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(model, o)
                end = torch.cuda.Event(enable_timing=True)
                end.record()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    total[(k, v)].append(dt)
                    if v == 'beam':
                        ev = beam.marks + [('backward', end)]
                        for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
                            parts[(k, name)].append(e0.elapsed_time(e1))
                beam.marks = None
            if i >= a.warmup:                  # the host assembly of the same tables (one device->host copy + Python bookkeeping)
                t = model._last_beam
                V1 = model.vocab_size + 1
                rows = torch.zeros(L, B * n, V1, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                beam.assemble_done_beams(argparse.Namespace(), t['parent'], t['token'], t['score'], t['ended'], rows, B, n, L, V1, n, n, {})
                torch.cuda.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e3)
    for k in built:
        print('%-7s beam-search SCST step  : %s' % (k, med(total[(k, 'beam')])))
        for ph in ('search', 'finalize', 'replay', 'backward'):
            print('%-7s   %-22s: %s' % (k, {'finalize': 'finalise + mask gather', 'replay': 'replay forward'}.get(ph, ph), med(parts[(k, ph)])))
        print('%-7s sampled SCST step      : %s' % (k, med(total[(k, 'sample')])))
        print('%-7s host assemble_done_beams: %s' % (k, med(host[k])), flush=True)


if __name__ == '__main__':
    main()
