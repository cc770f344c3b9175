#!/usr/bin/env python3
"""The numbers of DESIGN.md's section on the truncation samplers (csrc/truncate.hip, capmi_truncate_rows).

us per call of each rule (minp0.1, eps0.0003, eta0.002, typ0.9) at `--rows` x `--v1` log-probability rows, on the register arm and
on the streaming arm (CAPMI_TRUNCATE_STREAM on the same rows), with the store row written as decode.sample_steps asks for it.
Beside them the yardstick for "a filter of this kind": capmi_select_logp with top_p = 0.9 on the same rows (the nucleus descent
plus the token choice, in-kernel Philox), and the floor: 2 * N * V1 * 4 bytes -- the row read once, q written once -- over the copy
rate this box reaches on a buffer of that size (torch's device-to-device copy of N * V1 floats, counted as read + write).
Device events around `--launches` back-to-back launches, `--rounds` rounds with the candidates alternating, mean per candidate.

    python scripts/truncate_bench.py [--rows 50,320] [--v1 9488] [--launches 40] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RULES = (('minp0.1', 0, 0.1), ('eps0.0003', 1, 3e-4), ('eta0.002', 2, 2e-3), ('typ0.9', 3, 0.9))


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches           # us per launch


def numbers(N, V1, a, dev):
    from imagecaptioning.pytorch_amd import _lib
    from imagecaptioning.pytorch_amd._lib import lib, check, stream_ptr
    x = torch.log_softmax(torch.randn(N, V1, device=dev, generator=torch.Generator(device=dev).manual_seed(N)) * 2.5, 1)
    q, store, copy = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    seq = torch.zeros(N, 1, dtype=torch.long, device=dev)
    it = torch.zeros(N, dtype=torch.long, device=dev)
    unf = torch.ones(N, dtype=torch.uint8, device=dev)
    kept = torch.zeros(N, dtype=torch.int32, device=dev)
    flt = _lib.SampleFilter(0, 0.9)
    st = stream_ptr()
    cands = {}
    for name, kind, param in RULES:
        for arm, flag in (('reg', 0), ('stream', _lib.TRUNCATE_STREAM)):
            cands['%s_%s' % (name, arm)] = (lambda kind=kind, param=param, flag=flag: check(lib.capmi_truncate_rows(
                x.data_ptr(), V1, q.data_ptr(), V1, N, V1, kind | flag, param, 1.0, kept.data_ptr(), None, store.data_ptr(), V1,
                unf.data_ptr(), st), 'capmi_truncate_rows'))
    cands['select_top_p0.9'] = lambda: check(lib.capmi_select_logp(
        x.data_ptr(), N, V1, 0, 1, 1, 1.0, None, 1234, seq.data_ptr(), 1, it.data_ptr(), unf.data_ptr(), None, None, 0, C.byref(flt), st),
        'capmi_select_logp')
    cands['select_plain'] = lambda: check(lib.capmi_select_logp(
        x.data_ptr(), N, V1, 0, 1, 1, 1.0, None, 1234, seq.data_ptr(), 1, it.data_ptr(), unf.data_ptr(), None, None, 0, None, st),
        'capmi_select_logp')
    cands['copy'] = lambda: copy.copy_(x)
    for fn in cands.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(a.rounds):
        for k, fn in cands.items():
            times[k].append(timed(fn, a.launches))
    out = {k: {'us': round(sum(ts) / len(ts), 2), 'us_rounds': [round(t, 2) for t in ts]} for k, ts in times.items()}
    nbytes = 2 * N * V1 * 4
    out['bytes'] = nbytes
    out['copy_GBps'] = round(nbytes / out['copy']['us'] * 1e-3, 1)
    out['floor_us'] = out['copy']['us']                   # the same 2 * N * V1 * 4 bytes at the rate the copy reached
    out['kept_typ0.9_mean'] = None
    check(lib.capmi_truncate_rows(x.data_ptr(), V1, q.data_ptr(), V1, N, V1, 3, 0.9, 1.0, kept.data_ptr(), None, None, 0, None, st),
          'capmi_truncate_rows')
    out['kept_typ0.9_mean'] = round(float(kept.float().mean()), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=str, default='50,320')
    ap.add_argument('--v1', type=int, default=9488)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device: a time taken elsewhere says nothing'
    dev = torch.device('cuda', 0)
    out = {'V1': a.v1, 'launches': a.launches, 'rounds': a.rounds}
    for N in [int(r) for r in a.rows.split(',')]:
        out['rows_%d' % N] = numbers(N, a.v1, a, dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
