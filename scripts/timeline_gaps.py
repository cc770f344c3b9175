#!/usr/bin/env python3
"""What a launch leaves BEHIND itself, from a rocprofv3 --kernel-trace .db (timestamps, no --stats needed):
    python timeline_gaps.py file.db [nsteps] [title]
For every kernel name: the mean gap between its end and the start of the next launch, over the last `nsteps` complete training
steps (Adam to Adam), and the sum of those gaps per phase of the SCST step.  Phases: `rollout` ends with the last select launch
of the step, `bptt` runs from the first to the last LSTM-cell backward / dX launch, `tail` is everything else (prefill, reward,
time-batched gradients, Adam).  The loader / consumer GEMM serves two populations under one name: launches of >= 9 us are the
weight-streaming ones (gates, logits), the shorter ones the small decode GEMMs; they are listed apart."""
import sqlite3
import sys


def short(name, dur_us):
    n = name.replace('void ', '').replace('capmi_gemm::', '').replace('(anonymous namespace)::', '')
    n = n.split('(')[0][:48]
    if n.startswith('gemm_lc_kernel<true'):
        n += ' stream' if dur_us >= 9.0 else ' small'
    return n


def main():
    db = sqlite3.connect(sys.argv[1])
    nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    title = sys.argv[3] if len(sys.argv) > 3 else sys.argv[1]
    rows = db.execute('select start, end, name from kernels order by start').fetchall()
    adam = [i for i, r in enumerate(rows) if 'adam' in r[2]]
    if len(adam) <= nsteps:
        sys.exit('fewer than %d complete steps in the trace' % nsteps)
    per = {}                                    # name -> [n, gap sum, duration sum]
    phase = {'rollout': [0, 0.0, 0.0], 'bptt': [0, 0.0, 0.0], 'tail': [0, 0.0, 0.0]}
    span = 0.0
    for s in range(nsteps):
        lo, hi = adam[-nsteps - 1 + s] + 1, adam[-nsteps + s] + 1
        st = rows[lo:hi]
        span += (st[-1][1] - st[0][0]) / 1e3
        sel = [i for i, r in enumerate(st) if 'select' in r[2]]
        bw = [i for i, r in enumerate(st) if 'lstm_cell_bwd' in r[2] or 'gemm_lc_kernel<false' in r[2]]
        roll_end = sel[-1] if sel else -1
        b0, b1 = (bw[0], bw[-1]) if bw else (len(st), len(st))
        last_end = st[0][1]
        for i in range(len(st) - 1):
            last_end = max(last_end, st[i][1])
            gap = max(0.0, (st[i + 1][0] - last_end) / 1e3)
            dur = (st[i][1] - st[i][0]) / 1e3
            p = per.setdefault(short(st[i][2], dur), [0, 0.0, 0.0])
            p[0] += 1; p[1] += gap; p[2] += dur
            ph = phase['rollout' if i <= roll_end else 'bptt' if b0 <= i <= b1 else 'tail']
            ph[0] += 1; ph[1] += gap; ph[2] += dur
    print('# %s\n' % title)
    print('last %d steps (Adam to Adam), %.1f us per step from first kernel start to last kernel end\n' % (nsteps, span / nsteps))
    print('| phase | launches/step | kernel us/step | gap us/step | mean gap us |\n|---|---|---|---|---|')
    for k in ('rollout', 'bptt', 'tail'):
        n, g, d = phase[k]
        print('| %s | %.1f | %.0f | %.1f | %.2f |' % (k, n / nsteps, d / nsteps, g / nsteps, g / max(n, 1)))
    print('\n| kernel (gap BEHIND it) | launches/step | mean us | mean gap us | gap us/step |\n|---|---|---|---|---|')
    for k, (n, g, d) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        if n / nsteps >= 1:
            print('| `%s` | %.1f | %.2f | %.2f | %.1f |' % (k, n / nsteps, d / n, g / n, g / nsteps))


if __name__ == '__main__':
    main()
