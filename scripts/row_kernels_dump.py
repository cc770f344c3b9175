"""Every output of the vocabulary-row kernels (xe_loss, ppo, distill, ensemble, score) on seeded inputs, for a bit-for-bit
comparison of two builds of libcapmi:

    python scripts/row_kernels_dump.py OUT.pt          # needs a HIP device; run once per build
    python scripts/row_kernels_dump.py --compare A.pt B.pt

The shapes are small and sit where a row sweep (csrc/row_sweep.h) can go wrong: V1 below, at and above a float4 group, a row
long enough for two body trips per thread, every row-base phase 0..3, operand pairs that share their phase (float4 body) and
pairs that do not (scalar sweep), padded leading dimensions where ops takes one, more rows than a finish kernel has threads,
and masks with no, some and all rows off.  --compare wants exact equality, NaN positions included."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

V1S = (1, 3, 4, 5, 7, 8, 1031)
ROWS = ((1, 1), (2, 3), (50, 22))            # (N, T): N * T = 1, 6, 1100; N even for ppo's n = 2


def at(t, off):
    """a contiguous copy of t that starts `off` floats into a 16-byte aligned buffer"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def padded(t, pad, off=0):
    """a [rows, V1] view of leading dimension V1 + pad, `off` floats into its buffer"""
    rows, V1 = t.shape
    buf = torch.zeros(rows * (V1 + pad) + 8, dtype=t.dtype, device=t.device)
    v = buf[off:off + rows * (V1 + pad)].view(rows, V1 + pad)[:, :V1]
    v.copy_(t)
    return v


def masks(g, N, T, dev):
    m = (torch.rand(N, T, generator=g) < 0.7).float()
    m[:, 0] = 1.0
    some = m.clone()
    if N > 1:
        some[N - 1] = 0.0                    # a fully masked sample: 0 / 0 under per_row
    return {'all': torch.ones(N, T).to(dev), 'some': some.to(dev), 'none': torch.zeros(N, T).to(dev)}


def dump(dev='cuda'):
    from imagecaptioning.pytorch_amd import ops
    g = torch.Generator().manual_seed(1234)
    res = {}

    def put(name, *tensors):
        res[name] = [None if t is None else t.detach().cpu().clone() for t in tensors]

    def logp(N, T, V1):
        return torch.log_softmax(torch.randn(N, T, V1, generator=g) * 2.0, -1).to(dev)

    for V1 in V1S:
        for N, T in ROWS:
            if V1 == 1031 and N * T > 6:
                N, T = 4, 3
            tok = torch.randint(0, V1, (N, T), generator=g).to(dev)
            tok_out = tok.clone()
            tok_out[0, 0] = V1 + 2           # a token outside [0, V1)
            a, b = logp(N, T, V1), logp(N, T, V1)
            if V1 > 1:
                b[0, 0, 1] = float('-inf')   # a teacher / old row containing -inf
            for off in range(4):
                key = 'V%d.R%d.o%d' % (V1, N * T, off)
                x = at(a, off)
                for mname, m in masks(g, N, T, dev).items():
                    if off and mname != 'some':
                        continue
                    for per_row in (0, 1):
                        # xe
                        for sm in (0.0, 0.1):
                            if sm > 0 and V1 < 2:
                                continue
                            for tk, tkn in ((tok, 'in'), (tok_out, 'out')):
                                loss, msum, pos = ops.xe_loss_fwd(x, tk, m, smoothing=sm, per_row=bool(per_row))
                                gs, gq = ops.xe_loss_bwd(m, msum, T, V1, smoothing=sm, per_row=bool(per_row))
                                put('xe.%s.%s.p%d.s%g.%s' % (key, mname, per_row, sm, tkn), loss, msum, pos, gs, gq)
                        # distill: same phase (float4) and another phase (scalar), a padded teacher
                        for doff, dpad in ((off, 0), ((off + 1) % 4, 0), (off, 4), (off, 1)):
                            if (dpad and mname != 'some') or (doff != off and mname == 'none'):
                                continue
                            y = padded(b.view(N * T, V1), dpad, doff).unflatten(0, (N, T)) if dpad else at(b, doff)
                            for lam in (0.0, 0.5, 1.0):
                                for tk, tkn in ((tok, 'in'), (tok_out, 'out')):
                                    out, rows, stats, msum = ops.distill_loss_fwd(x, y, tk, m, lam, tau=2.0, per_row=bool(per_row))
                                    go = torch.full((N if per_row else 1,), 0.75, device=dev)
                                    gr = ops.distill_loss_bwd(x, y, tk, m, stats, msum, go, lam, tau=2.0, per_row=bool(per_row),
                                                              out=at(torch.zeros(N, T, V1, device=dev), off))
                                    put('kd.%s.%s.p%d.t%d+%d.l%g.%s' % (key, mname, per_row, doff, dpad, lam, tkn), out, rows, stats,
                                        msum, gr)
                if N % 2:
                    continue
                # ppo: the mask is the sequence's own (a 0 ends it); all on, some on, and all but column 0 off
                scores = torch.randn(N, generator=g).to(dev)
                for sname in ('all', 'some', 'none'):
                    if off and sname != 'some':
                        continue
                    seq = torch.randint(1, max(V1, 2), (N, T), generator=g).clamp_(max=V1 - 1 if V1 > 1 else 5)
                    if sname == 'some':
                        seq[:, T // 2] = 0
                    if sname == 'none':
                        seq[:] = 0
                    seq[0, 0] = V1 + 2
                    seq = seq.to(dev)
                    for ooff in (off, (off + 1) % 4):
                        y = at(b, ooff)
                        for per_row in (0, 1):
                            out, rows, stats, msum = ops.ppo_loss_fwd(x, y, seq, scores, 2, per_row=bool(per_row))
                            go = torch.full((N if per_row else 1,), 0.75, device=dev)
                            gr = ops.ppo_loss_bwd(y, seq, stats, msum, go, 2, per_row=bool(per_row),
                                                  out=at(torch.zeros(N, T, V1, device=dev), off))
                            put('ppo.%s.%s.p%d.old%d' % (key, sname, per_row, ooff), out, rows, stats, msum, gr)

    # ensemble: M = 2 and 4, members in one phase or not, padded leading dimensions, an output in another phase
    for V1 in V1S:
        for rows in (1, 6):
            xs = [torch.randn(rows, V1, generator=g).to(dev) * 3.0 for _ in range(4)]
            if V1 > 1:
                xs[1][0, 1] = float('-inf')
            for M in (2, 4):
                for off in range(4):
                    for moff, pad, ooff in ((off, 0, off), (off, 4, off), (off, 1, off), ((off + 1) % 4, 0, off),
                                            (off, 0, (off + 2) % 4)):
                        ins = [padded(xs[0], pad, off)] + [padded(x, pad, moff) for x in xs[1:M]]
                        out = padded(torch.zeros(rows, V1, device=dev), pad, ooff)
                        ops.ensemble_logprobs(ins, [1.0, 2.0, 0.5, 1.5][:M], out=out)
                        put('ens.V%d.R%d.M%d.o%d.m%d.p%d.out%d' % (V1, rows, M, off, moff, pad, ooff), out)

    # score: the wave / workgroup boundary at V1 = 1024 | 1025, and retrieval over the same widths
    for V1 in V1S + (1024, 1025):
        for rows in (1, 6):
            x = torch.randn(rows, V1, generator=g).to(dev) * 3.0
            if V1 > 1:
                x[0, 1] = float('-inf')
            tok = torch.randint(0, V1, (rows,), generator=g).to(dev)
            for off in range(4):
                for pad in (0, 1, 4):
                    lg = padded(x, pad, off)
                    live = torch.ones(rows, dtype=torch.uint8, device=dev)
                    live[rows // 2] = rows == 1
                    acc = torch.zeros(rows, device=dev)
                    cnt = torch.zeros(rows, dtype=torch.int32, device=dev)
                    tl = torch.zeros(rows, device=dev)
                    ops.score_step(lg, tok, live, acc, cnt, tl, inv_temperature=0.5, unk_col=V1 - 1)
                    rank, post = ops.retrieval_rank(lg, tok.cpu())
                    put('score.V%d.R%d.o%d.p%d' % (V1, rows, off, pad), live, acc, cnt, tl, rank, post)
    torch.cuda.synchronize()
    return res


def compare(pa, pb):
    A, B = torch.load(pa), torch.load(pb)
    bad, n = [], 0
    if set(A) != set(B):
        bad.append('result names differ: %s' % sorted(set(A) ^ set(B))[:5])
    def bits(t):                             # NaNs compare by position, everything else (infinities, signed zeros) by its bits
        return torch.where(t.isnan(), torch.zeros_like(t), t).view(torch.int32) if t.dtype == torch.float32 else t

    for k in sorted(set(A) & set(B)):
        if len(A[k]) != len(B[k]):
            bad.append('%s: %d against %d tensors' % (k, len(A[k]), len(B[k])))
            continue
        for i, (x, y) in enumerate(zip(A[k], B[k])):
            n += 1
            same = (x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and x.shape == y.shape
                                                and torch.equal(x.isnan(), y.isnan()) and torch.equal(bits(x), bits(y)))
            if not same:
                bad.append('%s[%d]' % (k, i))
    print('%d results, %d tensors compared, %d differ' % (len(A), n, len(bad)))
    for b in bad[:20]:
        print('  differs:', b)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = dump()
    torch.save(out, sys.argv[1])
    print('%d results, %d tensors -> %s' % (len(out), sum(len(v) for v in out.values()), sys.argv[1]))
