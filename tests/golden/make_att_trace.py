#!/usr/bin/env python3
"""Generate ``tests/golden/att_trace_tiny.npz``: the per-word region attention of the REAL reference's greedy decode, for
caption_model updown, att2in2, adaatt and adaattmo.  Run only where the reference checkout exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_att_trace.py

The reference returns no attention weights, so a forward hook on its ``core.attention.alpha_net`` records the scores of every
decoder step (one call per step: [rows * Kc, 1], Kc = the clipped region count, + 1 for AdaAtt's sentinel in front), and the few
lines of ``weights_of`` below restate what the reference does with them -- softmax, times the mask, renormalise (Attention.forward,
AttModel.py:741-745; AdaAtt_attention, :588-593, where the sentinel takes the mask of region 0) -- in float64.  Like the other
make_*.py it imports the reference's own modules unmodified and stores only weights, inputs and recorded results.

Sizes are the smallest at which the trace kernels can go wrong: B = 3 images with 5, 3 and 4 valid regions inside Kfull = 6 (so
the clipped K = 5 < Kfull and the masks bite), one batch without masks (K = Kfull), rows per image n = 1 and 2, L = 6 steps,
rnn / encoding / attention width 16 (AdaAtt needs them equal), vocabulary 12.  Per family and case (keys
``<family>.<case>.<name>``, cases ``n1``, ``n2``, ``nomask``): scores [S, N, Kc] float32 as hooked (S <= L: the reference stops once
every row has ended), seq [N, L], trace [N, L, Kout] float64 (caption-major, zero behind the clipped K, zero where
losses._shifted_mask is 0).

Asserted before anything is written, for the (seed, jitter) kept per family: in case n1 one caption ends at step 1 and one never
ends; on every kept (row, step) of every case the two largest weights differ by more than 1e-4 (``top`` is well defined); every
greedy decision has a gap of at least 1e-3 in log-prob to its runner-up (float32 rounding elsewhere cannot flip a token).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, tiny_opt, to_np      # noqa: E402
from make_ss import save_npz                       # noqa: E402

FAMILIES = ('updown', 'att2in2', 'adaatt', 'adaattmo')
B, KFULL, L, V = 3, 6, 6, 12
REGIONS = (5, 3, 4)
MIN_TOKEN_GAP, MIN_WEIGHT_GAP = 1e-3, 1e-4
SEARCH = [(seed, jit) for jit in (0.4, 0.3, 0.5, 0.6, 0.25) for seed in range(9100, 9200)]


class Reject(Exception):
    pass


def weights_of(scores, masks, sentinel):
    """float64 softmax over the last axis, times the mask, renormalised; masks [N, K] or None"""
    s = scores.astype(np.float64)
    e = np.exp(s - s.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    if masks is not None:
        m = masks.astype(np.float64)
        if sentinel:
            m = np.concatenate([m[:, :1], m], 1)
        w = w * m[None]
        w = w / w.sum(-1, keepdims=True)
    return w


def decode(model, fc, att, att_masks, n, sentinel):
    scores = []
    hook = model.core.attention.alpha_net.register_forward_hook(lambda mod, inp, out: scores.append(out.detach().clone()))
    try:
        with torch.no_grad():
            seq, slp = model(fc, att, att_masks, opt={'sample_method': 'greedy', 'beam_size': 1, 'sample_n': n}, mode='sample')
    finally:
        hook.remove()
    N = B * n
    # AttModel._sample runs the core once more after the last word (its loop covers seq_length + 1 steps, :283-288): that call
    # chooses nothing and is dropped
    scores = torch.stack([s.view(N, -1) for s in scores[:L]]).numpy()          # [S, N, Kc]
    K = KFULL if att_masks is None else int(att_masks.sum(1).max())
    assert scores.shape[2] == K + int(sentinel), scores.shape
    rows = None if att_masks is None else att_masks[:, :K].numpy().repeat(n, 0)
    w = weights_of(scores, rows, sentinel)
    S = w.shape[0]
    seq_np = seq.numpy()
    keep = np.concatenate([np.ones((N, 1), bool), seq_np[:, :-1] > 0], 1)
    trace = np.zeros((N, L, KFULL + int(sentinel)))
    trace[:, :S, :w.shape[2]] = w.transpose(1, 0, 2)
    trace *= keep[:, :, None]
    assert not keep[:, S:].any(), 'a kept step behind the steps the reference ran'
    # the conditions
    for r in range(N):
        for t in range(L):
            if keep[r, t]:
                top = torch.topk(slp[r, t], 2).values
                if float(top[0] - top[1]) < MIN_TOKEN_GAP:
                    raise Reject('token gap')
                two = np.sort(trace[r, t])[-2:]
                if two[1] - two[0] <= MIN_WEIGHT_GAP:
                    raise Reject('weight gap')
    return dict(scores=scores, seq=seq_np, trace=trace)


def one_family(models, name, seed, jitter):
    torch.manual_seed(seed)
    opt = tiny_opt(name, drop=0.0)
    opt.vocab_size, opt.seq_length, opt.max_length, opt.att_hid_size = V, L, L, 16
    opt.vocab = {str(i): 'w%d' % i for i in range(1, V + 1)}
    model = models.setup(opt)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(jitter * torch.randn_like(p))
        model.logit.bias[0] += 0.5
    model.eval()
    fc = torch.randn(B, opt.fc_feat_size).clamp_min(0)
    att = torch.randn(B, KFULL, opt.att_feat_size).clamp_min(0)
    att_masks = torch.zeros(B, KFULL)
    for b, k in enumerate(REGIONS):
        att_masks[b, :k] = 1
    boxes = (torch.rand(B, KFULL, 4) * 100).numpy().astype(np.float32)
    out = {('P.' + k): v for k, v in to_np(model.state_dict()).items()}
    out.update(fc=fc.numpy(), att=att.numpy(), att_masks=att_masks.numpy(), boxes=boxes, seed=np.array(seed), jitter=np.array(jitter))
    sentinel = name.startswith('adaatt')
    for case, masks, n in (('n1', att_masks, 1), ('n2', att_masks, 2), ('nomask', None, 1)):
        for k, v in decode(model, fc, att, masks, n, sentinel).items():
            out['%s.%s' % (case, k)] = v
    lens = (out['n1.seq'] > 0).sum(1)
    if not (lens == 1).any():
        raise Reject('no caption ends at step 1')
    if not (lens == L).any():
        raise Reject('no caption runs to the end')
    assert np.array_equal(out['n2.seq'][::2], out['n1.seq']) and np.array_equal(out['n2.seq'][1::2], out['n1.seq'])
    print('%-9s seed %d jitter %.2f: lengths %s / nomask %s, steps run %s' %
          (name, seed, jitter, lens.tolist(), (out['nomask.seq'] > 0).sum(1).tolist(),
           [out[c + '.scores'].shape[0] for c in ('n1', 'n2', 'nomask')]))
    return {'%s.%s' % (name, k): v for k, v in out.items()}


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models          # noqa: E402  (the reference)
    torch.set_num_threads(1)
    out = {}
    for name in FAMILIES:
        for seed, jitter in SEARCH:
            try:
                out.update(one_family(models, name, seed, jitter))
                break
            except Reject:
                pass
        else:
            raise SystemExit('no (seed, jitter) of the search order meets the fixture conditions for ' + name)
    path = os.path.join(HERE, 'att_trace_tiny.npz')
    save_npz(path, out)
    print('att_trace_tiny.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
