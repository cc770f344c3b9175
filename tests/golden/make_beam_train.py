#!/usr/bin/env python3
"""Generate ``tests/golden/beam_train_tiny.npz``: the REAL reference's beam search called in train() mode with gradients
(ADVANCED.md "SCST in Topdown Bottomup paper": train_sample_method greedy, train_beam_size > 1) for UpDownModel and
NewFCModel at a tiny size, on CPU with fixed seeds.  Run only where the reference checkout exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_beam_train.py

Like make_att2in2.py it imports the reference's own modules unmodified and stores data only.  Per family: perturbed weights,
inputs (ragged att_masks for updown), logit.bias[0] raised so that some beams end early and some run to seq_length; beam 3;
four runs that cover sample_n 3 / 1, length_penalty '' / 'wu_0.5' and drop_prob_lm 0 / 0.5 (every dropout call recorded by
make_golden.DropRecorder): seq, dense seqLogprobs, a fixed random reward, the RewardCriterion loss, every parameter gradient.

A search is only a fair fixture if fp32 reordering cannot flip it: for every run the fp64 replay (tests/beam_train_ref64.py,
which must return the reference's seq exactly) measures the gap between the last kept and the first dropped candidate at
every step and image and between neighbouring final p; the seed is advanced until the smallest gap of all runs is >= 1e-3.
The smallest gap is printed and stored as ``min_gap``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: beam_train_ref64
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # repository root: oracle
from make_golden import REF, DropRecorder, tiny_opt, to_np      # noqa: E402

RUNS = (('a3', 0.0, 3, ''), ('a1', 0.0, 1, 'wu_0.5'), ('b3', 0.5, 3, 'wu_0.5'), ('b1', 0.5, 1, ''))
BEAM, B, K = 3, 3, 6
MIN_GAP = 1e-3


def build(models, losses, family, seed):
    import beam_train_ref64 as ref
    torch.manual_seed(seed)
    opt = tiny_opt(family, drop=0.0)
    L = opt.seq_length
    model = models.setup(opt)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.4 * torch.randn_like(p))
        model.logit.bias[0] += 1.0       # some beams end early, some run to seq_length
    fc = torch.randn(B, opt.fc_feat_size).clamp_min(0)
    att = torch.randn(B, K, opt.att_feat_size).clamp_min(0)
    att_masks = None
    if family == 'updown':
        att_masks = torch.ones(B, K)
        att_masks[0, 4:] = 0
        att_masks[2, 5:] = 0
    P = to_np(model.state_dict())
    out = {('P.' + k): v for k, v in P.items()}
    out.update(fc=fc.numpy(), att=att.numpy())
    if att_masks is not None:
        out['att_masks'] = att_masks.numpy()
    gap = float('inf')
    lengths = []
    for tag, drop, sample_n, pen in RUNS:
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = drop
        if hasattr(model, 'core') and hasattr(model.core, 'drop_prob_lm'):
            model.core.drop_prob_lm = drop
        model.drop_prob_lm = drop
        model.train()
        model.zero_grad()
        o = {'sample_method': 'greedy', 'beam_size': BEAM, 'sample_n': sample_n, 'length_penalty': pen}
        with DropRecorder(7000 + seed) as rec:
            seq, slp = model(fc, att, att_masks, opt=o, mode='sample')
        assert slp.requires_grad
        rows = B * sample_n
        reward = torch.from_numpy(np.random.RandomState(11).randn(rows, 1).astype(np.float32)).repeat(1, L)
        loss = losses.RewardCriterion()(slp, seq.data, reward)
        loss.backward()
        rec.dump(out, tag)
        out[tag + '.seq'], out[tag + '.logp'] = seq.numpy(), slp.detach().numpy()
        out[tag + '.reward'], out[tag + '.loss'] = reward.numpy(), loss.detach().numpy()
        out[tag + '.opt'] = np.array([drop, sample_n], np.float64)
        out[tag + '.length_penalty'] = np.array(pen)
        for k, p in model.named_parameters():
            out['%s.grad.%s' % (tag, k)] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
        # the gap of this search, measured by the fp64 replay, which must reproduce the reference's beams
        masks = ref.recorded_masks(out, tag, family, B, BEAM, L, att_masks) if drop > 0 else None
        r = ref.run(family, {k: torch.from_numpy(v) for k, v in P.items()}, fc, att, att_masks, BEAM, sample_n, L, pen, masks)
        if not np.array_equal(r['seq'], seq.numpy()):
            return None, 0.0, []
        gap = min(gap, r['gap'], r['p_gap'])
        lengths += r['length'].tolist()
    out['min_gap'] = np.array(gap)
    return out, gap, lengths


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models          # noqa: E402  (the reference)
    from captioning.modules import losses        # noqa: E402
    L = tiny_opt('updown').seq_length
    allout = {}
    for family in ('updown', 'newfc'):
        seed = 100
        while True:
            out, gap, lengths = build(models, losses, family, seed)
            ok = out is not None and gap >= MIN_GAP and min(lengths) < L and max(lengths) == L
            print('%s seed %d: smallest gap %.3e, beam lengths %s%s' % (family, seed, gap, sorted(set(lengths)), '' if ok else '  -> reseed'))
            if ok:
                break
            seed += 1
            assert seed < 400
        allout.update({family + '.' + k: v for k, v in out.items()})
        allout[family + '.seed'] = np.array(seed)
    path = os.path.join(HERE, 'beam_train_tiny.npz')
    np.savez_compressed(path, **allout)
    print('beam_train_tiny.npz:', len(allout), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
