#!/usr/bin/env python3
"""Generate ``tests/golden/aoa_variants.npz``: the REAL reference's AoAModel under the ablation switches of AoAModel.py:100-226,
eval mode (every dropout off), at the tiny size of tests/aoa_variants_ref64.SIZE.  Run only where the reference checkout exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_aoa_variants.py

Like make_ss.py it imports the reference's own modules unmodified and only stores weights, inputs and outputs.  Shared inputs:
fc / att / att_masks (one image masked down to 3 regions) / labels / masks.  Per variant (keys ``<tag>.<name>``, tags and
switches: aoa_variants_ref64.VARIANTS): the state-dict keys in order (``keys``), every weight (``P``: one flat array in key order, ``shapes``), the teacher-forced
log-probs and XE loss, the gradient of the masked XE loss with respect to every parameter (``grad``, packed like ``P``), the greedy decode and
the beam_size 2 decode (sequences, log-probs, the finished beams' scores).

The feed-forward tensors with a 2048 axis of a use_ff variant (w_1.weight, w_1.bias, w_2.weight: 2 x 2048 x 16 floats per layer,
six layers) do not fit a committed file: they are set from aoa_variants_ref64.ff_weight before anything is computed and only their shapes are stored; of their
gradients the file keeps ff_grad_digest (sums over every 32 consecutive hidden units, and every 32nd hidden unit as it is).

The script refuses a seed at which a greedy or beam decision is nearly tied: at every decode step of both decodes the two best
log-probs of every live row must be >= 1e-4 apart (for the beams: the three best, and the finished beams' scores), so a
float32 implementation takes the same decisions.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import REF                      # noqa: E402
from make_ss import save_npz                     # noqa: E402
import aoa_variants_ref64 as V                   # noqa: E402

SEED = 2024
GAP = 1e-4


def inputs():
    s = V.SIZE
    g = torch.Generator().manual_seed(SEED)
    B, K, n, T = s['B'], s['K'], s['n'], s['L'] + 2
    fc = torch.randn(B, s['F'], generator=g).clamp_min(0)
    att = torch.randn(B, K, s['F'], generator=g).clamp_min(0)
    am = torch.ones(B, K)
    am[1, 3:] = 0
    labels = torch.zeros(B, n, T, dtype=torch.long)
    masks = torch.zeros(B, n, T)
    for b in range(B):
        for j in range(n):
            ln = int(torch.randint(2, s['L'] + 1, (1,), generator=g))
            labels[b, j, 1:1 + ln] = torch.randint(1, s['V'] + 1, (ln,), generator=g)
            masks[b, j, :ln + 2] = 1
    labels[0, 0, 1:s['L'] + 1] = torch.randint(1, s['V'] + 1, (s['L'],), generator=g)      # one row of full length
    masks[0, 0, :] = 1
    return fc, att, am, labels, masks


def check_gaps(model, what, rows_live=None):
    """wrap the instance's get_logprobs_state: the k best log-probs of every row of every step must be GAP apart"""
    inner = model.get_logprobs_state
    worst = [1.0]

    def recording(it, *a, **kw):
        lp, st = inner(it, *a, **kw)
        top = lp.detach().topk(what, 1)[0]
        worst[0] = min(worst[0], float((top[:, :-1] - top[:, 1:]).min()))
        return lp, st
    model.get_logprobs_state = recording
    return worst, lambda: setattr(model, 'get_logprobs_state', inner)


def one_variant(models, losses, tag, fc, att, am, labels, masks):
    torch.manual_seed(SEED + ord(tag))
    opt = V.variant_opt(tag)
    model = models.setup(opt)
    with torch.no_grad():            # default inits leave some biases ~0: perturb everything so no term can hide
        for p in model.parameters():
            p.add_(0.1 * torch.randn_like(p))
        for k, p in model.named_parameters():
            if V.is_ff_weight(k):
                p.copy_(torch.from_numpy(V.ff_weight(tag, k, tuple(p.shape))))
    model.eval()
    sd = model.state_dict()
    keys = list(sd.keys())
    assert keys == [k for k, _ in model.named_parameters()]       # (the model has no buffers)
    small = [k for k in keys if not V.is_ff_weight(k)]
    big = [k for k in keys if V.is_ff_weight(k)]
    out = {'keys': np.array(keys), 'shapes': np.array([','.join(str(d) for d in sd[k].shape) for k in keys]),
           'P': V.pack([(k, sd[k].detach().numpy()) for k in small])}
    model.zero_grad()
    logp = model(fc, att, labels[..., :-1], am)
    loss = losses.LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    loss.backward()
    out['xe_logp'], out['xe_loss'] = logp.detach().numpy(), loss.detach().numpy()
    grads = {k: p.grad.detach().numpy() for k, p in model.named_parameters()}
    out['grad'] = V.pack([(k, grads[k]) for k in small])
    digests = {k: V.ff_grad_digest(grads[k]) for k in big}
    out['grad_sum32'], out['grad_sub'] = V.pack([(k, digests[k][0]) for k in big]), V.pack([(k, digests[k][1]) for k in big])
    with torch.no_grad():
        worst, undo = check_gaps(model, 2)
        seq, slp = model(fc, att, am, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')
        undo()
        assert worst[0] >= GAP, ('greedy decision nearly tied: choose another SEED', tag, worst[0])
        out['greedy_seq'], out['greedy_logp'] = seq.numpy(), slp.numpy()
        worst, undo = check_gaps(model, 3)
        seq, slp = model(fc, att, am, opt={'sample_method': 'beam_search', 'beam_size': 2, 'sample_n': 1}, mode='sample')
        undo()
        assert worst[0] >= GAP, ('beam decision nearly tied: choose another SEED', tag, worst[0])
        out['beam2_seq'], out['beam2_logp'] = seq.numpy(), slp.numpy()
        scores = np.array([[bm['p'] for bm in beams] for beams in model.done_beams], dtype=np.float64)
        assert scores.shape[1] < 2 or float(np.abs(np.diff(np.sort(scores, 1), axis=1)).min()) >= GAP, (tag, scores)
        out['beam2_p'] = scores
    print('%s: %d keys, loss %.6f, greedy %s' % (tag, len(sd), loss.item(), seq[0].tolist()))
    return {'%s.%s' % (tag, k): v for k, v in out.items()}


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models          # noqa: E402  (the reference)
    from captioning.modules import losses        # noqa: E402
    torch.set_num_threads(1)
    fc, att, am, labels, masks = inputs()
    out = dict(fc=fc.numpy(), att=att.numpy(), att_masks=am.numpy(), labels=labels.numpy(), masks=masks.numpy())
    for tag in V.VARIANTS:
        out.update(one_variant(models, losses, tag, fc, att, am, labels, masks))
    path = os.path.join(HERE, 'aoa_variants.npz')
    save_npz(path, out)
    print('aoa_variants.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()
