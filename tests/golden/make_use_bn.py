#!/usr/bin/env python3
"""Generate ``tests/golden/use_bn_tiny_<family>_bn<use_bn>.npz``: the REAL reference's UpDown and Att2in2 models with ``use_bn`` 1 and 2 (BatchNorm1d
around att_embed, AttModel.py:80-85) at a tiny size, run on CPU with fixed seeds.  Run only where the reference checkout exists
(never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_use_bn.py

Like make_att2in2.py it imports the reference's own modules unmodified and only stores arrays.  Per configuration: perturbed parameters (gamma / beta too), ragged att_masks (the reference needs them with use_bn);
three train-mode XE steps at drop_prob_lm 0 on three scalings of the features (log-probs, loss, every gradient, the running buffers
after each step); eval-mode XE, greedy and beam 3 on the resulting running buffers; one train-mode step at drop_prob_lm 0.5 with
the recorded keep masks, att_embed's re-ordered from the packed order to [B, K, R].  Every float quantity k is stored as ``k@64``
(the reference in .double() on the same inputs and masks) and ``k@d`` (max |float32 reference - k@64|); token arrays as ``k``.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, DropRecorder, tiny_opt, to_np      # noqa: E402

B, n, K, T = 3, 2, 6, 9


class ReplayDrop(DropRecorder):
    """the keep masks of an earlier DropRecorder, call by call (the float64 run sees the float32 run's masks)"""

    def __init__(self, calls):
        self.calls, self.i = calls, 0

    def __call__(self, input, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return input
        p_, keep = self.calls[self.i]
        self.i += 1
        assert p_ == float(p) and keep.shape == tuple(input.shape)
        return input * (torch.from_numpy(keep).to(input.dtype) / (1.0 - p))


def buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if 'running_' in k or 'num_batches' in k}


def run(model, dt, fc, att_steps, labels, masks, att_masks, losses, drops=None):
    """the whole protocol on one model in dtype dt -> (dict of arrays, the dropout record)"""
    out = {}
    crit = losses.LanguageModelCriterion()
    fc, att_steps, masks = fc.to(dt), [a.to(dt) for a in att_steps], masks.to(dt)

    def xe(tag, att, att_m):
        model.zero_grad()
        logp = model(fc, att, labels[..., :-1], att_m)
        loss = crit(logp, labels[..., 1:], masks[..., 1:])
        loss.backward()
        out[tag + '_logp'], out[tag + '_loss'] = logp.detach().numpy(), loss.detach().numpy()
        for k, p in model.named_parameters():
            out[tag + '_grad.' + k] = p.grad.detach().numpy().copy()

    model.train()
    for s, att in enumerate(att_steps):
        xe('train%d' % s, att, att_masks)
        for k, v in buffers(model).items():
            out['train%d_buf.%s' % (s, k)] = v.numpy()
    model.eval()
    xe('eval', att_steps[0], att_masks)
    with torch.no_grad():
        seq, slp = model(fc, att_steps[0], att_masks, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')
        out['greedy_seq'], out['greedy_logp'] = seq.numpy(), slp.numpy()
        seq, slp = model(fc, att_steps[0], att_masks, opt={'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1}, mode='sample')
        out['beam3_seq'], out['beam3_logp'] = seq.numpy(), slp.numpy()
    for k, v in buffers(model).items():          # eval updates nothing
        assert np.array_equal(v.numpy(), out['train2_buf.' + k]), k
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.5
    model.drop_prob_lm = 0.5
    if hasattr(model, 'core') and hasattr(model.core, 'drop_prob_lm'):
        model.core.drop_prob_lm = 0.5
    model.train()
    with (DropRecorder(3000) if drops is None else ReplayDrop(drops)) as rec:
        xe('drop', att_steps[1], att_masks)
    for k, v in buffers(model).items():
        out['drop_buf.' + k] = v.numpy()
    return out, rec.calls


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models          # noqa: E402  (the reference)
    RA = sys.modules['captioning.models.AttModel']      # (the package re-exports the class under the module's name)
    from captioning.modules import losses        # noqa: E402
    from torch.nn.utils.rnn import PackedSequence

    N = B * n
    out = {}
    for fam in ('updown', 'att2in2'):
        for use_bn in (1, 2):
            torch.manual_seed(8000 + 10 * use_bn + len(fam))
            opt = tiny_opt(fam, drop=0.0)
            opt.use_bn = use_bn
            model = models.setup(opt)
            with torch.no_grad():            # perturb everything (gamma and beta included) so no term can hide
                for p in model.parameters():
                    p.add_(0.4 * torch.randn_like(p))
                model.logit.bias[0] += 0.5
            fc = torch.randn(B, opt.fc_feat_size).clamp_min(0)
            att = torch.randn(B, K, opt.att_feat_size).clamp_min(0)
            att[:, :, 3] = 0.0                   # a column that is exactly zero (post-ReLU features have them)
            att[:, :, 5] = 3.0 + 0.01 * torch.randn(B, K)        # mean >> std
            att_steps = [att, 1.5 * att + 0.1, 0.5 * att]
            labels = torch.zeros(B, n, T + 1, dtype=torch.long)
            for b in range(B):
                for j in range(n):
                    ln = int(torch.randint(3, T - 1, (1,)))
                    labels[b, j, 1:1 + ln] = torch.randint(1, opt.vocab_size + 1, (ln,))
            labels[:, :, T - 1:] = 0
            masks = torch.zeros(B, n, T + 1)
            for b in range(B):
                for j in range(n):
                    masks[b, j, :int((labels[b, j] > 0).sum()) + 2] = 1
            att_masks = torch.ones(B, K)         # ragged; row 1 is full, so clip_att keeps K
            att_masks[0, 4:] = 0
            att_masks[2, 5:] = 0

            pre = '%s.bn%d.' % (fam, use_bn)
            for k, v in to_np(model.state_dict()).items():
                out[pre + 'P.' + k] = v.copy()          # (a copy: the buffers are updated in place below)
            out[pre + 'keys'] = np.array(list(model.state_dict().keys()))
            out.update({pre + 'fc': fc.numpy(), pre + 'labels': labels.numpy(), pre + 'masks': masks.numpy(),
                        pre + 'att_masks': att_masks.numpy()})
            for s, a in enumerate(att_steps):
                out[pre + 'att%d' % s] = a.numpy()
            m64 = copy.deepcopy(model).double()
            o32, calls = run(model, torch.float32, fc, att_steps, labels, masks, att_masks, losses)
            o64, _ = run(m64, torch.float64, fc, att_steps, labels, masks, att_masks, losses, drops=calls)
            for k, v in o32.items():
                if v.dtype.kind == 'f':              # (the float32 arrays themselves are not kept: the committed files stay under 1 MiB)
                    out[pre + k + '@64'] = o64[k]
                    out[pre + k + '@d'] = np.float64(np.abs(v.astype(np.float64) - o64[k]).max())
                else:
                    out[pre + k] = v
                    assert np.array_equal(v, o64[k]), k
            # the dropout record in call order: (fc_embed [B,R] -- UpDown only,) att_embed on the PACKED rows (sorted by length,
            # time-major), then per step embed [N,E] and the core output [N,R]
            i = 0
            if fam == 'updown':
                out[pre + 'drop.fc'] = calls[0][1]
                i = 1
            lengths = att_masks.long().sum(1)
            packed, inv_ix = RA.sort_pack_padded_sequence(att_steps[1], lengths)
            keep = torch.from_numpy(calls[i][1])
            assert keep.shape[0] == int(lengths.sum())
            full = RA.pad_unsort_packed_sequence(PackedSequence(keep, packed[1]), inv_ix)          # [B, K, R], padded rows False
            out[pre + 'drop.att'] = full.numpy()
            steps = (len(calls) - i - 1) // 2
            assert len(calls) == i + 1 + 2 * steps
            out[pre + 'drop.xt'] = np.stack([calls[i + 1 + 2 * t][1] for t in range(steps)])
            out[pre + 'drop.out'] = np.stack([calls[i + 2 + 2 * t][1] for t in range(steps)])
            assert out[pre + 'drop.xt'].shape[1] == N

    for fam in ('updown', 'att2in2'):            # one file per configuration: each stays well under 1 MiB
        for use_bn in (1, 2):
            pre = '%s.bn%d.' % (fam, use_bn)
            part = {k[len(pre):]: v for k, v in out.items() if k.startswith(pre)}
            name = 'use_bn_tiny_%s_bn%d.npz' % (fam, use_bn)
            path = os.path.join(HERE, name)
            np.savez_compressed(path, **part)
            print(name, len(part), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
