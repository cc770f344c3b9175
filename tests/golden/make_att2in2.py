#!/usr/bin/env python3
"""Generate ``tests/golden/att2in2_tiny.npz``: the REAL reference's Att2in2Model (caption_model att2in2, configs/a2i2*.yml)
at a tiny size, run on CPU with fixed seeds.  Run only where the reference checkout exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_att2in2.py

Like make_golden.py it imports the reference's own modules unmodified and only stores weights, inputs and outputs:
eval-mode XE log-probs / loss / gradients (ragged att_masks), greedy and beam-3 decodes, a train-mode XE pass at
drop_prob_lm 0.5 with every dropout call recorded (make_golden.DropRecorder), and a RewardCriterion gradient over a fixed
(greedy, sample_n 2) sequence with fixed rewards.  tests/test_att2in2_host.py replays it through tests/att2in2_ref64.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, DropRecorder, tiny_opt, to_np      # noqa: E402


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models          # noqa: E402  (the reference)
    from captioning.modules import losses        # noqa: E402

    torch.manual_seed(4321)
    B, n, K, T = 3, 2, 6, 9          # T = seq_length + 1 inputs
    N = B * n
    opt = tiny_opt('att2in2', drop=0.0)
    model = models.setup(opt)
    with torch.no_grad():            # default inits leave some biases ~0: perturb everything so no term can hide
        for p in model.parameters():
            p.add_(0.4 * torch.randn_like(p))
        model.logit.bias[0] += 0.5   # EOS after a few words for some rows, not at once
    fc = torch.randn(B, opt.fc_feat_size).clamp_min(0)
    att = torch.randn(B, K, opt.att_feat_size).clamp_min(0)
    labels = torch.zeros(B, n, T + 1, dtype=torch.long)
    for b in range(B):
        for j in range(n):
            ln = int(torch.randint(3, T - 1, (1,)))
            labels[b, j, 1:1 + ln] = torch.randint(1, opt.vocab_size + 1, (ln,))
    labels[:, :, T - 1:] = 0         # the trailing all-pad-column break (AttModel.py:158) triggers
    masks = torch.zeros(B, n, T + 1)
    for b in range(B):
        for j in range(n):
            masks[b, j, :int((labels[b, j] > 0).sum()) + 2] = 1
    att_masks = torch.ones(B, K)
    att_masks[0, 4:] = 0
    att_masks[2, 5:] = 0

    out = {('P.' + k): v for k, v in to_np(model.state_dict()).items()}
    out.update(fc=fc.numpy(), att=att.numpy(), labels=labels.numpy(), masks=masks.numpy(), att_masks=att_masks.numpy())
    crit = losses.LanguageModelCriterion()

    model.eval()
    model.zero_grad()
    logp = model(fc, att, labels[..., :-1], att_masks)
    loss = crit(logp, labels[..., 1:], masks[..., 1:])
    loss.backward()
    out['xe_logp'], out['xe_loss'] = logp.detach().numpy(), loss.detach().numpy()
    for k, p in model.named_parameters():
        out['xe_grad.' + k] = p.grad.detach().numpy().copy()

    with torch.no_grad():
        seq, slp = model(fc, att, att_masks, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')
        out['greedy_seq'], out['greedy_logp'] = seq.numpy(), slp.numpy()
        seq, slp = model(fc, att, att_masks, opt={'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1}, mode='sample')
        out['beam3_seq'], out['beam3_logp'] = seq.numpy(), slp.numpy()

    # RewardCriterion over a fixed sequence: the greedy decode with sample_n 2 (deterministic), fixed rewards
    model.zero_grad()
    seq, slp = model(fc, att, att_masks, opt={'sample_method': 'greedy', 'beam_size': 1, 'sample_n': n}, mode='sample')
    reward = torch.from_numpy(np.random.RandomState(5).randn(N, 1).astype(np.float32)).repeat(1, seq.shape[1])
    rl = losses.RewardCriterion()(slp, seq.data, reward)
    rl.backward()
    out['rl_seq'], out['rl_logp'], out['rl_reward'], out['rl_loss'] = seq.numpy(), slp.detach().numpy(), reward.numpy(), rl.detach().numpy()
    for k, p in model.named_parameters():
        out['rl_grad.' + k] = p.grad.detach().numpy().copy()

    # train mode, drop_prob_lm 0.5 at the three sites (att_embed, embed, core output), no att_masks
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.5
    model.train()
    model.zero_grad()
    with DropRecorder(3000) as rec:
        logp = model(fc, att, labels[..., :-1], None)
    loss = crit(logp, labels[..., 1:], masks[..., 1:])
    loss.backward()
    rec.dump(out, 'train')
    out['train_logp'], out['train_loss'] = logp.detach().numpy(), loss.detach().numpy()
    for k, p in model.named_parameters():
        out['train_grad.' + k] = p.grad.detach().numpy().copy()

    path = os.path.join(HERE, 'att2in2_tiny.npz')
    np.savez_compressed(path, **out)
    print('att2in2_tiny.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
