"""Child process of tests/test_xe_loss_gpu.py: one XE step of a tiny model, loss and parameter gradients written to an .npz.
    python xe_step_child.py <family> <out.npz>          (CAPMI_FUSED_XE in the environment selects the criterion's route)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXTRA = {'updown': {}, 'newfc': {},
         'transformer': dict(N_enc=1, N_dec=1, d_model=16, d_ff=32, num_att_heads=2, dropout=0.0)}


def main(family, out):
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    kw = dict(caption_model=family, input_encoding_size=16, rnn_size=16, att_hid_size=8, seq_length=5, max_length=5, vocab_size=20,
              fc_feat_size=12, att_feat_size=12, vocab={str(i): 'w%d' % i for i in range(1, 21)}, drop_prob_lm=0.0)
    kw.update(EXTRA[family])
    torch.manual_seed(7)
    model = models.setup(synthetic.updown_opt(**kw)).cuda()
    model.train()
    g = torch.Generator().manual_seed(11)
    B, n, K, L = 2, 2, 3, 5
    fc = torch.randn(B, 12, generator=g).cuda()
    att = torch.randn(B, K, 12, generator=g).cuda()
    labels = torch.zeros(B, n, L + 2, dtype=torch.int64)
    masks = torch.zeros(B, n, L + 2)
    for b in range(B):
        for j in range(n):
            ln = 2 + (b * n + j) % 4
            labels[b, j, 1:1 + ln] = torch.randint(1, 21, (ln,), generator=g)
            masks[b, j, :ln + 2] = 1
    labels, masks = labels.cuda(), masks.cuda()
    calls = {'select': 0, 'sum': 0}
    for name, key in (('select_logp', 'select'), ('sum_logp', 'sum')):
        def wrap(orig, key):
            def f(*a, **k):
                calls[key] += 1
                return orig(*a, **k)
            return f
        setattr(losses, name, wrap(getattr(losses, name), key))
    res = {}
    for tag, crit in (('lm', losses.LanguageModelCriterion()), ('ls', losses.LabelSmoothing(smoothing=0.1))):
        model.zero_grad()
        logp = model(fc, att, labels[..., :-1], None)
        loss = crit(logp, labels[..., 1:], masks[..., 1:])
        loss.backward()
        res[tag + '.loss'] = loss.detach().cpu().numpy()
        res[tag + '.positions'] = np.int64(logp.shape[0] * logp.shape[1])
        for k, p in model.named_parameters():
            if p.grad is not None:
                res[tag + '.g.' + k] = p.grad.detach().cpu().numpy()
    res['select_calls'], res['sum_calls'] = np.int64(calls['select']), np.int64(calls['sum'])
    np.savez(out, **res)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
