#!/usr/bin/env python3
"""Generate ``tests/golden/ppo_tiny.npz``: the REAL reference's PPOLoss (captioning/modules/losses.py:267-357) in float64, run on
CPU over two old models.  Run only where the reference checkout exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ppo.py

The old models are make_golden.family_model('updown') and family_model('transformer') -- the weights P.* of updown_tiny.npz and
transformer_tiny.npz, converted to float64; they are not stored again (the Transformer's alone would exceed the fixture's size
budget).  Each one's state_dict is written to a temporary ``ppo_old_model_path`` that the reference constructor loads.  The inputs
are updown_tiny.npz's (fc, att, ragged att_masks) with n = 3 samples per image.  ``get_scores`` is replaced by fixed scores.

Per family <f> (key prefix):
    <f>_seq [N, L]          ragged: EOS at step 0, no EOS at all, EOS in the middle, ...
    <f>_scores [N]          image 1's three samples score the same (advantage 0)
    <f>_old_logp [N, L, V1] the old model's teacher-forced log-probs of [0, seq[:, :-1]] (its rows after the early stop are zeros)
    <f>_input [N, L, V1]    log_softmax(old log-probs + noise): ratios on both sides of the clip range
and per case <f>_<tag>_<reduction> with tag e2k2 = (eps 0.2, kl_coef 0.02, the defaults) or e05k50 = (0.05, 0.5):
    _loss, _pg_loss, _kl_loss, _clipfrac, _reward, _grad (d loss / d input; for 'none' of sum_i u_i loss_i with u = <f>_u)
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, family_model, warnings_off      # noqa: E402

FAMILIES = ('updown', 'transformer')
CASES = (('e2k2', 0.2, 0.02), ('e05k50', 0.05, 0.5))
N_PER = 3


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models            # noqa: E402  (the reference)
    import captioning.modules.losses as RL
    u = np.load(os.path.join(HERE, 'updown_tiny.npz'))
    fc, att, am = (torch.from_numpy(u[k]).double() for k in ('fc', 'att', 'att_masks'))
    B, n = fc.shape[0], N_PER
    N = B * n
    out = {'fc': fc.numpy(), 'att': att.numpy(), 'att_masks': am.numpy(), 'n': np.int64(n)}
    g = torch.Generator().manual_seed(2718)
    for fi, fam in enumerate(FAMILIES):
        model = family_model(models, fam).double()
        L, V = 8, model.vocab_size
        seq = torch.randint(1, V + 1, (N, L), generator=g)
        for r, ln in enumerate([0, 8, 4, 2, 8, 6, 1, 5, 3]):              # ragged: EOS at step 0, none at all, in the middle
            seq[r, ln:] = 0
        scores = torch.rand(N, generator=g, dtype=torch.float64)
        scores[3:6] = scores[3]                                          # image 1: every sample scores the same
        scores = scores.numpy()
        RL.get_scores = lambda data_gts, gen_result, opt, s=scores: s.copy()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'old.pth')
            torch.save(model.state_dict(), path)
            for tag, eps, klc in CASES:
                for red in ('mean', 'none'):
                    opt = argparse.Namespace(use_ppo=1, ppo_old_model_path=path, ppo_cliprange=eps, ppo_kl_coef=klc,
                                             train_sample_n=n)
                    with contextlib.redirect_stdout(io.StringIO()), warnings_off():
                        crit = RL.PPOLoss(opt, model)
                    if fam + '_input' not in out:
                        mis = torch.cat([seq.new_zeros(N, 1), seq[:, :-1]], 1)
                        with torch.no_grad():
                            lo = crit.old_model(fc, att, mis, am)
                        noise = 0.35 * torch.randn(lo.shape, generator=g, dtype=torch.float64)
                        x0 = torch.log_softmax(lo + noise, 2)
                        out[fam + '_seq'] = seq.numpy()
                        out[fam + '_scores'] = scores
                        out[fam + '_old_logp'] = lo.numpy()
                        out[fam + '_input'] = x0.numpy()
                        out[fam + '_u'] = np.linspace(0.5, 1.5, N)
                    x = torch.from_numpy(out[fam + '_input']).clone().requires_grad_(True)
                    with contextlib.redirect_stdout(io.StringIO()), warnings_off():
                        o = crit(x, seq, [None] * B, fc, att, am, reduction=red)
                    loss = o['loss']
                    (loss if red == 'mean' else (loss * torch.from_numpy(out[fam + '_u'])).sum()).backward()
                    key = '%s_%s_%s' % (fam, tag, red)
                    for k in ('loss', 'pg_loss', 'kl_loss', 'clipfrac', 'reward'):
                        out[key + '_' + k] = o[k].detach().numpy()
                    out[key + '_grad'] = x.grad.numpy()
                    print(key, 'loss', o['loss'].detach().numpy().round(5), 'clipfrac', float(o['clipfrac']))
    np.savez_compressed(os.path.join(HERE, 'ppo_tiny.npz'), **out)
    print('wrote ppo_tiny.npz with', len(out), 'arrays,', os.path.getsize(os.path.join(HERE, 'ppo_tiny.npz')), 'bytes')


if __name__ == '__main__':
    main()
