#!/usr/bin/env python3
"""Generate ``tests/golden/ss_tiny.npz``: scheduled sampling (AttModel._forward with ss_prob > 0, AttModel.py:144-162) of the
REAL reference for the three families that inherit it unchanged and run it in their own rollouts here -- newfc, aoa, att2in2 --
at make_golden.tiny_opt size.  Run only where the reference checkout exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ss.py

Like make_att2in2.py it imports the reference's own modules unmodified and only stores weights, inputs and outputs.  Per family
(keys ``<family>.<name>``): the state dict (``P.*``), fc / att / labels / masks / att_masks, the token really fed at every step
(``fed`` [T_eff, N], recorded by wrapping the instance's get_logprobs_state), the returned log-probs, the LanguageModelCriterion
loss and every parameter gradient.  Train mode with EVERY dropout probability 0 (the hard-coded 0.1 rates of AoAModel.py:18,119
included: the p of the nn.Dropout instances is set, the source is not edited), ss_prob 0.6, ragged labels with a trailing all-pad
column (the break at :158), ragged att_masks.

A test reproduces the reference's inputs without sharing its RNG: coin = "fed token differs from the label" (a draw that happens
to equal the label is the same input), noise = a large constant at the fed token.  tests/test_ss_host.py replays the file through
tests/ss_ref64.py and tests/att2in2_ref64.py, tests/test_ss_gpu.py through the HIP rollouts.

The archive is written with fixed zip timestamps, so the same machine regenerates it byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, tiny_opt, to_np      # noqa: E402

SS_PROB = 0.6
FAMILIES = (('newfc', 101, 0.3), ('aoa', 102, 0.15), ('att2in2', 103, 0.4))     # (name, seed, weight perturbation)


def family_opt(name):
    opt = tiny_opt(name, drop=0.0)
    if name == 'aoa':            # the configs/aoa.yml switches, as make_golden.main_aoa
        opt.refine, opt.refine_aoa, opt.use_ff, opt.decoder_type, opt.use_multi_head = 1, 1, 0, 'AoA', 2
        opt.num_heads, opt.multi_head_scale, opt.mean_feats, opt.ctx_drop, opt.dropout_aoa = 2, 1, 1, 1, 0.0
        opt.num_layers = 2
    return opt


def save_npz(path, arrays):
    """np.savez_compressed with constant member timestamps (numpy stamps the current time)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def one_family(models, losses, name, seed, jitter):
    torch.manual_seed(seed)
    B, n, K, T = 3, 2, 6, 9          # T = seq_length + 1 inputs
    N = B * n
    opt = family_opt(name)
    model = models.setup(opt)
    with torch.no_grad():            # default inits leave some biases ~0: perturb everything so no term can hide
        for p in model.parameters():
            p.add_(jitter * torch.randn_like(p))
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    fc = torch.randn(B, opt.fc_feat_size).clamp_min(0)
    att = torch.randn(B, K, opt.att_feat_size).clamp_min(0)
    labels = torch.zeros(B, n, T + 1, dtype=torch.long)
    for b in range(B):
        for j in range(n):
            ln = int(torch.randint(3, T - 1, (1,)))
            labels[b, j, 1:1 + ln] = torch.randint(1, opt.vocab_size + 1, (ln,))
    labels[0, 0, 1:T - 1] = torch.randint(1, opt.vocab_size + 1, (T - 2,))     # one row reaches the last column before the pad
    labels[:, :, T - 1:] = 0         # the trailing all-pad-column break (AttModel.py:158) triggers
    masks = torch.zeros(B, n, T + 1)
    for b in range(B):
        for j in range(n):
            masks[b, j, :int((labels[b, j] > 0).sum()) + 2] = 1
    att_masks = torch.ones(B, K)
    att_masks[0, 4:] = 0
    att_masks[2, 5:] = 0

    fed = []
    inner = model.get_logprobs_state

    def recording(it, *a, **kw):
        fed.append(it.detach().clone())
        return inner(it, *a, **kw)
    model.get_logprobs_state = recording        # an instance attribute: AttModel._forward calls self.get_logprobs_state

    model.train()
    model.ss_prob = SS_PROB
    model.zero_grad()
    torch.manual_seed(seed + 1000)
    logp = model(fc, att, labels[..., :-1], att_masks)
    loss = losses.LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:])
    loss.backward()
    fed = torch.stack(fed)                        # [T_eff, N]
    seq = labels[..., :-1].reshape(N, -1)
    T_eff = fed.shape[0]
    assert T_eff == T - 1, T_eff                  # the break fired one column early
    assert torch.equal(fed[0], seq[:, 0])
    n_draw = int((fed != seq[:, :T_eff].t()).sum())
    assert n_draw > (T_eff - 1) * N // 3, n_draw  # most positions after the first are draws that differ from the label

    out = {('P.' + k): v for k, v in to_np(model.state_dict()).items()}
    out.update(fc=fc.numpy(), att=att.numpy(), labels=labels.numpy(), masks=masks.numpy(), att_masks=att_masks.numpy(),
               ss_prob=np.array(SS_PROB), fed=fed.numpy(), logp=logp.detach().numpy(), loss=loss.detach().numpy())
    for k, p in model.named_parameters():
        out['grad.' + k] = p.grad.detach().numpy().copy()
    print('%-8s T_eff %d, %d of %d inputs after the first differ from the label, loss %.6f' %
          (name, T_eff, n_draw, (T_eff - 1) * N, loss.item()))
    return {'%s.%s' % (name, k): v for k, v in out.items()}


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models          # noqa: E402  (the reference)
    from captioning.modules import losses        # noqa: E402
    torch.set_num_threads(1)
    out = {}
    for name, seed, jitter in FAMILIES:
        out.update(one_family(models, losses, name, seed, jitter))
    path = os.path.join(HERE, 'ss_tiny.npz')
    save_npz(path, out)
    print('ss_tiny.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
