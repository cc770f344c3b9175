#!/usr/bin/env python3
"""Generate ``tests/golden/adaatt_tiny.npz``: the REAL reference's AdaAttModel / AdaAttMOModel (caption_model adaatt / adaattmo,
AttModel.py:451-613, 843-852) at make_golden.tiny_opt size with att_hid_size = 16 (the views at :569-582 need
input_encoding_size == rnn_size == att_hid_size), run on CPU with fixed seeds.  Run only where the reference checkout exists
(never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_adaatt.py

Like make_att2in2.py it imports the reference's own modules unmodified and only stores weights, inputs and outputs.  Per variant
(keys ``<variant>.<name>``): eval-mode XE log-probs / loss / gradients with ragged att_masks (region 0 valid for every image, as
the reference itself assumes at :592), greedy and beam-3 decodes, a RewardCriterion gradient over the (greedy, sample_n 2)
sequence with fixed rewards, a train-mode XE pass at drop_prob_lm 0.5 with every dropout call recorded
(make_golden.DropRecorder), and a scheduled-sampling pass (ss_prob 0.6, dropout off) with the token really fed at every step
recorded as make_ss.py does.

Two conditions are asserted before anything is written, so that fp32 rounding on another machine cannot flip a discrete result:
every greedy and beam decision of the stored decodes has a gap of at least 1e-3 in log-prob to its runner-up, and the stored
decodes are not degenerate (some row ends with EOS before seq_length, some row does not, no stored sequence is one token
repeated).  The (seed, perturbation scale) pairs below are the first of the search order that meet both; the seed is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, DropRecorder, tiny_opt, to_np      # noqa: E402
from make_ss import save_npz                                      # noqa: E402

MIN_GAP = 1e-3
SS_PROB = 0.6
SEARCH = [(seed, jit) for jit in (0.4, 0.3, 0.5, 0.25, 0.6) for seed in range(7000, 7040)]


class Reject(Exception):
    pass


def greedy_gaps(slp, seq):
    """smallest top-1 / top-2 gap over the decisions of rows that were still running"""
    gap = 1e9
    N, L, _ = slp.shape
    for r in range(N):
        for t in range(L):
            top = torch.topk(slp[r, t], 2).values
            gap = min(gap, float(top[0] - top[1]))
            if int(seq[r, t]) == 0:
                break
    return gap


def repeated(seq):
    """some stored sequence is one token repeated"""
    lens = (seq > 0).sum(1)
    return any(int(ln) >= 2 and len(set(row[:int(ln)].tolist())) == 1 for row, ln in zip(seq, lens))


def degenerate(seq, L):
    lens = (seq > 0).sum(1)
    return not (bool((lens < L).any()) and bool((lens == L).any())) or repeated(seq)


def one_variant(models, losses, name, seed, jitter):
    torch.manual_seed(seed)
    B, n, K, T = 3, 2, 6, 9          # T = seq_length + 1 inputs
    N = B * n
    opt = tiny_opt(name, drop=0.0)
    opt.att_hid_size = 16
    L = opt.seq_length
    model = models.setup(opt)
    with torch.no_grad():            # default inits leave some biases ~0: perturb everything so no term can hide
        for p in model.parameters():
            p.add_(jitter * torch.randn_like(p))
        model.logit.bias[0] += 0.5
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

    out = {('P.' + k): v for k, v in to_np(model.state_dict()).items()}
    out.update(fc=fc.numpy(), att=att.numpy(), labels=labels.numpy(), masks=masks.numpy(), att_masks=att_masks.numpy(),
               seed=np.array(seed), jitter=np.array(jitter))
    crit = losses.LanguageModelCriterion()

    # decodes first: they decide whether this (seed, jitter) is kept
    model.eval()
    with torch.no_grad():
        seq, slp = model(fc, att, att_masks, opt={'sample_method': 'greedy', 'beam_size': 1}, mode='sample')
        if degenerate(seq, L) or greedy_gaps(slp, seq) < MIN_GAP:
            raise Reject('greedy')
        out['greedy_seq'], out['greedy_logp'] = seq.numpy(), slp.numpy()
        sorts = []
        real_sort = torch.sort

        def spy_sort(x, *a, **k):
            ys, ix = real_sort(x, *a, **k)
            if x.dim() == 2 and len(a) >= 2 and a[1] is True:       # CaptionModel.beam_step: torch.sort(cand, 1, True)
                sorts.append(ys)
            return ys, ix
        torch.sort = spy_sort
        try:
            seq, slp = model(fc, att, att_masks, opt={'sample_method': 'greedy', 'beam_size': 3, 'sample_n': 1}, mode='sample')
        finally:
            torch.sort = real_sort
        assert sorts, 'the beam search sorted nothing through torch.sort'
        gap = 1e9
        for ys in sorts:             # the order of the first four candidates of every image and step (ended beams sit at -1000)
            w = min(4, ys.shape[1])
            d = ys[:, :w - 1] - ys[:, 1:w]
            gap = min(gap, float(torch.where(ys[:, 1:w] > -500, d, torch.full_like(d, 1e9)).min()))
        for beams in model.done_beams:
            ps = sorted((float(bm['p']) for bm in beams), reverse=True)
            if len(ps) > 1:
                gap = min(gap, ps[0] - ps[1])
        if gap < MIN_GAP or repeated(seq):
            raise Reject('beam')
        if np.array_equal(seq.numpy(), out['greedy_seq']):
            raise Reject('beam == greedy')
        out['beam3_seq'], out['beam3_logp'], out['beam3_min_gap'] = seq.numpy(), slp.numpy(), np.array(gap)

    # RewardCriterion over a fixed sequence: the greedy decode with sample_n 2 (deterministic), fixed rewards
    model.zero_grad()
    seq, slp = model(fc, att, att_masks, opt={'sample_method': 'greedy', 'beam_size': 1, 'sample_n': n}, mode='sample')
    if greedy_gaps(slp.detach(), seq) < MIN_GAP or repeated(seq):
        raise Reject('rl')
    reward = torch.from_numpy(np.random.RandomState(5).randn(N, 1).astype(np.float32)).repeat(1, seq.shape[1])
    rl = losses.RewardCriterion()(slp, seq.data, reward)
    rl.backward()
    out['rl_seq'], out['rl_logp'], out['rl_reward'], out['rl_loss'] = seq.numpy(), slp.detach().numpy(), reward.numpy(), rl.detach().numpy()
    for k, p in model.named_parameters():
        out['rl_grad.' + k] = p.grad.detach().numpy().copy()

    model.zero_grad()
    logp = model(fc, att, labels[..., :-1], att_masks)
    loss = crit(logp, labels[..., 1:], masks[..., 1:])
    loss.backward()
    out['xe_logp'], out['xe_loss'] = logp.detach().numpy(), loss.detach().numpy()
    for k, p in model.named_parameters():
        out['xe_grad.' + k] = p.grad.detach().numpy().copy()

    # scheduled sampling, every dropout off, the fed tokens recorded
    fed = []
    inner = model.get_logprobs_state

    def recording(it, *a, **kw):
        fed.append(it.detach().clone())
        return inner(it, *a, **kw)
    model.get_logprobs_state = recording
    model.train()
    model.ss_prob = SS_PROB
    model.zero_grad()
    torch.manual_seed(seed + 1000)
    logp = model(fc, att, labels[..., :-1], att_masks)
    loss = crit(logp, labels[..., 1:], masks[..., 1:])
    loss.backward()
    del model.get_logprobs_state
    model.ss_prob = 0.0
    fed = torch.stack(fed)
    assert fed.shape[0] == T - 1 and torch.equal(fed[0], labels[..., :-1].reshape(N, -1)[:, 0])
    # a drawn token must be a clear arg-max of "log-prob + a large constant at the fed token": it is, by construction
    out['ss_fed'], out['ss_logp'], out['ss_loss'] = fed.numpy(), logp.detach().numpy(), loss.detach().numpy()
    for k, p in model.named_parameters():
        out['ss_grad.' + k] = p.grad.detach().numpy().copy()

    # train mode, drop_prob_lm 0.5 at every site, no att_masks
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.5
    model.drop_prob_lm = model.core.lstm.drop_prob_lm = model.core.attention.drop_prob_lm = 0.5
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
    print('%-9s seed %d jitter %.2f: greedy lengths %s, beam gap %.3g, %d dropout calls' %
          (name, seed, jitter, (out['greedy_seq'] > 0).sum(1).tolist(), float(out['beam3_min_gap']), len(rec.calls)))
    return {'%s.%s' % (name, k): v for k, v in out.items()}


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    import captioning.models as models          # noqa: E402  (the reference)
    from captioning.modules import losses        # noqa: E402
    torch.set_num_threads(1)
    out = {}
    for name in ('adaatt', 'adaattmo'):
        for seed, jitter in SEARCH:
            try:
                out.update(one_variant(models, losses, name, seed, jitter))
                break
            except Reject as e:
                print('%s seed %d jitter %.2f rejected (%s)' % (name, seed, jitter, e))
        else:
            raise SystemExit('no (seed, jitter) of the search order meets the fixture conditions for ' + name)
    path = os.path.join(HERE, 'adaatt_tiny.npz')
    save_npz(path, out)
    print('adaatt_tiny.npz:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
