"""float64 torch restatement of the use_bn prefill (reference AttModel.py:80-85 under pack_wrapper :44-49, _prepare_feature :114-124)
and of the teacher-forced / free-running passes of UpDown and Att2in2 on it -- a test helper: pinned to the reference by
tests/golden/use_bn_tiny_*.npz (tests/test_use_bn_host.py), then the yardstick of the HIP path at sizes no fixture covers.
Its backward is autograd's.

P: dict of the model's parameters AND buffers (state_dict names; any device; float tensors are cast to float64 by p64()).
BatchNorm over the M valid region rows: train = batch mean / biased variance, eps 1e-5, and the running buffers move with
momentum 0.1 on the unbiased variance; eval = the running statistics.  att_masks None: all B * K rows are valid.
Dropout masks are pre-scaled keep masks."""
import torch
import torch.nn.functional as F

import att2in2_ref64
from oracle import att_lstm

D = torch.float64
EPS, MOMENTUM = 1e-5, 0.1


def p64(P, grad=False):
    out = {}
    for k, v in P.items():
        v = v.detach()
        out[k] = v.to(D).requires_grad_(grad and 'running_' not in k) if v.is_floating_point() else v.clone()
    return out


def use_bn_of(P):
    return 0 if 'att_embed.1.weight' not in P else (2 if 'att_embed.4.weight' in P else 1)


def batch_norm(x, valid, P, name, train, new_bufs):
    """x [rows, C]; valid [rows] bool; statistics over the valid rows; -> y [rows, C] (padded rows are whatever the affine map gives;
    the caller zeroes them).  train: the updated buffers go to new_bufs (P is left alone)."""
    g, b = P[name + '.weight'], P[name + '.bias']
    if train:
        xv = x[valid]
        M = xv.shape[0]
        mean = xv.mean(0)
        var = ((xv - mean) ** 2).mean(0)
        if new_bufs is not None and M >= 2:
            new_bufs[name + '.running_mean'] = ((1 - MOMENTUM) * P[name + '.running_mean'] + MOMENTUM * mean).detach()
            new_bufs[name + '.running_var'] = ((1 - MOMENTUM) * P[name + '.running_var'] + MOMENTUM * var * M / (M - 1)).detach()
            new_bufs[name + '.num_batches_tracked'] = P[name + '.num_batches_tracked'] + 1
    else:
        mean, var = P[name + '.running_mean'], P[name + '.running_var']
    return (x - mean) / torch.sqrt(var + EPS) * g + b


def att_embed(P, att_feats, att_masks=None, train=False, drop_att=None, new_bufs=None):
    """(att' [B,K,R], p_att [B,K,A], masks [B,K] or None) after clip_att; padded regions of att' are zero"""
    att_feats = att_feats.to(D)
    if att_masks is not None:
        k = int(att_masks.long().sum(1).max())
        att_feats, att_masks = att_feats[:, :k], att_masks[:, :k].to(D)
        if drop_att is not None:
            drop_att = drop_att[:, :k]
    B, K, C = att_feats.shape
    use_bn = use_bn_of(P)
    lin = 'att_embed.1' if use_bn else 'att_embed.0'
    valid = torch.ones(B * K, dtype=torch.bool, device=att_feats.device) if att_masks is None else att_masks.reshape(-1) > 0
    x = att_feats.reshape(B * K, C)
    if use_bn:
        x = batch_norm(x, valid, P, 'att_embed.0', train, new_bufs)
    a = F.relu(x @ P[lin + '.weight'].t() + P[lin + '.bias'])
    if drop_att is not None:
        a = a * drop_att.to(D).reshape(B * K, -1)
    if use_bn == 2:
        a = batch_norm(a, valid, P, 'att_embed.4', train, new_bufs)
    a = (a * valid.to(D).unsqueeze(1)).reshape(B, K, -1)
    return a, a @ P['ctx2att.weight'].t() + P['ctx2att.bias'], att_masks


def xe(family, P, fc_feats, att_feats, att_masks, seq, train=False, drops=None, new_bufs=None):
    """teacher-forced log-probs [N,T,V1] (AttModel._forward) with the trailing all-pad break.  P: p64() tensors.
    drops: att_lstm.Drops (fc only for UpDown) or None."""
    drops = drops or att_lstm.Drops()
    B = att_feats.shape[0]
    seq = seq.reshape(-1, seq.shape[-1])
    N, T = seq.shape
    n = N // B
    att, p_att, am = att_embed(P, att_feats, att_masks, train, drops.att, new_bufs)
    V1 = P['logit.weight'].shape[0]
    out = torch.zeros(N, T, V1, dtype=D, device=att.device)
    if family == 'updown':
        fc = F.relu(fc_feats.to(D) @ P['fc_embed.0.weight'].t() + P['fc_embed.0.bias'])
        if drops.fc is not None:
            fc = fc * drops.fc.to(D)
        fc, att_r, p_att_r, am_r = att_lstm.repeat_rows(n, fc, att, p_att, am)
        state = att_lstm.zero_state(P, N)
        state = tuple(s.to(D) for s in state) if isinstance(state, tuple) else state
    else:
        R = P['core.h2h.weight'].shape[1]
        h = torch.zeros(N, R, dtype=D, device=att.device)
        c = torch.zeros_like(h)
    for t in range(T):
        if t >= 1 and int(seq[:, t].sum()) == 0:
            break
        dx = None if drops.xt is None else drops.xt[t].to(D)
        do = None if drops.out is None else drops.out[t].to(D)
        if family == 'updown':
            logp, state = att_lstm.updown_step(P, seq[:, t], fc, att_r, p_att_r, am_r, state, dx, do)
        else:
            logits, h, c = att2in2_ref64.step(P, seq[:, t], h, c, att, p_att, am, n, dx, do)
            logp = F.log_softmax(logits, 1)
        out[:, t] = logp
    return out


def lm_loss(logp, labels, masks):
    """LanguageModelCriterion on labels / masks [B,n,T+1] (shifted here)"""
    N, T = logp.shape[:2]
    tgt = labels[..., 1:].reshape(N, -1)[:, :T]
    m = masks[..., 1:].reshape(N, -1)[:, :T].to(D)
    return -(logp.gather(2, tgt.unsqueeze(2)).squeeze(2) * m).sum() / m.sum()


def greedy(family, P, fc_feats, att_feats, att_masks, L, n=1, gumbel=None, train=False, new_bufs=None):
    """free-running decode in eval numerics of the decoder (no dropout): arg-max of logp (+ injected Gumbel noise [L,N,V1]);
    train: the prefill uses batch statistics.  -> (seq [N,L], seqLogprobs [N,L,V1]) with the reference's finished-row masking."""
    B = att_feats.shape[0]
    N = B * n
    att, p_att, am = att_embed(P, att_feats, att_masks, train, None, new_bufs)
    V1 = P['logit.weight'].shape[0]
    dev = att.device
    if family == 'updown':
        fc = F.relu(fc_feats.to(D) @ P['fc_embed.0.weight'].t() + P['fc_embed.0.bias'])
        fc, att_r, p_att_r, am_r = att_lstm.repeat_rows(n, fc, att, p_att, am)
        state = att_lstm.zero_state(P, N)
    else:
        R = P['core.h2h.weight'].shape[1]
        h = torch.zeros(N, R, dtype=D, device=dev)
        c = torch.zeros_like(h)
    it = torch.zeros(N, dtype=torch.long, device=dev)
    seq = torch.zeros(N, L, dtype=torch.long, device=dev)
    slp = torch.zeros(N, L, V1, dtype=D, device=dev)
    unfinished = None
    for t in range(L):
        if family == 'updown':
            logp, state = att_lstm.updown_step(P, it, fc, att_r, p_att_r, am_r, state, None, None)
        else:
            logits, h, c = att2in2_ref64.step(P, it, h, c, att, p_att, am, n, None, None)
            logp = F.log_softmax(logits, 1)
        score = logp.detach() if gumbel is None else logp.detach() + gumbel[t].to(D)
        it = score.argmax(1)
        if t == 0:
            unfinished = it != 0
        else:
            it = torch.where(unfinished, it, torch.zeros_like(it))
            logp = logp * unfinished.unsqueeze(1).to(D)
            unfinished = unfinished & (it != 0)
        seq[:, t] = it
        slp[:, t] = logp
        if int(unfinished.sum()) == 0:
            break
    return seq, slp
