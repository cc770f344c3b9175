"""fp64 torch restatement of Att2in2Model (reference AttModel.py:854-859 over Att2in2Core 750-790, Attention 719-748) --
a test helper: pinned to the reference by tests/golden/att2in2_tiny.npz (tests/test_att2in2_host.py), then used as the
yardstick of the HIP path at sizes no fixture covers.  P: dict of state_dict tensors (any device; cast to fp64 here).

Dropout masks, when given, are pre-scaled keep masks: drop_att [B,K,R], drop_x [T,N,E], drop_o [T,N,R]."""
import torch
import torch.nn.functional as F

D = torch.float64


def _p(P):
    return {k: v.to(D) for k, v in P.items()}


def prefill(P, att_feats, att_masks=None, drop_att=None):
    """(att' [B,K,R], p_att [B,K,A], masks [B,K] or None) after clip_att; padded regions are zero (pack_wrapper)."""
    att_feats = att_feats.to(D)
    if att_masks is not None:
        k = int(att_masks.long().sum(1).max())
        att_feats, att_masks = att_feats[:, :k], att_masks[:, :k].to(D)
        if drop_att is not None:
            drop_att = drop_att[:, :k]
    a = F.relu(att_feats @ P['att_embed.0.weight'].t() + P['att_embed.0.bias'])
    if drop_att is not None:
        a = a * drop_att.to(D)
    if att_masks is not None:
        a = a * att_masks.unsqueeze(-1)
    return a, a @ P['ctx2att.weight'].t() + P['ctx2att.bias'], att_masks


def step(P, it, h, c, att, p_att, att_masks, n, drop_x=None, drop_o=None):
    """One core step for N = B*n rows (image-major); returns (logits [N,V1], h', c')."""
    xt = F.relu(P['embed.0.weight'][it])
    if drop_x is not None:
        xt = xt * drop_x.to(D)
    att_r, patt_r = att.repeat_interleave(n, 0), p_att.repeat_interleave(n, 0)
    dot = torch.tanh(patt_r + (h @ P['core.attention.h2att.weight'].t() + P['core.attention.h2att.bias']).unsqueeze(1))
    e = (dot @ P['core.attention.alpha_net.weight'].t()).squeeze(-1) + P['core.attention.alpha_net.bias']
    w = F.softmax(e, dim=1)
    if att_masks is not None:
        w = w * att_masks.repeat_interleave(n, 0)
        w = w / w.sum(1, keepdim=True)
    ctx = torch.bmm(w.unsqueeze(1), att_r).squeeze(1)
    R = h.shape[1]
    s = xt @ P['core.i2h.weight'].t() + P['core.i2h.bias'] + h @ P['core.h2h.weight'].t() + P['core.h2h.bias']
    g = torch.sigmoid(s[:, :3 * R])
    cand = s[:, 3 * R:] + ctx @ P['core.a2c.weight'].t() + P['core.a2c.bias']
    cand = torch.max(cand[:, :R], cand[:, R:])
    c2 = g[:, R:2 * R] * c + g[:, :R] * cand
    h2 = g[:, 2 * R:] * torch.tanh(c2)
    out = h2 if drop_o is None else h2 * drop_o.to(D)
    return out @ P['logit.weight'].t() + P['logit.bias'], h2, c2


def xe(P, att_feats, att_masks, seq, drop_att=None, drop_x=None, drop_o=None, ss_coin=None, ss_gumbel=None):
    """Teacher-forced log-probs [N,T,V1] (AttModel._forward), with the trailing all-pad break.  Scheduled sampling with
    injected draws: where ss_coin[t, r] (t >= 1) the input of step t is argmax(logp[t-1] + ss_gumbel[t-1])."""
    P = _p(P)
    B = att_feats.shape[0]
    seq = seq.reshape(-1, seq.shape[-1])
    N, T = seq.shape
    n = N // B
    att, p_att, am = prefill(P, att_feats, att_masks, drop_att)
    R = P['core.h2h.weight'].shape[1]
    h = torch.zeros(N, R, dtype=D, device=att.device)
    c = torch.zeros_like(h)
    out = torch.zeros(N, T, P['logit.weight'].shape[0], dtype=D, device=att.device)
    for t in range(T):
        if t >= 1 and int(seq[:, t].sum()) == 0:
            break
        it = seq[:, t].clone()
        if ss_coin is not None and t >= 1:
            draw = (out[:, t - 1].detach() + ss_gumbel[t - 1].to(D)).argmax(1)
            it = torch.where(ss_coin[t].bool(), draw, it)
        logits, h, c = step(P, it, h, c, att, p_att, am, n, None if drop_x is None else drop_x[t],
                            None if drop_o is None else drop_o[t])
        out[:, t] = F.log_softmax(logits, 1)
    return out


def rollout(P, att_feats, att_masks, n, L, gumbel=None, drop_att=None, drop_x=None, drop_o=None):
    """Free-running decode (AttModel._sample): greedy, or with injected Gumbel noise [L,N,V1] the arg-max of logp + noise.
    Returns (seq [N,L], seqLogprobs [N,L,V1]) with the reference's finished-row masking."""
    P = _p(P)
    B = att_feats.shape[0]
    N = B * n
    att, p_att, am = prefill(P, att_feats, att_masks, drop_att)
    R = P['core.h2h.weight'].shape[1]
    V1 = P['logit.weight'].shape[0]
    dev = att.device
    h = torch.zeros(N, R, dtype=D, device=dev)
    c = torch.zeros_like(h)
    it = torch.zeros(N, dtype=torch.long, device=dev)
    seq = torch.zeros(N, L, dtype=torch.long, device=dev)
    slp = torch.zeros(N, L, V1, dtype=D, device=dev)
    unfinished = None
    for t in range(L):
        logits, h, c = step(P, it, h, c, att, p_att, am, n, None if drop_x is None else drop_x[t],
                            None if drop_o is None else drop_o[t])
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


def unpack_drops(z, tag, T_steps):
    """The DropRecorder record of a train-mode XE pass without att_masks: (drop_att [B,K,R], drop_x [T,N,E], drop_o [T,N,R])
    as pre-scaled fp32 keep masks.  Call order: att_embed once, then per step embed, core output."""
    import numpy as np
    p = z[tag + '.drop_p']
    assert len(p) == 1 + 2 * T_steps, len(p)

    def mask(i):
        shape = tuple(z['%s.drop%03d.shape' % (tag, i)])
        keep = np.unpackbits(z['%s.drop%03d' % (tag, i)])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
        return torch.from_numpy(keep / (1.0 - float(p[i])))
    drop_att = mask(0)
    drop_x = torch.stack([mask(1 + 2 * t) for t in range(T_steps)])
    drop_o = torch.stack([mask(2 + 2 * t) for t in range(T_steps)])
    return drop_att, drop_x, drop_o
