"""fp64 torch restatement of AdaAttModel / AdaAttMOModel (reference AttModel.py:843-852 over AdaAttCore 604-613 = AdaAtt_lstm
451-537 + AdaAtt_attention 539-602, one layer) -- a test helper: pinned to the reference by tests/golden/adaatt_tiny.npz
(tests/test_adaatt_host.py), then used as the yardstick of the HIP path at sizes no fixture covers.  P: dict of state_dict
tensors (any device; cast to fp64 here).  The variant (tanh or maxout candidate) is read off the width of core.lstm.w2h.

Dropout masks, when given, are a dict of pre-scaled keep masks: fc [B,R], att [B,K,R], and per step xt [T,N,E], h, fake [T,N,R],
fr, ho [T,N,E], tile [T,N,K+1,A], out [T,N,R]."""
import torch
import torch.nn.functional as F

D = torch.float64
STEP_SITES = ('xt', 'h', 'fake', 'fr', 'ho', 'tile', 'out')       # the reference's call order inside one step


def _p(P):
    return {k: v.to(D) for k, v in P.items()}


def _lin(P, name, x):
    return x @ P[name + '.weight'].t() + P[name + '.bias']


def prefill(P, fc_feats, att_feats, att_masks=None, drops=None):
    """(fc' [B,R], att' [B,K,R], p_att [B,K,A], masks [B,K] or None) after clip_att; padded regions are zero (pack_wrapper)."""
    drops = drops or {}
    att_feats = att_feats.to(D)
    d_att = drops.get('att')
    if att_masks is not None:
        k = int(att_masks.long().sum(1).max())
        att_feats, att_masks = att_feats[:, :k], att_masks[:, :k].to(D)
        if d_att is not None:
            d_att = d_att[:, :k]
    fc = F.relu(_lin(P, 'fc_embed.0', fc_feats.to(D)))
    if drops.get('fc') is not None:
        fc = fc * drops['fc'].to(D)
    a = F.relu(_lin(P, 'att_embed.0', att_feats))
    if d_att is not None:
        a = a * d_att.to(D)
    if att_masks is not None:
        a = a * att_masks.unsqueeze(-1)
    return fc, a, _lin(P, 'ctx2att', a), att_masks


def step(P, it, h, c, fc, att, p_att, att_masks, n, d=None):
    """One core step for N = B*n rows (image-major); d: this step's keep masks by site.  Returns (logits [N,V1], h', c')."""
    d = d or {}
    m = lambda x, k: x if d.get(k) is None else x * d[k].to(D)       # noqa: E731
    R = h.shape[1]
    maxout = P['core.lstm.w2h.weight'].shape[0] == 5 * R
    xt = m(F.relu(P['embed.0.weight'][it]), 'xt')
    fc_r = fc.repeat_interleave(n, 0)
    s = _lin(P, 'core.lstm.w2h', xt) + _lin(P, 'core.lstm.v2h', fc_r) + _lin(P, 'core.lstm.h2h.0', h)
    g = torch.sigmoid(s[:, :3 * R])
    cand = torch.max(s[:, 3 * R:4 * R], s[:, 4 * R:]) if maxout else torch.tanh(s[:, 3 * R:])
    c2 = g[:, R:2 * R] * c + g[:, :R] * cand
    tc = torch.tanh(c2)
    h2 = g[:, 2 * R:] * tc
    n5 = _lin(P, 'core.lstm.r_w2h', xt) + _lin(P, 'core.lstm.r_v2h', fc_r) + _lin(P, 'core.lstm.r_h2h', h)
    fake = m(torch.sigmoid(n5) * tc, 'fake')
    h_out = m(h2, 'h')                                   # the state keeps the undropped h2
    # AdaAtt_attention
    fr = m(F.relu(_lin(P, 'core.attention.fr_linear.0', fake)), 'fr')
    fr_e = _lin(P, 'core.attention.fr_embed', fr)
    ho = m(torch.tanh(_lin(P, 'core.attention.ho_linear.0', h_out)), 'ho')
    ho_e = _lin(P, 'core.attention.ho_embed', ho)
    img = torch.cat([fr.unsqueeze(1), att.repeat_interleave(n, 0)], 1)
    img_e = torch.cat([fr_e.unsqueeze(1), p_att.repeat_interleave(n, 0)], 1)
    hA = m(torch.tanh(img_e + ho_e.unsqueeze(1)), 'tile')
    e = (hA @ P['core.attention.alpha_net.weight'].t()).squeeze(-1) + P['core.attention.alpha_net.bias']
    pi = F.softmax(e, dim=1)
    if att_masks is not None:
        am = att_masks.repeat_interleave(n, 0)
        pi = pi * torch.cat([am[:, :1], am], 1)          # the sentinel takes the mask of region 0 (AttModel.py:592)
        pi = pi / pi.sum(1, keepdim=True)
    ctx = torch.bmm(pi.unsqueeze(1), img).squeeze(1) + ho
    out = m(torch.tanh(_lin(P, 'core.attention.att2h', ctx)), 'out')
    return _lin(P, 'logit', out), h2, c2


def _at(drops, t):
    return None if not drops else {k: drops[k][t] for k in STEP_SITES if drops.get(k) is not None}


def xe(P, fc_feats, att_feats, att_masks, seq, drops=None, ss_coin=None, ss_gumbel=None):
    """Teacher-forced log-probs [N,T,V1] (AttModel._forward), with the trailing all-pad break.  Scheduled sampling with
    injected draws: where ss_coin[t, r] (t >= 1) the input of step t is argmax(logp[t-1] + ss_gumbel[t-1])."""
    P = _p(P)
    B = att_feats.shape[0]
    seq = seq.reshape(-1, seq.shape[-1])
    N, T = seq.shape
    n = N // B
    fc, att, p_att, am = prefill(P, fc_feats, att_feats, att_masks, drops)
    R = P['core.lstm.r_h2h.weight'].shape[0]
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
        logits, h, c = step(P, it, h, c, fc, att, p_att, am, n, _at(drops, t))
        out[:, t] = F.log_softmax(logits, 1)
    return out


def rollout(P, fc_feats, att_feats, att_masks, n, L, gumbel=None, drops=None):
    """Free-running decode (AttModel._sample): greedy, or with injected Gumbel noise [L,N,V1] the arg-max of logp + noise.
    Returns (seq [N,L], seqLogprobs [N,L,V1]) with the reference's finished-row masking."""
    P = _p(P)
    B = att_feats.shape[0]
    N = B * n
    fc, att, p_att, am = prefill(P, fc_feats, att_feats, att_masks, drops)
    R = P['core.lstm.r_h2h.weight'].shape[0]
    V1 = P['logit.weight'].shape[0]
    dev = att.device
    h = torch.zeros(N, R, dtype=D, device=dev)
    c = torch.zeros_like(h)
    it = torch.zeros(N, dtype=torch.long, device=dev)
    seq = torch.zeros(N, L, dtype=torch.long, device=dev)
    slp = torch.zeros(N, L, V1, dtype=D, device=dev)
    unfinished = None
    for t in range(L):
        logits, h, c = step(P, it, h, c, fc, att, p_att, am, n, _at(drops, t))
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
    """The DropRecorder record of a train-mode XE pass without att_masks as the dict prefill / step take.  Call order of the
    reference: fc_embed, att_embed, then per step embed, lstm h, lstm sentinel, fr_linear, ho_linear, the tanh tile, the output."""
    import numpy as np
    p = z[tag + '.drop_p']
    assert len(p) == 2 + len(STEP_SITES) * T_steps, len(p)

    def mask(i):
        shape = tuple(z['%s.drop%03d.shape' % (tag, i)])
        keep = np.unpackbits(z['%s.drop%03d' % (tag, i)])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
        return torch.from_numpy(keep / (1.0 - float(p[i])))
    out = {'fc': mask(0), 'att': mask(1)}
    for s, name in enumerate(STEP_SITES):
        out[name] = torch.stack([mask(2 + len(STEP_SITES) * t + s) for t in range(T_steps)])
    return out
