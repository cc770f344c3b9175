"""fp64 scheduled-sampling forwards (AttModel._forward with ss_prob > 0, reference AttModel.py:144-162) for NewFC and AoA -- a test
helper beside att2in2_ref64.py.  The single steps are the oracle's own (oracle.att_lstm.newfc_step, oracle.aoa.step: pinned to the
reference by their fixtures); only the time loop with the input choice is stated here, and that loop is itself pinned to the real
reference's scheduled sampling by tests/golden/ss_tiny.npz (tests/test_ss_host.py).

The input of step t >= 1, row r is chosen in one of two ways:
  * ``fed`` [T,N] (a table of the tokens really fed, e.g. a HIP run's it_all or the fixture's record): fed[t, r];
  * ``ss_coin`` [T,N] bool + ``ss_gumbel`` [T,N,V1]: arg-max(logp[t-1] + ss_gumbel[t-1]) where ss_coin[t, r], else seq[r, t]
    (the draw is not differentiated, AttModel.py:153).
Step 0 always feeds seq[:, 0]; the all-pad-column break looks at seq, not at the fed token (:158).
Returns (log-probs [N,T,V1] with zeros from the break on, the fed tokens [T_eff,N]).  P: dict of state_dict tensors, cast to
``dtype`` (fp64; fp32 serves to count how often the precision alone moves an arg-max)."""
import torch

from oracle import aoa as A, att_lstm as O

D = torch.float64


def _p(P, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in P.items()}


def _choose(seq, t, prev_logp, ss_coin, ss_gumbel, fed):
    if t == 0 or (fed is None and ss_coin is None):
        return seq[:, t].clone()
    if fed is not None:
        return fed[t].to(seq.device).long().clone()
    draw = (prev_logp.detach() + ss_gumbel[t - 1].to(prev_logp)).argmax(1)
    return torch.where(ss_coin[t].bool().to(seq.device), draw, seq[:, t])


def _loop(step, seq, V1, like, ss_coin, ss_gumbel, fed):
    N, T = seq.shape
    out = like.new_zeros(N, T, V1)
    used = []
    for t in range(T):
        if t >= 1 and int(seq[:, t].sum()) == 0:
            break
        it = _choose(seq, t, out[:, t - 1] if t else None, ss_coin, ss_gumbel, fed)
        used.append(it)
        out[:, t] = step(t, it)
    return out, torch.stack(used)


def newfc_xe(P, fc_feats, seq, ss_coin=None, ss_gumbel=None, fed=None, drop_out=None, dtype=D):
    """NewFCModel.  drop_out: pre-scaled keep masks [T,N,R] of the LSTMCore output dropout, or None."""
    P = _p(P, dtype)
    seq = seq.reshape(-1, seq.shape[-1])
    N = seq.shape[0]
    B = fc_feats.shape[0]
    fc = fc_feats.to(dtype) @ P['fc_embed.weight'].t() + P['fc_embed.bias']
    fc, = O.repeat_rows(N // B, fc)
    state = [O.zero_state(P, N, layers=1)]

    def step(t, it):
        logp, state[0] = O.newfc_step(P, it, fc, state[0], None if drop_out is None else drop_out[t].to(dtype))
        return logp
    return _loop(step, seq, P['logit.weight'].shape[0], fc, ss_coin, ss_gumbel, fed)


def aoa_xe(P, att_feats, att_masks, seq, h, ss_coin=None, ss_gumbel=None, fed=None, drop=None, dtype=D):
    """AoAModel.  drop(name, x): the oracle's dropout hook (oracle/aoa.py), or None."""
    P = _p(P, dtype)
    seq = seq.reshape(-1, seq.shape[-1])
    N = seq.shape[0]
    B = att_feats.shape[0]
    n = N // B
    am = None if att_masks is None else att_masks.to(dtype)
    mean, _, p_att, masks = A.prepare(P, att_feats.to(dtype), am, h, drop)
    if n > 1:
        mean, p_att = mean.repeat_interleave(n, 0), p_att.repeat_interleave(n, 0)
        masks = None if masks is None else masks.repeat_interleave(n, 0)
    R = mean.shape[1]
    state = [(mean.new_zeros(2, N, R), mean.new_zeros(2, N, R))]

    def step(t, it):
        logp, state[0] = A.step(P, it, mean, p_att, masks, state[0], h, drop, t)
        return logp
    return _loop(step, seq, P['logit.weight'].shape[0], mean, ss_coin, ss_gumbel, fed)


def lm_loss(logp, labels, masks):
    """LanguageModelCriterion (losses.py:203-219) on labels / masks [B,n,T+1] (column 0 = BOS), in logp's precision"""
    N, T = logp.shape[:2]
    tgt = labels[..., 1:].reshape(N, -1)[:, :T]
    m = masks[..., 1:].reshape(N, -1)[:, :T].to(logp)
    return -(logp.gather(2, tgt.unsqueeze(2)).squeeze(2) * m).sum() / m.sum()


def injection(fed, seq, V1, big=1e4):
    """(coin [T_eff,N] bool, noise [T_eff,N,V1] fp32) that make a run feed exactly `fed` [T_eff,N]: a coin wherever the fed token
    differs from the label (t >= 1), noise `big` at the token fed at t+1 stored in slice t (arg-max(logp[t] + noise[t]) is that
    token by construction) and 0 elsewhere."""
    T_eff, N = fed.shape
    seq = seq.reshape(N, -1)
    coin = fed != seq[:, :T_eff].t()
    assert not bool(coin[0].any())
    noise = torch.zeros(T_eff, N, V1)
    if T_eff > 1:
        noise[:-1].scatter_(2, fed[1:].unsqueeze(2), big)
    return coin, noise
