"""fp64 restatement of a TRAIN-MODE beam search as the HIP backend runs it (search with dropout masks laid out by search row,
finalise, lineage, forced replay with gradient) for UpDown and NewFC -- a test helper in the role of att2in2_ref64.py /
ss_ref64.py: pinned to the reference by tests/golden/beam_train_tiny.npz (tests/test_beam_train_host.py), then the yardstick of
the kernels.  The decoder steps are oracle/att_lstm.py's (dtype-agnostic), run on float64 copies of the weights.

Reference: AttModel._sample_beam (AttModel.py:218-256) + CaptionModel.beam_search (CaptionModel.py:35-209), group_size 1,
called in train() mode.  Masks are pre-scaled keep masks:

    updown: drop_fc [B,R], drop_att [B,K,R], drop_xt [L,B*bd,E], drop_out [L,B*bd,R]
    newfc:  drop_out [L,B*bd,R]

Slot t of drop_xt / drop_out belongs to the decoder call that produces the distributions step t selects from; call 0 runs on
one row per image (rows 0..B-1 of slot 0), the later calls on B*bd rows, image-major.
"""
import numpy as np
import torch

from oracle import att_lstm as O

D = torch.float64


def penalty_fn(cfg):
    """captioning/utils/misc.py:133-157 penalty_builder."""
    if cfg == '':
        return lambda length, logp: logp
    kind, alpha = cfg.split('_')
    alpha = float(alpha)
    if kind == 'wu':
        return lambda length, logp: logp / (((5 + length) ** alpha) / ((5 + 1) ** alpha))
    if kind == 'avg':
        return lambda length, logp: logp / length
    raise ValueError(cfg)


def _p64(P):
    return {k: torch.as_tensor(v).to(D) for k, v in P.items()}


def _m(masks, key, t=None, rows=None):
    m = (masks or {}).get(key)
    if m is None:
        return None
    m = torch.as_tensor(m).to(D)
    return m if t is None else m[t][:rows]


class _Decoder:
    """One family's decoder over `rows` image-major rows: step(it, rows_per_image, drop_xt, drop_out) -> logp; reorder(idx)."""

    def __init__(self, family, P, fc_feats, att_feats, att_masks, masks):
        self.family, self.P = family, P
        if family == 'updown':
            drops = O.Drops(fc=_m(masks, 'drop_fc'), att=_m(masks, 'drop_att'))
            self.fc, self.att, self.p_att, self.am = O.prepare_feature(P, fc_feats.to(D), att_feats.to(D), att_masks, drops)
            self.state = None
        else:
            self.fc = fc_feats.to(D) @ P['fc_embed.weight'].t() + P['fc_embed.bias']
            self.state = None

    def start(self, row_img):
        """rows given by their image index (int64 [rows]); zero state (NewFC: the image step is taken inside the first step)."""
        self.row_img = row_img
        self.state = O.zero_state(self.P, len(row_img), layers=2 if self.family == 'updown' else 1)

    def step(self, it, drop_xt=None, drop_out=None):
        ri = self.row_img
        if self.family == 'updown':
            am = None if self.am is None else self.am[ri]
            logp, self.state = O.updown_step(self.P, it, self.fc[ri], self.att[ri], self.p_att[ri], am, self.state, drop_xt, drop_out)
        else:
            logp, self.state = O.newfc_step(self.P, it, self.fc[ri], self.state, drop_out)
        return logp

    def reorder(self, src_rows, row_img):
        self.state = tuple(s[:, src_rows] for s in self.state)
        self.row_img = row_img


def search(family, P, fc_feats, att_feats, att_masks, bd, L, masks=None):
    """The search; returns dict(parent [L,B,bd] int32, token int64, score float64, ended uint8, gap: the smallest difference
    between the last kept and the first dropped candidate over all steps and images)."""
    P = _p64(P)
    B = fc_feats.shape[0]
    V1 = P['logit.weight'].shape[0]
    dec = _Decoder(family, P, fc_feats, att_feats, att_masks, masks)
    parent = np.zeros((L, B, bd), np.int32)
    token = np.zeros((L, B, bd), np.int64)
    score = np.zeros((L, B, bd), np.float64)
    ended = np.zeros((L, B, bd), np.uint8)
    gap = float('inf')
    with torch.no_grad():
        dec.start(torch.arange(B))
        logp = dec.step(torch.zeros(B, dtype=torch.long), _m(masks, 'drop_xt', 0, B), _m(masks, 'drop_out', 0, B))
        sums = torch.zeros(B, 1, dtype=D)
        cur = 1
        for t in range(L):
            cand = (sums.unsqueeze(2) + logp.view(B, cur, V1)).reshape(B, cur * V1)
            val, idx = torch.sort(cand, dim=1, descending=True, stable=True)
            gap = min(gap, float((val[:, bd - 1] - val[:, bd]).min()))
            val, idx = val[:, :bd], idx[:, :bd]
            par, tok = idx // V1, idx % V1
            end = (tok == 0) | (t == L - 1)
            parent[t], token[t], score[t], ended[t] = par.numpy(), tok.numpy(), val.numpy(), end.numpy()
            if t == L - 1:
                break
            sums = torch.where(end, val - 1000.0, val)                        # CaptionModel.py:198
            img = torch.arange(B).repeat_interleave(bd)
            dec.reorder((torch.arange(B).unsqueeze(1) * cur + par).reshape(-1), img)
            logp = dec.step(tok.reshape(-1), _m(masks, 'drop_xt', t + 1, B * bd), _m(masks, 'drop_out', t + 1, B * bd))
            cur = bd
    return dict(parent=parent, token=token, score=score, ended=ended, gap=gap)


def finalize(parent, token, score, ended, sample_n, length_penalty=''):
    """CaptionModel.py:183-208 in NumPy: candidates = ended (t, j) in order of t then j, key = penalty(t + 1, score) in Python
    doubles, stable descending sort, the best sample_n.  score is taken as given (float32 tables -> float(score), as the host
    code does).  Returns seq [B*sample_n, L] int64, lineage [L, B*sample_n] int32 (-1 behind the end), length, p (float64),
    p_gap (smallest difference between neighbouring kept-or-first-dropped keys)."""
    L, B, bd = parent.shape
    pen = penalty_fn(length_penalty)
    rows = B * sample_n
    seq = np.zeros((rows, L), np.int64)
    lineage = np.full((L, rows), -1, np.int32)
    length = np.zeros(rows, np.int32)
    p = np.zeros(rows, np.float64)
    p_gap = float('inf')
    for b in range(B):
        fin = [(pen(t + 1, float(score[t, b, j])), t, j) for t in range(L) for j in range(bd) if ended[t, b, j]]
        fin = sorted(fin, key=lambda x: -x[0])
        for a, c in zip(fin[:bd], fin[1:bd + 1]):
            p_gap = min(p_gap, a[0] - c[0])
        for i, (pv, t, j) in enumerate(fin[:sample_n]):
            row = b * sample_n + i
            jj = j
            for s in range(t, -1, -1):
                seq[row, s] = token[s, b, jj]
                par = int(parent[s, b, jj])
                lineage[s, row] = b if s == 0 else b * bd + par
                jj = par
            length[row], p[row] = t + 1, pv
    return seq, lineage, length, p, p_gap


def replay(family, P, fc_feats, att_feats, att_masks, seq, lineage, sample_n, masks=None):
    """Forced rollout of the returned beams with the masks their ancestors saw: seqLogprobs [B*sample_n, L, V1] (float64, with
    autograd through P when its tensors require grad), rows zero from the step after a beam's end on (AttModel.py:330-340)."""
    B = fc_feats.shape[0]
    seq = torch.as_tensor(seq)
    lineage = torch.as_tensor(np.asarray(lineage)).long().clamp_min(0)
    rows, L = seq.shape
    V1 = P['logit.weight'].shape[0]
    dec = _Decoder(family, P, fc_feats, att_feats, att_masks, masks)
    dec.start(torch.arange(B).repeat_interleave(sample_n))
    out = []
    it = torch.zeros(rows, dtype=torch.long)
    unfinished = torch.ones(rows, dtype=torch.bool)
    for t in range(L):
        dx, do = _m(masks, 'drop_xt'), _m(masks, 'drop_out')
        logp = dec.step(it, None if dx is None else dx[t][lineage[t]], None if do is None else do[t][lineage[t]])
        it = seq[:, t]
        out.append(logp * unfinished.unsqueeze(1).to(D))
        unfinished = unfinished & (it != 0)
    return torch.stack(out, 1)


def replay_loss_grads(family, P, fc_feats, att_feats, att_masks, seq, lineage, sample_n, masks, reward, dtype=D):
    """The forced replay, its RewardCriterion loss and every parameter gradient in `dtype`: float64 is the yardstick; float32 is
    the SAME restatement at the kernels' precision -- its distance from the float64 run is what fp32 arithmetic alone costs a
    gradient, the measure a config-size test falls back on where 1e-3 is too tight.  Returns (logp, loss, grads)."""
    global D
    keep, D = D, dtype
    try:
        Pg = {k: torch.as_tensor(v).to(D).clone().requires_grad_(True) for k, v in P.items()}
        logp = replay(family, Pg, fc_feats, att_feats, att_masks, seq, lineage, sample_n, masks)
        loss = O.reward_criterion(logp, torch.as_tensor(seq), torch.as_tensor(reward).to(D))
        loss.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in Pg.items()}
        return logp.detach(), float(loss.detach()), grads
    finally:
        D = keep


def run(family, P, fc_feats, att_feats, att_masks, bd, sample_n, L, length_penalty='', masks=None, reward=None):
    """search -> finalize -> replay; with `reward` [rows, L] also the RewardCriterion loss and every parameter gradient."""
    s = search(family, P, fc_feats, att_feats, att_masks, bd, L, masks)
    seq, lineage, length, p, p_gap = finalize(s['parent'], s['token'], s['score'], s['ended'], sample_n, length_penalty)
    res = dict(s, seq=seq, lineage=lineage, length=length, p=p, p_gap=p_gap)
    if reward is not None:
        res['logp'], res['loss'], res['grads'] = replay_loss_grads(family, P, fc_feats, att_feats, att_masks, seq, lineage, sample_n,
                                                                   masks, reward)
    else:
        with torch.no_grad():
            res['logp'] = replay(family, _p64(P), fc_feats, att_feats, att_masks, seq, lineage, sample_n, masks)
    return res


def mask_dict(family, drops):
    """oracle.att_lstm.make_drops(p, B, K, B*bd, L, E, R, g) -> the masks by search row as this module and opt['_beam_masks'] take
    them (NewFC drops the LSTM output only)."""
    if family == 'updown':
        return dict(drop_fc=drops.fc, drop_att=drops.att, drop_xt=drops.xt, drop_out=drops.out)
    return dict(drop_out=drops.out)


# ------------------------------------------------------------------------------------------------------ fixture plumbing
def unpack_regions(packed, am):
    """The reference drops att_embed's output on the PACKED regions (AttModel.pack_wrapper, AttModel.py:44-49: rows sorted by
    length descending, then time-major): scatter [sum(len), R] back to [B, K', R]; padded positions get 0."""
    lens = torch.as_tensor(am).long().sum(1)
    order = sorted(range(len(lens)), key=lambda b: -int(lens[b]))
    assert len(set(lens.tolist())) == len(lens), 'fixture rows must have distinct lengths'
    out = packed.new_zeros(len(lens), int(lens.max()), packed.shape[1])
    r = 0
    for t in range(int(lens.max())):
        for b in order:
            if int(lens[b]) > t:
                out[b, t] = packed[r]
                r += 1
    assert r == packed.shape[0]
    return out


def recorded_masks(z, tag, family, B, bd, L, att_masks=None):
    """The DropRecorder record of a reference train-mode beam search -> the masks by search row (float32, pre-scaled).
    Call order -- updown: fc_embed [B,R], att_embed (packed or [B,K,R]), then per decoder call embed, core output: [B,.] for
    the first call, [B*bd,.] for the following L (the last call's output is never used).  newfc: the image step's discarded
    output [B,R], the first word step [B,R], then L times [B*bd,R]."""
    p = z[tag + '.drop_p']

    def mask(i):
        shape = tuple(z['%s.drop%03d.shape' % (tag, i)])
        keep = np.unpackbits(z['%s.drop%03d' % (tag, i)])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
        return torch.from_numpy(keep / (1.0 - float(p[i])))
    N = B * bd

    def by_row(first, rest):
        out = torch.ones(L, N, first.shape[1])
        out[0, :B] = first
        for t in range(1, L):
            assert rest[t - 1].shape[0] == N
            out[t] = rest[t - 1]
        return out
    if family == 'updown':
        assert len(p) == 2 + 2 * (L + 1), len(p)
        att = mask(1)
        if att.ndim == 2:
            att = unpack_regions(att, att_masks)
        assert mask(2).shape[0] == B and mask(3).shape[0] == B
        return dict(drop_fc=mask(0), drop_att=att, drop_xt=by_row(mask(2), [mask(4 + 2 * t) for t in range(L)]),
                    drop_out=by_row(mask(3), [mask(5 + 2 * t) for t in range(L)]))
    assert len(p) == 2 + L, len(p)
    assert mask(0).shape[0] == B and mask(1).shape[0] == B
    return dict(drop_out=by_row(mask(1), [mask(2 + t) for t in range(L)]))
