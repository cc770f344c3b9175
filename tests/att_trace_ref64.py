"""float64 replay of the per-word attention trace (imagecaptioning/pytorch_amd/att_trace.py), numpy only.

    weights()   alpha_net scores -> attention weights: softmax, mask, renormalise (Attention.forward, AttModel.py:741-745;
                AdaAtt_attention, :588-593: the sentinel is column 0 and takes the mask of region 0)
    trace()     per-step weights [S, N, Kc] + seq [N, L] -> att [N, L, Kout]: caption-major, zero columns behind the clipped K, zero
                steps where losses._shifted_mask is 0 and behind the S steps that were run
    ground()    att -> top (lowest index on ties, -1 on zeroed steps), top_w, entropy, attention-weighted box
"""
import numpy as np


def weights(scores, masks=None, sentinel=False):
    """scores [..., Kc] -> float64 weights; masks [..., K] (0 / 1) of the same leading shape, Kc = K + 1 with the sentinel"""
    s = np.asarray(scores, dtype=np.float64)
    e = np.exp(s - s.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    if masks is not None:
        m = np.asarray(masks, dtype=np.float64)
        if sentinel:
            m = np.concatenate([m[..., :1], m], -1)
        w = w * m
        w = w / w.sum(-1, keepdims=True)
    return w


def shifted_mask(seq):
    m = (np.asarray(seq) > 0)
    return np.concatenate([np.ones((m.shape[0], 1), dtype=bool), m[:, :-1]], 1)


def trace(step_weights, seq, Kout):
    """step_weights [S, N, Kc] -> att [N, L, Kout] float64"""
    w = np.asarray(step_weights, dtype=np.float64)
    S, N, Kc = w.shape
    L = seq.shape[1]
    att = np.zeros((N, L, Kout))
    att[:, :min(S, L), :Kc] = w.transpose(1, 0, 2)[:, :L]
    return att * shifted_mask(seq)[:, :, None]


def ground(att, boxes=None, n=1, col0=0):
    """-> dict(top int32 [N, L], top_w, entropy[, box [N, L, 4]]) in float64"""
    a = np.asarray(att, dtype=np.float64)
    kept = a.max(-1) > 0
    top = np.where(kept, a.argmax(-1), -1).astype(np.int32)          # numpy's argmax returns the first of equal values
    with np.errstate(divide='ignore', invalid='ignore'):
        ent = -np.where(a > 0, a * np.log(np.where(a > 0, a, 1.0)), 0.0).sum(-1)
    out = dict(top=top, top_w=np.where(kept, a.max(-1), 0.0), entropy=np.where(kept, ent, 0.0))
    if boxes is not None:
        b = np.asarray(boxes, dtype=np.float64)
        Kb = b.shape[1]
        img = np.arange(a.shape[0]) // n
        out['box'] = np.einsum('nlk,nkc->nlc', a[:, :, col0:col0 + Kb], b[img])
    return out
