"""Float64 replay of the AoANet captioner under every ablation switch of AoAModel.py:100-226 (decoder_type AoA / LSTM / base,
out_res, ctx_drop, mean_feats, refine, refine_aoa, use_ff), for tests/test_aoa_variants_gpu.py and the fixture script
tests/golden/make_aoa_variants.py.  Test infrastructure: plain PyTorch on the CPU over the reference's state_dict keys.

Dropout is injected through ``drop(name, tensor)`` (identity when None), the protocol of oracle/aoa.py.  Hook names:
att_embed, fc_embed, ref<i>.attn / .aoa / .res / .ff / .res2, and per decode step xt<t>, ctx<t> (only with ctx_drop 1), dec<t>.attn,
out<t>.

Also the shared description of the variants (VARIANTS, variant_opt) and of the two feed-forward weights per refiner layer, which
the fixture does not store: 6 x 2 x 2048 x 16 floats per use_ff variant would not fit a committed file, so both sides build them
from ``ff_weight`` (numpy's RandomState stream is frozen across numpy versions).
"""
import argparse

import numpy as np
import torch
import torch.nn.functional as F

from oracle.aoa import dot_attention
from oracle.transformer import layer_norm, _d

FF_HIDDEN = 2048
SIZE = dict(R=16, E=16, h=2, V=20, L=5, B=3, K=5, F=20, n=2)

# tag -> switches moved away from configs/aoa.yml (refine 1, refine_aoa 1, use_ff 0, decoder_type AoA, mean_feats 1, ctx_drop 1, out_res 0)
VARIANTS = {
    'A': dict(decoder_type='LSTM'),
    'B': dict(decoder_type='base', out_res=1),
    'C': dict(refine_aoa=0, use_ff=1),
    'D': dict(refine=0, mean_feats=0, ctx_drop=0),
    'E': dict(decoder_type='LSTM', out_res=1, use_ff=1, mean_feats=0),
}


def variant_opt(tag, **kw):
    s = SIZE
    o = argparse.Namespace(caption_model='aoa', vocab_size=s['V'], input_encoding_size=s['E'], rnn_size=s['R'], num_layers=2,
                           drop_prob_lm=0.0, seq_length=s['L'], max_length=s['L'], fc_feat_size=s['F'], att_feat_size=s['F'],
                           att_hid_size=12, use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, s['V'] + 1)},
                           rnn_type='lstm', refine=1, refine_aoa=1, use_ff=0, decoder_type='AoA', use_multi_head=2, num_heads=s['h'],
                           multi_head_scale=1, mean_feats=1, ctx_drop=1, out_res=0, dropout_aoa=0.3)
    for k, v in dict(VARIANTS[tag], **kw).items():
        setattr(o, k, v)
    return o


def is_ff_weight(key):
    """the refiner's feed-forward tensors with a 2048 axis that the fixture rebuilds instead of storing: w_1.weight, w_1.bias, w_2.weight"""
    return '.feed_forward.w_' in key and not key.endswith('w_2.bias')


def ff_weight(tag, key, shape):
    """the feed-forward weight `key` of variant `tag` (float32): a fixed stream per (variant, key)"""
    seed = (sum(ord(c) * (i + 1) for i, c in enumerate(tag + '/' + key)) * 2654435761) % (2 ** 31)
    scale = 0.5 / np.sqrt(shape[1]) if len(shape) == 2 else 0.1
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def ff_grad_digest(g):
    """what the fixture keeps of a feed-forward weight gradient (hidden units along `axis` 0 of w_1, 1 of w_2): the sums over
    every 32 consecutive hidden units (all elements take part) and every 32nd hidden unit as it is"""
    g = np.asarray(g)
    if g.ndim == 1:
        g = g[:, None]
    if g.shape[0] != FF_HIDDEN:
        g = g.T
    return g.reshape(FF_HIDDEN // 32, 32, -1).sum(1), g[::32].copy()


def pack(named):
    """[(key, array)] -> one flat float32 array (the fixture keeps a few large members, not hundreds of small ones)"""
    return np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1) for _, a in named]) if named else np.zeros(0, np.float32)


def unpack(flat, keys, shapes):
    out, o = {}, 0
    for k in keys:
        n = int(np.prod(shapes[k]))
        out[k] = np.asarray(flat[o:o + n]).reshape(shapes[k])
        o += n
    assert o == flat.size
    return out


def fixture_variant(z, tag):
    """(keys in state-dict order, shapes, stored weights, stored gradients, gradient digests) of variant `tag`"""
    keys = [str(x) for x in z[tag + '.keys']]
    shapes = {k: tuple(int(x) for x in str(sh).split(',') if x) for k, sh in zip(keys, z[tag + '.shapes'])}
    small = [k for k in keys if not is_ff_weight(k)]
    big = [k for k in keys if is_ff_weight(k)]
    P = unpack(z[tag + '.P'], small, shapes)
    G = unpack(z[tag + '.grad'], small, shapes)
    dshape = lambda k: (FF_HIDDEN // 32, int(np.prod(shapes[k])) // FF_HIDDEN)      # noqa: E731
    ds = {k: dshape(k) for k in big}
    digests = (unpack(z[tag + '.grad_sum32'], big, ds), unpack(z[tag + '.grad_sub'], big, ds)) if big else ({}, {})
    return keys, shapes, P, G, digests


def load_weights(z, tag):
    """state dict (name -> float32 tensor, the fixture's key order) of variant `tag` from the open fixture `z`"""
    keys, shapes, P, _, _ = fixture_variant(z, tag)
    return {k: torch.from_numpy(ff_weight(tag, k, shapes[k]) if is_ff_weight(k) else P[k].copy()) for k in keys}


# --------------------------------------------------------------------------------------------------------------- the model
def _lin(P, pre, x):
    return x @ P[pre + '.weight'].t() + P[pre + '.bias']


def prepare(P, v, h, fc_feats, att_feats, att_masks, drop=None):
    """AoAModel._prepare_feature (AoAModel.py:207-226); v: the variant's opt"""
    if att_masks is not None:
        ml = int(att_masks.long().sum(1).max())
        att_feats, att_masks = att_feats[:, :ml], att_masks[:, :ml]
    x = _d(drop, 'att_embed', F.relu(_lin(P, 'att_embed.0', att_feats)))
    if att_masks is not None:
        x = x * att_masks.unsqueeze(-1)
    if v.refine:
        for i in range(6):
            pre = 'refiner.layers.%d' % i
            y = layer_norm(P, pre + '.sublayer.0.norm', x)
            q, k, val = (_lin(P, '%s.self_attn.linears.%d' % (pre, j), y) for j in range(3))
            a = dot_attention(q, k, val, att_masks, h, drop, 'ref%d' % i)
            if v.refine_aoa:
                a = F.glu(_lin(P, pre + '.self_attn.aoa_layer.0', _d(drop, 'ref%d.aoa' % i, torch.cat([a, y], -1))), -1)
            else:
                a = _lin(P, pre + '.self_attn.output_layer', a)
            x = x + _d(drop, 'ref%d.res' % i, a)
            if v.use_ff:
                y = layer_norm(P, pre + '.sublayer.1.norm', x)
                hid = _d(drop, 'ref%d.ff' % i, F.relu(_lin(P, pre + '.feed_forward.w_1', y)))
                x = x + _d(drop, 'ref%d.res2' % i, _lin(P, pre + '.feed_forward.w_2', hid))
        x = layer_norm(P, 'refiner.norm', x)
    if v.mean_feats:
        mean = x.mean(1) if att_masks is None else (x * att_masks.unsqueeze(-1)).sum(1) / att_masks.unsqueeze(-1).sum(1)
    else:
        mean = _d(drop, 'fc_embed', F.relu(_lin(P, 'fc_embed.0', fc_feats)))
    return mean, _lin(P, 'ctx2att', x), att_masks


def _cell(P, pre, x, hc):
    gates = x @ P[pre + '.weight_ih'].t() + P[pre + '.bias_ih'] + hc[0] @ P[pre + '.weight_hh'].t() + P[pre + '.bias_hh']
    i, f, g, o = gates.chunk(4, 1)
    c = torch.sigmoid(f) * hc[1] + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def step(P, v, h, it, mean, p_att, att_masks, state, drop=None, t=0, ctx_mask=True):
    """AoA_Decoder_Core.forward (AoAModel.py:163-186) + the logit; ctx_mask False: never ask for the ctx<t> mask"""
    hs, cs = state
    R = mean.shape[1]
    xt = _d(drop, 'xt%d' % t, F.relu(P['embed.0.weight'][it]))
    ctx = _d(drop, 'ctx%d' % t, hs[1]) if (v.ctx_drop and ctx_mask) else hs[1]
    h_att, c_att = _cell(P, 'core.att_lstm', torch.cat([xt, mean + ctx], 1), (hs[0], cs[0]))
    q = _lin(P, 'core.attention.linears.0', layer_norm(P, 'core.attention.norm', h_att))
    att = dot_attention(q.unsqueeze(1), p_att[:, :, R:], p_att[:, :, :R], att_masks, h, drop, 'dec%d' % t).squeeze(1)
    x = torch.cat([att, h_att], 1)
    c_logic = cs[1]
    if v.decoder_type == 'AoA':
        out = F.glu(_lin(P, 'core.att2ctx.0', x), -1)
    elif v.decoder_type == 'LSTM':
        out, c_logic = _cell(P, 'core.att2ctx', x, (hs[1], cs[1]))
    else:
        out = F.relu(_lin(P, 'core.att2ctx.0', x))
    state = (torch.stack([h_att, out]), torch.stack([c_att, c_logic]))
    if v.out_res:
        out = out + h_att
    return F.log_softmax(_lin(P, 'logit', _d(drop, 'out%d' % t, out)), 1), state


def forward_teacher(P, v, h, fc_feats, att_feats, seq, att_masks, drop=None, ctx_mask=True):
    """AttModel._forward (AttModel.py:126-164): seq [B,n,T] or [N,T] -> log-probs [N,T,V1]"""
    if seq.ndim == 3:
        seq = seq.reshape(-1, seq.shape[2])
    B = att_feats.shape[0]
    N, T = seq.shape
    n = N // B
    mean, p_att, masks = prepare(P, v, h, fc_feats, att_feats, att_masks, drop)
    if n > 1:
        mean, p_att = mean.repeat_interleave(n, 0), p_att.repeat_interleave(n, 0)
        masks = None if masks is None else masks.repeat_interleave(n, 0)
    R = mean.shape[1]
    state = (mean.new_zeros(2, N, R), mean.new_zeros(2, N, R))
    out = mean.new_zeros(N, T, P['logit.weight'].shape[0])
    for t in range(T):
        if t >= 1 and int(seq[:, t].sum()) == 0:
            break
        logp, state = step(P, v, h, seq[:, t], mean, p_att, masks, state, drop, t, ctx_mask)
        out[:, t] = logp
    return out


def lm_criterion(logp, target, mask):
    """LanguageModelCriterion (losses.py): masked mean of the negative log-prob of the target tokens"""
    N, T = logp.shape[:2]
    target, mask = target.reshape(N, -1)[:, :T], mask.reshape(N, -1)[:, :T].to(logp)
    return -(logp.gather(2, target.unsqueeze(2)).squeeze(2) * mask).sum() / mask.sum()
