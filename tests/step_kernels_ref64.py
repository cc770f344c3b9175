"""Float64 restatements, on the CPU, of the per-step kernels (LSTM / maxout / att2in2 / adaatt cells, additive attention forward,
backward and time-batched pass, the same three for AdaAtt's sentinel attention) plus the case tables and input builders that test_step_kernels_host.py and
test_step_kernels_gpu.py share.  Nothing of the package is imported here: the operand semantics are those of include/capmi.h and of
the Python models (AttModel.py, NewFCModel.py, Att2in2Model.py, AdaAttModel.py); backward is torch.autograd on the forward."""
import torch

F64 = torch.float64

# one row of every cell case carries these pre-activations (saturation on both sides, signed zeros, the flush-to-zero range of exp)
EXTREMES = (0.0, -0.0, 1e-6, -1e-6, 15.0, -15.0, 90.0, -90.0, 1e4, -1e4)
# element j of gate `g` of the planted row holds EXTREMES[(j + OFF[g]) % 10].  The two maxout chunks sit 4 apart, so no pair of
# them is closer than 15 (no planted near-tie); the input gate shares the offset of the second chunk, so the one combination whose
# float32 SAVED activation cannot carry the product (sigmoid(+-15) saved to 6e-8 beside a candidate of 1e4) does not occur.
OFF = {'in': 8, 'f': 2, 'out': 6, 'cand': 4, 'cand_b': 8, 'sent': 0}
TIE = 1e-4          # maxout chunks closer than this (float64) are left out of the d_sums[3], d_sums[4] comparison
TIE_CAP = 0.01      # ... at most this share of a case's elements


def d64(t):
    return None if t is None else t.detach().to(F64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def extremes_row(R, gates):
    e = torch.tensor(EXTREMES, dtype=F64)
    j = torch.arange(R)
    return torch.cat([e[(j + OFF[g]) % len(EXTREMES)] for g in gates])


def plant_row(N):
    return N // 2


# ------------------------------------------------------------------------------------------------ summed inputs
def presum(N, width, slab_sets=(), addend=None, biases=(), row_bias=None, row_idx=None, row_div=1, fc_gates=None, n=1):
    """sum of every operand of a cell's pre-activations [N, width]: slab lists ([S, N, w] each, w <= width columns starting at
    `col0`), addend, bias vectors, row_bias[row_idx[r]] (or r // row_div), fc_gates[r // n]"""
    pre = torch.zeros(N, width, dtype=F64)
    for slabs, col0 in slab_sets:
        if slabs is not None:
            pre[:, col0:col0 + slabs.shape[2]] += d64(slabs).sum(0)
    if addend is not None:
        pre = pre + d64(addend)
    for b, col0 in biases:
        if b is not None:
            pre[:, col0:col0 + b.numel()] += d64(b)
    if row_bias is not None:
        idx = row_idx.long() if row_idx is not None else torch.arange(N) // row_div
        pre = pre + d64(row_bias)[idx]
    if fc_gates is not None:
        pre = pre + d64(fc_gates)[torch.arange(N) // n]
    return pre


# ------------------------------------------------------------------------------------------------ pointwise maths, once per cell
def lstm_point(pre, c_prev):
    """torch.nn.LSTMCell gate maths, gate order i, f, g, o -> h, c, activated gates"""
    i, f, g, o = pre.chunk(4, 1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return o * torch.tanh(c), c, torch.cat([i, f, g, o], 1)


def maxout_point(pre, c_prev):
    """LSTMCore / Att2in2Core: (in, forget, out, cand_a, cand_b) -> h, c, saved = (sig, sig, sig, cand_a, cand_b)"""
    R = c_prev.shape[1]
    i, f, o = (torch.sigmoid(pre[:, q * R:(q + 1) * R]) for q in range(3))
    ca, cb = pre[:, 3 * R:4 * R], pre[:, 4 * R:5 * R]
    c = f * c_prev + i * torch.max(ca, cb)
    return o * torch.tanh(c), c, torch.cat([i, f, o, ca, cb], 1)


def adaatt_point(pre, c_prev, maxout):
    """AdaAtt_lstm: (in, forget, out, candidate | the two maxout chunks, sentinel gate) -> h, c, fake_region, saved"""
    R = c_prev.shape[1]
    i, f, o = (torch.sigmoid(pre[:, q * R:(q + 1) * R]) for q in range(3))
    if maxout:
        ca, cb = pre[:, 3 * R:4 * R], pre[:, 4 * R:5 * R]
        cand, keep = torch.max(ca, cb), [ca, cb]
    else:
        cand = torch.tanh(pre[:, 3 * R:4 * R])
        keep = [cand]
    s = torch.sigmoid(pre[:, -R:])
    c = f * c_prev + i * cand
    tc = torch.tanh(c)
    return o * tc, c, s * tc, torch.cat([i, f, o] + keep + [s], 1)


def cell_backward(point, pre, c_prev, dh, dc_next, dfake=None):
    """autograd through `point`: gradients w.r.t. the pre-activations and c_prev"""
    pre = pre.clone().requires_grad_(True)
    cp = c_prev.clone().requires_grad_(True)
    out = point(pre, cp)
    loss = (out[0] * dh).sum()
    if dc_next is not None:
        loss = loss + (out[1] * dc_next).sum()
    if dfake is not None:
        loss = loss + (out[2] * dfake).sum()
    loss.backward()
    return pre.grad, cp.grad


def tie_mask(pre, R):
    """elements of the two maxout chunks that are too close to say which one the gradient belongs to"""
    return (pre[:, 3 * R:4 * R] - pre[:, 4 * R:5 * R]).abs() < TIE


# ------------------------------------------------------------------------------------------------ cell inputs
def _flags(s):
    return set(s.split())


def cell_inputs(kind, N, R, splits, splits2, flags, seed):
    """float32 operands of one cell case (kind: 'lstm', 'maxout' (also att2in2), 'adaatt', 'adaattmo') and their float64 sum.
    Pre-activations have standard deviation 3; row plant_row(N) is set to the EXTREMES pattern through slab 0."""
    fl = _flags(flags)
    g = gen(seed)
    gates = {'lstm': ('in', 'f', 'cand', 'out'), 'maxout': ('in', 'f', 'out', 'cand', 'cand_b'),
             'adaatt': ('in', 'f', 'out', 'cand', 'sent'), 'adaattmo': ('in', 'f', 'out', 'cand', 'cand_b', 'sent')}[kind]
    W = len(gates) * R
    has2 = splits2 > 0
    W2 = W if kind == 'lstm' else 2 * R                   # lstm: a second slab list of full width; att2in2: the a2c product
    col2 = 0 if kind == 'lstm' else 3 * R
    terms = splits + splits2 + sum(k in fl for k in ('bih', 'bhh', 'rbdiv', 'rbidx', 'addend', 'ba2c', 'fc'))
    sd = 3.0 / terms ** 0.5                               # the sum of `terms` independent draws has standard deviation 3
    rnd = lambda *s: (torch.randn(*s, generator=g) * sd).float()       # noqa: E731
    d = {'partial': rnd(splits, N, W), 'partial2': rnd(splits2, N, W2) if has2 else None,
         'b1': rnd(W) if 'bih' in fl else None, 'b2': rnd(W) if 'bhh' in fl else None,
         'addend': rnd(N, W) if 'addend' in fl else None, 'ba2c': rnd(2 * R) if 'ba2c' in fl else None,
         'row_bias': None, 'row_idx': None, 'row_div': 1, 'fc_gates': None, 'n': 1}
    if 'rbdiv' in fl:
        d['row_div'] = 5
        d['row_bias'] = rnd((N + 4) // 5, W)
    if 'rbidx' in fl:
        rows = max(2, N // 3)
        d['row_bias'] = rnd(rows, W)
        d['row_idx'] = torch.randint(0, rows, (N,), generator=g).int()
    if 'fc' in fl:
        d['n'] = 5 if N % 5 == 0 else 1
        d['fc_gates'] = rnd(N // d['n'], W)
    d['c_prev'] = torch.randn(N, R, generator=g).float()
    d['mask'] = ((torch.rand(N, R, generator=g) < 0.5).float() * 2) if 'mask' in fl else None
    d['mask2'] = ((torch.rand(N, R, generator=g) < 0.5).float() * 2) if 'mask2' in fl else None

    def total():
        return presum(N, W, [(d['partial'], 0), (d['partial2'], col2)], d['addend'], [(d['b1'], 0), (d['b2'], 0), (d['ba2c'], 3 * R)],
                      d['row_bias'], d['row_idx'], d['row_div'], d['fc_gates'], d['n'])

    p = plant_row(N)
    d['partial'][0, p] = (d['partial'][0, p].double() + extremes_row(R, gates) - total()[p]).float()
    d['pre'] = total()
    d['gates'], d['W'], d['plant'] = gates, W, p
    return d


# ------------------------------------------------------------------------------------------------ attention
def attention_fwd(att_h, p_att, att, mask, w, b, img):
    """Attention.forward (AttModel.py:728-748) for rows whose image is img[r]: alpha [N,K], ctx [N,R], scores e [N,K]"""
    e = torch.tanh(p_att[img] + att_h.unsqueeze(1)) @ w + b
    al = torch.softmax(e, 1)
    if mask is not None:
        al = al * mask[img]
        al = al / al.sum(1, keepdim=True)
    return (al.unsqueeze(2) * att[img]).sum(1), al, e


def attention_case(B, n, K, A, R, h_splits, flags, seed, d_ctx=None):
    """float32 operands of one attention case + float64 forward and backward (autograd)"""
    fl = _flags(flags)
    g = gen(seed)
    N = B * n
    img = torch.randint(0, B, (N,), generator=g) if 'rowimg' in fl else torch.arange(N) // n      # rowimg: shuffled, repeating
    S = max(h_splits, 1)
    h_pad = 3 if 'hodd' in fl else (8 if 'hpad' in fl else 0)     # slab stride N*A + pad floats
    d = {'N': N, 'img': img, 'h_pad': h_pad,
         'h_slabs': (torch.randn(S, N * A + h_pad, generator=g) / S ** 0.5).float(),
         'h_bias': torch.randn(A, generator=g).float() if h_splits > 0 else None,
         'p_att': torch.randn(B, K, A, generator=g).float(), 'att': torch.randn(B, K, R, generator=g).float(),
         'w': (torch.randn(A, generator=g) * (2.0 / A ** 0.5)).float(), 'b': torch.randn(1, generator=g).float(), 'mask': None}
    if 'mask' in fl:
        lens = torch.randint(1, K + 1, (B,), generator=g)
        lens[0] = 1                                           # an image with ONE unmasked region
        lens[B - 1] = K
        d['mask'] = (torch.arange(K).unsqueeze(0) < lens.unsqueeze(1)).float()
    att_h = d64(d['h_slabs'])[:, :N * A].sum(0).view(N, A)
    if d['h_bias'] is not None:
        att_h = att_h + d64(d['h_bias'])
    ah = att_h.clone().requires_grad_(True)
    ctx, al, e = attention_fwd(ah, d64(d['p_att']), d64(d['att']), d64(d['mask']), d64(d['w']), d64(d['b']), img)
    e.retain_grad()
    d['d_ctx'] = torch.randn(N, R, generator=g).float() if d_ctx is None else d_ctx       # (given: float64, e.g. a slab sum)
    (ctx * d64(d['d_ctx'])).sum().backward()
    d.update(att_h=att_h, ctx=ctx.detach(), alpha=al.detach(), d_att_h=ah.grad, d_e=e.grad)
    return d


def attention_batched(d_ctx, att_h, alpha, d_e, p_att, w, B, n):
    """the time-batched pass over [T, N_stride, .] buffers, rows >= B*n of a slab ignored (include/capmi.h)"""
    T = d_ctx.shape[0]
    live = B * n
    dc, ah, al, de = (d64(t)[:, :live].reshape(T, B, n, -1) for t in (d_ctx, att_h, alpha, d_e))
    d_att = torch.einsum('tbnk,tbnr->bkr', al, dc)
    th = torch.tanh(d64(p_att).view(1, B, 1, *p_att.shape[1:]) + ah.unsqueeze(3))      # [T,B,n,K,A]
    d_p_att = torch.einsum('tbnk,tbnka->bka', de, 1 - th * th) * d64(w)
    dw_rows = torch.einsum('tbnk,tbnka->bka', de, th)                                 # one row per (image, region)
    return d_att, d_p_att, dw_rows.sum((0, 1)), de.sum().view(1), dw_rows


# ------------------------------------------------------------------------------------------------ case tables
# LSTM forward: (N, R, splits, splits2, flags, branch it is meant to reach).  splits + splits2 lands on, below and above a multiple
# of 8 (the 8-at-a-time trip of both kernels); R % 4 == 0 and every operand 16-byte aligned -> lstm_cell_fwd_vec_kernel, any
# other -> lstm_cell_fwd_kernel.  'off:X' hands operand X in from a view one float off a 16-byte boundary.
LSTM_FWD = [
    (7, 36, 1, 0, 'bih bhh mask', 'vec, one slab: the clamped index is 0 for all 8 loads of the trip'),
    (7, 36, 3, 0, 'bih rbdiv', 'vec, partly filled single trip; row_bias by r // 5'),
    (64, 36, 8, 0, 'bhh rbidx mask planes', 'vec, exactly one full trip; row_bias through a shuffled index; planes of h, h_drop'),
    (65, 4, 9, 0, 'bih bhh', 'vec, one slab into the second trip; R = 4: one quad per row, N * R/4 = 65 threads: two workgroups'),
    (7, 260, 17, 0, 'rbidx mask noga', 'vec, third trip of one slab; gates_act NULL'),
    (1, 36, 1, 1, 'bih', 'vec, the second list supplies the last slab of the trip (si >= splits switch)'),
    (64, 4, 3, 1, 'bhh mask planes', 'vec, 4 slabs across both lists'),
    (7, 36, 8, 1, 'bih bhh rbdiv', 'vec, 9 = full trip from list 1, second trip entirely from list 2'),
    (7, 36, 9, 1, 'mask', 'vec, no bias at all; 10 slabs'),
    (7, 36, 17, 1, 'bih rbidx', 'vec, 18 slabs: three trips'),
    (7, 36, 1, 5, 'bhh', 'vec, list 2 longer than list 1'),
    (65, 36, 3, 5, 'bih bhh rbidx mask', 'vec, 3 + 5 = 8: the lists meet inside ONE full trip'),
    (7, 260, 8, 5, 'rbdiv', 'vec, 13 slabs'),
    (1, 4, 9, 5, 'bih mask', 'vec, 14 slabs, a single quad'),
    (7, 36, 17, 5, 'bih bhh rbdiv mask', 'vec, 22 slabs'),
    (7, 33, 3, 1, 'bih bhh rbidx mask planes', 'scalar: R % 4 != 0; planes by pl_store1'),
    (65, 33, 9, 5, 'bih rbdiv', 'scalar, grid-stride over 65 * 33 elements, second trip partly filled'),
    (7, 33, 17, 0, 'bhh mask noga', 'scalar, 17 slabs, gates_act NULL'),
    (7, 36, 3, 1, 'bih bhh rbidx mask off:partial', 'scalar through the alignment fallback: slabs one float off'),
    (7, 36, 9, 0, 'bih bhh rbdiv mask off:c_prev', 'scalar through the alignment fallback: c_prev one float off'),
    (64, 36, 8, 5, 'bih mask planes off:b1', 'scalar through the alignment fallback (bias one float off), planes still wanted'),
]
# LSTM backward: (N, R, pad_a, mask_a, b, c, pad_bc, dc_next, flags, branch).  b / c: 0 = absent, k = k slabs; pad_bc: extra floats per
# slab row (ld = R + pad_bc) -- the slab stride is N * ld + 8 floats, larger than N * ld.
LSTM_BWD = [
    (7, 36, 0, False, 0, 0, 0, True, '', 'vec, dh_a alone, contiguous'),
    (7, 36, 8, True, 1, 0, 0, True, '', 'vec, dh_a a column slice of a wider matrix (ld_a = R + 8) through its dropout mask; dh_b plain'),
    (64, 36, 4, False, 3, 8, 4, False, 'planes', 'vec, 3 and 8 slabs (partly filled trip, exactly one trip), dc_next NULL, planes'),
    (65, 4, 0, True, 9, 3, 0, True, '', 'vec, 9 slabs: one into the second trip; two workgroups'),
    (1, 260, 0, False, 8, 9, 8, True, 'planes', 'vec, single row'),
    (7, 36, 0, False, 0, 9, 0, False, 'noa', 'vec, dh_a and dh_b NULL: dh from dh_c slabs only'),
    (7, 33, 3, True, 3, 9, 0, True, 'planes', 'scalar: R % 4 != 0'),
    (7, 36, 0, False, 3, 1, 1, True, '', 'scalar: ld_b = ld_c = 37, not a multiple of 4'),
    (65, 36, 0, True, 9, 8, 0, False, 'off:dh_b', 'scalar through the alignment fallback: dh_b one float off'),
]
# maxout / att2in2 forward: (N, R, splits, splits2, flags, branch).  slab_sum walks 4 slabs at a time.
MAXOUT_FWD = [
    (7, 33, 1, 0, 'bih bhh mask', 'maxout entry point: one slab, partly filled group of 4'),
    (64, 36, 4, 0, 'bih', 'maxout entry point: exactly one group'),
    (65, 4, 5, 0, 'bhh mask', 'maxout entry point: one slab into the second group'),
    (1, 260, 9, 0, 'bih bhh', 'maxout entry point: third group'),
    (7, 33, 1, 1, 'bih bhh ba2c addend mask', 'att2in2: a2c slabs + b_a2c on the candidate half, addend'),
    (7, 36, 4, 6, 'bih ba2c', 'att2in2: 6 a2c slabs (second group partly filled)'),
    (65, 33, 5, 1, 'addend mask', 'att2in2: no bias at all'),
    (64, 4, 9, 6, 'bih bhh addend', 'att2in2: a2c slabs WITHOUT b_a2c'),
    (7, 36, 5, 0, 'bih bhh ba2c mask', 'att2in2: b_a2c WITHOUT a2c slabs (splits2 = 0, partial2 NULL)'),
]
# maxout / att2in2 backward: (N, R, b_splits (0: dh_b NULL), mask_a, dc_next, entry, branch)
MAXOUT_BWD = [
    (7, 33, 0, False, True, 'att2in2', 'dh_a alone'),
    (64, 36, 1, True, True, 'maxout', 'maxout entry point: dh_b one finished buffer'),
    (65, 4, 1, False, False, 'att2in2', 'one slab at a stride larger than N * R, dc_next NULL'),
    (7, 260, 3, True, True, 'att2in2', 'three slabs at a stride larger than N * R'),
    (1, 36, 3, False, True, 'att2in2', 'single row: the planted row is the whole case'),
]
# adaatt forward / backward: (N, R, maxout, splits, flags, branch)
ADAATT = [
    (7, 33, 0, 1, 'fc mask mask2 addend', 'tanh candidate (5 blocks), fc_gates per row (n = 1), both dropout masks'),
    (65, 36, 0, 5, 'fc', 'tanh candidate, fc_gates row r // 5, no masks'),
    (64, 4, 1, 4, 'fc mask addend', 'maxout candidate (6 blocks), n = 1'),
    (1, 260, 1, 9, 'mask2', 'maxout candidate, no fc_gates, fake-region mask only'),
    (65, 33, 1, 1, 'fc mask mask2', 'maxout candidate, fc_gates row r // 5'),
]

# attention forward: (B, n, K, A, R, h_splits, flags, branch).  "v2<NR,CS>": attention_fwd_v2_kernel with NR rows per workgroup
# and CS column splits; "stream": attention_fwd_kernel.  The dispatcher also declares v2<1,2>, v2<2,2> and v2<2,4>; none can be
# reached.  CS = 2 is chosen only when the column-split request is 2, and the product build fixes the request at 4.  CS = 4 is
# granted while 4 * workgroups <= 256, i.e. at most 64 workgroups, which at two rows each hold at most 128 rows -- but two rows
# per workgroup are chosen only for more than 256 rows.
ATT_FWD = [
    (3, 2, 7, 12, 36, 0, '', 'v2<1,4>: finished att_h rows, no slabs'),
    (3, 2, 7, 12, 36, 1, 'hpad', 'v2<1,4>: one slab + h_bias + att_h_out'),
    (3, 2, 7, 12, 36, 3, 'hpad', 'v2<1,4>: 3 slabs, one per slab group, the fourth group empty'),
    (3, 2, 7, 12, 36, 16, '', 'v2<1,4>: 16 slabs, four per group: the most the registers hold'),
    (3, 2, 7, 12, 36, 17, '', 'stream: h_splits > 16; third 8-slab trip of one'),
    (3, 2, 7, 12, 36, 3, 'hodd', 'stream: h_stride % 4 != 0'),
    (2, 3, 1, 12, 36, 3, '', 'v2<1,4>: K = 1, every region index clamps to 0'),
    (2, 3, 36, 12, 36, 0, '', 'v2<1,4>: K = 36'),
    (2, 3, 40, 12, 36, 3, '', 'v2<1,4>: K = 40 = V2_KMAX, all five score regions of every wave live'),
    (2, 3, 41, 12, 36, 3, '', 'stream: K > 40'),
    (3, 2, 7, 4, 36, 3, '', 'v2<1,4>: A = 4, one 16-byte piece, both lane halves clamp'),
    (3, 2, 7, 512, 36, 3, '', 'v2<1,4>: A = 512, the widest'),
    (3, 2, 7, 516, 36, 3, '', 'stream: A > 512, scalar score loop'),
    (3, 2, 7, 12, 4, 3, '', 'v2<1,4>: R = 4, one quad: column splits 1..3 own nothing'),
    (3, 2, 7, 12, 1000, 3, '', 'v2<1,4>: R = 1000, 250 quads in shares of 63'),
    (3, 2, 7, 12, 1024, 3, '', 'v2<1,4>: R = 1024, the widest'),
    (3, 2, 7, 12, 1028, 3, '', 'stream: R > 1024, scalar context loop'),
    (64, 1, 7, 12, 36, 3, '', 'v2<1,4>: 64 workgroups x 4 column splits = 256, the last shape with four'),
    (65, 1, 7, 12, 36, 3, '', 'v2<1,1>: 72 workgroups, 4 splits would pass 256'),
    (52, 5, 7, 12, 36, 3, '', 'v2<2,1>: 260 rows, two per workgroup, ragged last chunk (2, 2, 1)'),
    (33, 8, 7, 12, 36, 0, '', 'v2<2,1>: 264 rows, four full chunks per image, finished att_h'),
    (257, 1, 7, 12, 36, 3, '', 'stream: 264 workgroups > 256'),
    (4, 3, 7, 12, 36, 3, 'rowimg', 'v2<1,4>: row_img, shuffled repeating image index, one row per workgroup'),
    (4, 3, 41, 12, 36, 0, 'rowimg', 'stream: row_img'),
    (5, 2, 36, 512, 1000, 2, 'mask', 'v2<1,4> at the configured sizes: ragged mask, one image with a single unmasked region'),
    (5, 2, 9, 12, 36, 3, 'mask', 'v2<1,4>: mask, small'),
    (3, 2, 9, 20, 31, 3, 'mask', 'stream: R % 4 != 0, mask'),
    (3, 2, 7, 12, 36, 3, 'off:p_att', 'stream through the alignment fallback: p_att one float off (scalar score loop)'),
    (3, 2, 7, 12, 36, 3, 'off:att', 'stream through the alignment fallback: att one float off (scalar context loop)'),
]

# attention backward: (B, n, K, A, R, x_splits (0: capmi_attention_bwd), extra, flags, branch); extra = ld_dctx - R or x_cols - R
ATT_BWD = [
    (3, 2, 7, 12, 36, 0, 8, '', 'bwd_v2, d_ctx a column slice (ld_dctx = R + 8)'),
    (3, 2, 9, 20, 31, 0, 5, 'mask', 'stream (R % 4 != 0), ld_dctx = R + 5, masked forward'),
    (3, 2, 7, 12, 36, 1, 0, '', 'bwd_v2, one slab, x_cols = R: one role'),
    (3, 2, 7, 12, 36, 3, 8, '', 'bwd_v2, 3 slabs, x_cols = R + 8: two roles'),
    (3, 2, 7, 12, 36, 9, 2052, '', 'bwd_v2, 9 slabs, x_cols = R + 2052: four roles, 513 quads in shares of 171'),
    (3, 2, 7, 12, 33, 3, 2, '', 'x_cols = 35: reduce launch, then the streaming kernel on the finished rows'),
    (103, 5, 7, 12, 36, 3, 8, '', 'stream: 515 rows, two per workgroup, ragged last chunk; slabs finished in the kernel'),
    (2, 3, 41, 12, 36, 3, 8, '', 'stream: K > 40'),
    (2, 3, 7, 12, 1028, 9, 8, '', 'stream: R > 1024'),
    (2, 3, 40, 512, 1024, 3, 8, '', 'bwd_v2 at its widest: K = 40, A = 512, R = 1024'),
    (4, 3, 7, 12, 36, 3, 8, 'rowimg', 'bwd_v2, row_img'),
]
# batched pass: (T, B, n, K, A, R, pad rows per slab, branch)
ATT_BATCHED = [
    (1, 3, 2, 11, 12, 127, 0, 'one region chunk, partly filled; R below one column block'),
    (3, 3, 2, 12, 12, 128, 0, 'T = 3; exactly one chunk of 12 and one column block of 128'),
    (3, 2, 3, 13, 20, 129, 4, 'two chunks, two column blocks; N_stride = B * n + 4: the rows of another rollout between the steps'),
    (1, 128, 1, 13, 12, 36, 0, 'B * ceil(K / 4) = 512 workgroups: attn_dpatt_kernel<4>, last region group holds one'),
]


def cell_rows():
    """every cell case row of the GPU tests as (kind, N, R, splits, splits2, flags, seed), with the seed the GPU test draws it by
    (the backward rows draw their pre-activations as one slab + one bias)"""
    rows = [('lstm',) + c[:5] + (i,) for i, c in enumerate(LSTM_FWD)]
    rows += [('lstm', c[0], c[1], 1, 0, 'bih', 50 + i) for i, c in enumerate(LSTM_BWD)]
    rows += [r for r in maxout_rows() if r[0] == 'maxout']
    rows += [('adaattmo' if c[2] else 'adaatt', c[0], c[1], c[3], 0, c[4], 300 + i) for i, c in enumerate(ADAATT)]
    return rows


def maxout_rows():
    """every case row with a maxout candidate as (kind, N, R, splits, splits2, flags, seed): the inputs the GPU tests draw, so that
    the host test can hold the tie cap for each of them (the backward rows draw their pre-activations as one slab + one bias)"""
    rows = [('maxout',) + c[:5] + (100 + i,) for i, c in enumerate(MAXOUT_FWD)]
    rows += [('maxout', c[0], c[1], 1, 0, 'bih', 200 + i) for i, c in enumerate(MAXOUT_BWD)]
    rows += [('adaattmo', c[0], c[1], c[3], 0, c[4], 300 + i) for i, c in enumerate(ADAATT) if c[2]]
    return rows


# ------------------------------------------------------------------------------------------------ sentinel attention (AdaAtt)
def sentinel_fwd(fre, hoe, fr, ho, p_att, att, mask, w, b, tile, img):
    """AdaAtt_attention.forward (AttModel.py:565-602) from the two projections fr_e / ho_e on, for rows whose image is img[r]:
    pi [M,K+1] (sentinel first), ctx [M,R] (residual ho included), scores e [M,K+1], the dropped tanh tile hA [M,K+1,A]"""
    hA = torch.tanh(torch.cat([fre.unsqueeze(1), p_att[img]], 1) + hoe.unsqueeze(1))
    if tile is not None:
        hA = hA * tile
    e = hA @ w + b
    pi = torch.softmax(e, 1)
    if mask is not None:
        m = mask[img]
        pi = pi * torch.cat([m[:, :1], m], 1)                 # the sentinel takes the mask of region 0
        pi = pi / pi.sum(1, keepdim=True)
    ctx = (pi.unsqueeze(2) * torch.cat([fr.unsqueeze(1), att[img]], 1)).sum(1) + ho
    return pi, ctx, e, hA


def sentinel_case(T, B, n, K, A, R, fre_splits, hoe_splits, flags, seed):
    """float32 operands of one sentinel-attention case over T steps of N = B * n image-major rows + the float64 forward, its autograd
    backward and the time-batched results.  fre / hoe come as `splits` slabs [S, T*N*A + pad] (+ bias) or, with splits == 0, as one
    finished buffer (slab 0).  flags: mask, tile, hpad, hodd, nobias; noout and off:X only concern the caller."""
    fl = _flags(flags)
    g = gen(seed)
    N, K1 = B * n, K + 1
    M = T * N
    img = (torch.arange(M) % N) // n
    pad = 3 if 'hodd' in fl else (8 if 'hpad' in fl else 0)
    rnd = lambda *s: torch.randn(*s, generator=g).float()       # noqa: E731
    d = {'N': N, 'img': img, 'fre_stride': M * A + pad, 'hoe_stride': M * A + pad}
    for k, s in (('fre', fre_splits), ('hoe', hoe_splits)):
        S_ = max(s, 1)
        d[k + '_slabs'] = (torch.randn(S_, M * A + pad, generator=g) / S_ ** 0.5).float()
        d[k + '_bias'] = rnd(A) if (s > 0 and 'nobias' not in fl) else None
    d.update(fr=rnd(T, N, R), ho=rnd(T, N, R), p_att=rnd(B, K, A), att=rnd(B, K, R),
             w=(torch.randn(A, generator=g) * (2.0 / A ** 0.5)).float(), b=rnd(1), d_ctx=rnd(T, N, R), mask=None, tile=None)
    if 'mask' in fl:
        lens = torch.randint(1, K + 1, (B,), generator=g)
        lens[0] = 1                                           # an image with ONE unmasked region
        lens[B - 1] = K
        d['mask'] = (torch.arange(K).unsqueeze(0) < lens.unsqueeze(1)).float()
    if 'tile' in fl:
        d['tile'] = (torch.rand(T, N, K1, A, generator=g) < 0.5).float() * 2
    x = {}
    for k in ('fre', 'hoe'):
        v = d64(d[k + '_slabs'])[:, :M * A].sum(0).view(M, A)
        if d[k + '_bias'] is not None:
            v = v + d64(d[k + '_bias'])
        x[k] = v
    x.update(fr=d64(d['fr']).view(M, R), p_att=d64(d['p_att']), att=d64(d['att']), w=d64(d['w']), b=d64(d['b']))
    ref_in = {k: v.clone() for k, v in x.items()}
    x = {k: v.requires_grad_(True) for k, v in x.items()}
    tile = None if d['tile'] is None else d64(d['tile']).view(M, K1, A)
    pi, ctx, e, hA = sentinel_fwd(x['fre'], x['hoe'], x['fr'], d64(d['ho']).view(M, R), x['p_att'], x['att'], d64(d['mask']), x['w'],
                                  x['b'], tile, img)
    e.retain_grad()
    (ctx * d64(d['d_ctx']).view(M, R)).sum().backward()
    # alpha_net's weight gradient, one row per (image, score row): what dw_partial receives
    dw_rows = torch.einsum('tbnk,tbnka->bka', e.grad.view(T, B, n, K1), hA.detach().view(T, B, n, K1, A))
    d.update(fre=ref_in['fre'].view(T, N, A), hoe=ref_in['hoe'].view(T, N, A), pi=pi.detach().view(T, N, K1),
             ctx=ctx.detach().view(T, N, R), d_e=e.grad.view(T, N, K1), d_hoe=x['hoe'].grad.view(T, N, A),
             d_fre=x['fre'].grad.view(T, N, A), d_fr=x['fr'].grad.view(T, N, R), d_att=x['att'].grad, d_p_att=x['p_att'].grad,
             dw_rows=dw_rows, d_w=x['w'].grad, d_b=x['b'].grad)
    return d


# The last column of a sentinel row names its arm twice: `key=value` tokens, which test_step_kernels_host.py recomputes from the
# row with a mirror of the dispatcher's arithmetic, then ' | ' and words.  Forward keys: rpb (rows per workgroup), ragged (last chunk
# of an image shorter: 0/1), padwg (B % 8 != 0: padding workgroups), vecA / vecR (16-byte score / context arm), G (region groups of
# the context phase), idle (threads of the 512 outside the G * R/4 working ones), trips (trips of G * 6 regions a group makes),
# passes (score passes of 8 waves x 4 rows), lanes (softmax entries per lane), ftrips / htrips (8-slab trips of fr_e / ho_e).
# forward: (B, n, K, A, R, fre_splits, hoe_splits, flags, arm), one step
SENT_FWD = [
    (3, 2, 7, 12, 36, 0, 0, '', 'ftrips=0 htrips=0 rpb=1 padwg=1 vecA=1 vecR=1 G=4 | both projections finished, copied to fre_out / hoe_out'),
    (3, 2, 7, 12, 36, 1, 1, '', 'ftrips=1 htrips=1 G=4 trips=1 passes=1 lanes=1 | the product shape: one slab each + bias + rows out'),
    (3, 2, 7, 12, 36, 3, 3, 'hpad', 'ftrips=1 htrips=1 | 3 slabs, partly filled trip, slab stride N * A + 8'),
    (3, 2, 7, 12, 36, 8, 8, '', 'ftrips=1 htrips=1 | 8 slabs: exactly one trip'),
    (3, 2, 7, 12, 36, 9, 9, '', 'ftrips=2 htrips=2 | 9 slabs: one into the second trip'),
    (3, 2, 7, 12, 36, 17, 17, '', 'ftrips=3 htrips=3 | 17 slabs: third trip'),
    (3, 2, 7, 12, 36, 3, 9, '', 'ftrips=1 htrips=2 | the two operands at different slab counts'),
    (3, 2, 7, 12, 36, 0, 3, '', 'ftrips=0 htrips=1 | fr_e finished, ho_e as slabs'),
    (3, 2, 7, 12, 36, 8, 0, '', 'ftrips=1 htrips=0 | fr_e as slabs, ho_e finished'),
    (3, 2, 7, 12, 36, 3, 3, 'hodd', 'ftrips=1 vecA=1 | slab stride N * A + 3: the slab loads are scalar, the score arm stays 16-byte'),
    (3, 2, 7, 12, 36, 3, 1, 'nobias', 'ftrips=1 htrips=1 | slabs without biases'),
    (3, 2, 7, 12, 36, 3, 3, 'noout', 'ftrips=1 htrips=1 | fre_out / hoe_out NULL'),
    (3, 2, 7, 10, 36, 1, 1, '', 'vecA=0 vecR=1 | A % 4 != 0: scalar score loop'),
    (3, 2, 7, 12, 36, 1, 1, 'off:p_att', 'vecA=0 vecR=1 | p_att one float off'),
    (3, 2, 7, 12, 36, 1, 1, 'off:w', 'vecA=0 vecR=1 | w one float off'),
    (3, 2, 7, 12, 36, 1, 1, 'tile off:tile', 'vecA=0 vecR=1 | the tile mask one float off'),
    (3, 2, 7, 12, 31, 1, 1, '', 'vecA=1 vecR=0 G=1 | R % 4 != 0: scalar context loop'),
    (2, 3, 7, 12, 2052, 1, 1, '', 'vecA=1 vecR=0 G=1 | R > 2048: scalar context loop, five columns per thread'),
    (3, 2, 7, 12, 36, 1, 1, 'off:att', 'vecA=1 vecR=0 | att one float off'),
    (3, 2, 7, 12, 36, 1, 1, 'off:fr', 'vecA=1 vecR=0 | fr one float off'),
    (3, 2, 7, 12, 36, 1, 1, 'off:ho', 'vecA=1 vecR=0 | ho one float off'),
    (3, 2, 7, 12, 36, 1, 1, 'off:ctx', 'vecA=1 vecR=0 | ctx one float off'),
    (2, 3, 7, 12, 516, 1, 1, '', 'vecR=1 G=3 idle=125 | R = 516: 129 quads, three groups'),
    (2, 3, 7, 12, 1000, 1, 1, '', 'vecR=1 G=2 idle=12 | R = 1000, the configured width: 250 quads, two groups, 12 threads idle'),
    (2, 3, 7, 12, 2048, 1, 1, '', 'vecR=1 G=1 idle=0 | R = 2048: one group, no LDS partials'),
    (2, 3, 1, 12, 36, 1, 1, '', 'G=1 trips=1 | K = 1 clamps G to 1'),
    (2, 3, 2, 12, 36, 1, 1, '', 'G=2 trips=1 | K = 2 clamps G to 2'),
    (2, 3, 3, 12, 36, 1, 1, '', 'G=3 trips=1 | K = 3 clamps G to 3'),
    (103, 5, 7, 12, 36, 1, 1, '', 'rpb=3 ragged=1 G=2 padwg=1 | 515 rows: three per workgroup (3, 2), G = 2 by rows'),
    (2, 3, 24, 12, 36, 1, 1, '', 'G=4 trips=1 | K = 24 = G * 6: one full trip'),
    (2, 3, 25, 12, 36, 1, 1, '', 'G=4 trips=2 | K = 25: one region into the second trip'),
    (2, 3, 31, 12, 36, 1, 1, '', 'passes=1 lanes=1 | K + 1 = 32: one full score pass'),
    (2, 3, 32, 12, 36, 1, 1, '', 'passes=2 lanes=1 | K + 1 = 33: one score row into the second pass'),
    (2, 3, 64, 12, 36, 1, 1, '', 'passes=3 lanes=2 | K + 1 = 65: lane 0 takes two softmax entries'),
    (52, 5, 7, 12, 36, 1, 1, '', 'rpb=2 ragged=1 G=4 padwg=1 | 260 rows: two per workgroup, ragged last chunk (2, 2, 1)'),
    (225, 8, 7, 12, 36, 1, 1, '', 'rpb=8 ragged=0 G=2 padwg=1 | 1800 rows: NMAX = 8 per workgroup'),
    (16, 3, 7, 12, 36, 1, 1, '', 'rpb=1 padwg=0 | B a multiple of 8: no padding workgroup'),
    (5, 2, 9, 12, 36, 1, 1, 'mask', 'vecA=1 vecR=1 | mask, small: one image with a single unmasked region'),
    (5, 2, 36, 512, 512, 1, 1, 'mask', 'vecA=1 vecR=1 G=4 trips=2 passes=2 | mask at K = 36, A = 512, R = 512'),
    (3, 2, 7, 12, 36, 1, 1, 'tile', 'vecA=1 | tile drop through 16-byte mask loads'),
    (3, 2, 7, 10, 36, 1, 1, 'tile', 'vecA=0 | tile drop through scalar mask loads'),
    (52, 5, 7, 12, 36, 3, 3, 'tile mask', 'rpb=2 ragged=1 vecA=1 | tile drop and mask with two rows per workgroup'),
]
# backward keys: T, rpb, ragged, coltrips (trips of 4 x 64 columns of the d_pi dot product), apasses (passes of the 512 threads over A),
# kmod (K % 12, the region group CG of the score-gradient loop).  backward: (T, B, n, K, A, R, flags, arm)
SENT_BWD = [
    (1, 3, 2, 7, 12, 36, '', 'T=1 rpb=1 coltrips=1 apasses=1 | one step'),
    (3, 3, 2, 7, 12, 36, 'tile', 'T=3 rpb=1 | three steps (blockIdx.y), the tile mask of every step'),
    (1, 103, 5, 7, 12, 36, '', 'rpb=2 ragged=1 | 515 rows round DOWN to two per workgroup, ragged last chunk'),
    (2, 103, 5, 7, 12, 36, 'tile mask', 'T=2 rpb=2 ragged=1 | the same with tile drop, mask and two steps'),
    (1, 256, 8, 7, 12, 36, '', 'rpb=8 ragged=0 | 2048 rows: NMAX = 8 per workgroup'),
    (1, 3, 2, 7, 12, 256, '', 'coltrips=1 | R = 256: exactly one trip of 4 x 64 columns'),
    (1, 3, 2, 7, 12, 257, '', 'coltrips=2 | R = 257: one column into the second trip'),
    (1, 2, 3, 7, 12, 1000, '', 'coltrips=4 | R = 1000, the configured width'),
    (1, 3, 2, 7, 516, 36, '', 'apasses=2 | A = 516: four columns into the second pass of the threads'),
    (1, 3, 2, 11, 12, 36, '', 'kmod=11 | K = 11: one below the region group'),
    (1, 3, 2, 12, 12, 36, '', 'kmod=0 | K = 12: exactly one region group'),
    (1, 3, 2, 13, 12, 36, 'tile', 'kmod=1 | K = 13: one region into the second group, tile drop'),
    (1, 5, 2, 9, 12, 36, 'mask', 'rpb=1 | pi of a masked forward: zero weights and a single-region image'),
    (1, 3, 2, 7, 12, 36, 'off:att off:fr off:d_ctx', 'rpb=1 | operands one float off: the kernel is scalar, nothing may change'),
]
# batched keys: kchunks / kfill (chunks of KCH = 12 regions, K % 12), rblocks (column blocks of 128), rows (T * n), trips4 / trips8 (the
# 4-row trips of sentinel_datt_kernel, the 8-row trips of sentinel_dpatt_kernel), threads (of sentinel_dpatt_kernel), sumtrips (trips
# of sum_all_kernel: 8 x 1024 values each).  batched: (T, B, n, K, A, R, flags, arm)
SENT_BATCHED = [
    (1, 3, 1, 11, 12, 127, '', 'kchunks=1 kfill=11 rblocks=1 rows=1 trips4=1 trips8=1 threads=256 | one row: every clamped index is 0'),
    (3, 3, 1, 12, 12, 128, '', 'kchunks=1 kfill=0 rblocks=1 rows=3 trips4=1 | exactly one chunk and one column block'),
    (2, 2, 2, 13, 20, 129, '', 'kchunks=2 kfill=1 rblocks=2 rows=4 trips4=1 | exactly one trip of 4 rows'),
    (5, 3, 1, 7, 12, 36, '', 'rows=5 trips4=2 trips8=1 | one row into the second 4-row trip'),
    (7, 3, 1, 7, 12, 36, '', 'rows=7 trips8=1 | one below the 8-row trip'),
    (4, 3, 2, 7, 12, 36, '', 'rows=8 trips4=2 trips8=1 | exactly one 8-row trip'),
    (3, 2, 3, 7, 12, 36, 'tile', 'rows=9 trips4=3 trips8=2 | one row into the second 8-row trip; tile drop over steps and rows'),
    (1, 2, 2, 7, 512, 36, '', 'threads=512 | A = 512: 512-thread workgroups'),
    (2, 3, 2, 7, 516, 36, 'tile', 'threads=512 | A = 516: second pass of the threads'),
    (3, 50, 3, 20, 12, 36, '', 'sumtrips=2 kchunks=2 | T * N * (K + 1) = 9450 > 8192: second trip of sum_all_kernel'),
]
