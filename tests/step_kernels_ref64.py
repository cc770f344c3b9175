"""Float64 restatements, on the CPU, of the per-step kernels (LSTM / maxout / att2in2 / adaatt cells, additive attention forward,
backward and time-batched pass) plus the case tables and input builders that test_step_kernels_host.py and
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
