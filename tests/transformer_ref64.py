"""Float64 restatements, on the CPU, of the Transformer / AoA kernels of csrc/transformer.hip and csrc/aoa_ctx.hip (LayerNorm forward
and its three backward forms, short-sequence multi-head attention, the fused GLU / ctx forwards, their backwards and split_halves),
a Python restatement of the attention launch planner, and the case tables that test_transformer_kernels_host.py and
test_transformer_kernels_gpu.py share.  Nothing of the package is imported here: operand semantics are those of include/capmi.h,
TransformerModel.py and AoAModel.py.

Bounds (rel_err = max|got - ref| / max|ref|): the project's own for everything that has one (LayerNorm mean / inv 2e-6, y 5e-6; MHA
o / p 2e-6, dq / dk / dv 5e-6; the GLU / ctx / ReLU / split kernels 2e-6).  The LayerNorm backward had none.  LN_BWD_TOL is derived
as follows: the closed form below evaluated in float32 numpy on every row of LN_BWD, LN_PARTS and LN_SLABS (ln_bwd_f32) differs
from float64 by at most
    dx 1.65e-7, g_scaled 1.47e-7, d_a 2.25e-7, d_b 2.00e-7      (test_transformer_kernels_host.py recomputes and prints them)
and the GPU bound is four times the largest of these (a 64-lane tree sums in another order) but not below 5e-6: 4 x 2.3e-7 =
9.2e-7 < 5e-6, so LN_BWD_TOL = 5e-6.  The MHA accumulate = 1 rows pre-fill dk / dv with values of the gradients' own scale; the one
extra float32 addition (6e-8 relative) leaves them inside the plain 5e-6.

Every LayerNorm case plants one row of 0.5: all its float32 partial sums are exact, so mean = 0.5, std = 0, inv = 1 / eps, y = b and
dx = inv (g - mean g) (the k2 = 0 convention of the kernels).  That row is compared elementwise, not under the case's maximum: its
inv of 1e6 would set the scale (for dx with the row's own float32 scale, see check() in test_transformer_kernels_gpu.py)."""
import numpy as np
import torch

F64 = torch.float64
EPS = 1e-6
LN_BWD_FLOOR = 5e-6
LN_BWD_F32_MEASURED = 2.3e-7            # largest rel_err of ln_bwd_f32 over the tables (host test asserts it is not exceeded)
LN_BWD_TOL = max(4 * LN_BWD_F32_MEASURED, LN_BWD_FLOOR)
MAX_FLOATS = 4 << 20


def gen(seed):
    return torch.Generator().manual_seed(seed)


def d64(t):
    return None if t is None else t.detach().to(F64)


def rel_err(got, ref):
    return float((d64(got) - ref).abs().max() / (ref.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------ LayerNorm
def ne_bucket(D):
    """elements per lane of the register-resident instance capmi_layernorm_* picks for D columns; 0: the streaming kernel"""
    for ne in (4, 8, 16, 32):
        if D <= 64 * ne:
            return ne
    return 0


def ln_parts_rows(M):
    """capmi_layernorm_bwd_parts_rows"""
    return min(max((M + 7) // 8, 1), 4096)


def ln_plant(M):
    return M // 2


LN_DS = (8, 40, 256, 260, 261, 512, 516, 1024, 1028, 2048, 2052)       # NE 4|8, 8|16, 16|32, 32|streaming; 261 % 4 != 0; 8, 40 < 64
LN_MS = (1, 7, 33)                                                       # one wave; a last workgroup with idle waves; nine workgroups
LN_FWD = [(M, D) for D in LN_DS for M in LN_MS]
LN_BWD = [(M, D) for D in LN_DS for M in LN_MS]                          # each with accumulate 0 / 1 x g_scaled NULL / given
LN_PARTS = [(M, D, acc) for D in (8, 256, 260, 512, 516, 1024, 1028, 2048) for M, acc in ((9, 0), (17, 1))]
LN_SLABS = [(7, D, s_dy, s_acc) for D in (40, 260, 516, 1024, 1028, 2048) for s_dy, s_acc in ((1, 1), (3, 2), (5, 9))]


def ln_inputs(M, D, seed):
    """float32 operands of a LayerNorm case; row ln_plant(M) is constant 0.5"""
    g = gen(seed)
    x = (torch.randn(M, D, generator=g) * 1.5 + 0.25).float()
    x[ln_plant(M)] = 0.5
    return dict(x=x, a=(torch.rand(D, generator=g) + 0.5).float(), b=torch.randn(D, generator=g).float(),
                dy=torch.randn(M, D, generator=g).float(), dx0=torch.randn(M, D, generator=g).float(), plant=ln_plant(M))


def ln_fwd_ref(x, a, b, eps=EPS):
    """TransformerModel.py:76-87: a (x - mean) / (std_unbiased + eps) + b -> y, mean, inv"""
    x, a, b = d64(x), d64(a), d64(b)
    D = x.shape[1]
    mean = x.mean(1)
    xc = x - mean[:, None]
    inv = 1.0 / ((xc * xc).sum(1) / (D - 1)).sqrt().add(eps)
    return a * xc * inv[:, None] + b, mean, inv


def ln_bwd_ref(dy, x, a, eps=EPS):
    """closed form of the backward -> dx, g_scaled, d_a, d_b; a row of zero std takes k2 = 0 (transformer.hip)"""
    dy, x, a = d64(dy), d64(x), d64(a)
    D = x.shape[1]
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    sd = ((xc * xc).sum(1, keepdim=True) / (D - 1)).sqrt()
    inv = 1.0 / (sd + eps)
    g = dy * a
    k2 = torch.where(sd > 0, inv * inv / ((D - 1) * sd.clamp_min(1e-300)) * (g * xc).sum(1, keepdim=True), torch.zeros_like(sd))
    dx = inv * (g - g.mean(1, keepdim=True)) - k2 * xc
    gs = dy * xc * inv
    return dx, gs, gs.sum(0), dy.sum(0)


def ln_bwd_f32(dy, x, a, mean, inv, eps=EPS):
    """the same closed form as the kernels state it (from the saved float32 mean / inv), every operation in float32 numpy"""
    f = np.float32
    dy, x, a, mean, inv = (np.asarray(t, dtype=f) for t in (dy, x, a, mean, inv))
    D = x.shape[1]
    mu, iv = mean[:, None], inv[:, None]
    sd = f(1) / iv - f(eps)
    g = dy * a
    xc = x - mu
    sgx = (g * xc).sum(1, keepdims=True, dtype=f)
    mg = g.sum(1, keepdims=True, dtype=f) / f(D)
    with np.errstate(divide='ignore', invalid='ignore'):
        k2 = np.where(sd > 0, iv * iv / (f(D - 1) * sd) * sgx, f(0)).astype(f)
    dx = iv * (g - mg) - k2 * xc
    gs = dy * xc * iv
    return dx, gs, gs.sum(0, dtype=f), dy.sum(0, dtype=f)


def slab_sum(slabs):
    return d64(slabs).sum(0)


# ------------------------------------------------------------------------------------------------ attention launch planner
def _mha_chunk(total, fixed_f, per_f):
    if fixed_f + total * per_f <= 80 * 1024 // 4:
        return total
    budget = 160 * 1024 // 4
    room = (budget - fixed_f) // per_f if budget > fixed_f else 0
    if total <= room:
        return total
    if room < 1:
        return 1
    n = (total + room - 1) // room
    ch = (total + n - 1) // n
    if ((ch + 15) & ~15) <= room:
        ch = (ch + 15) & ~15
    return ch


def mha_plan(kind, Nq, q_per_kv, Tq, Tk, h, dk):
    """(CH, threads, mfma, lds_bytes) of capmi_mha_fwd* (kind 'fwd') / capmi_mha_bwd* ('bwd'): mha_chunk, mha_threads, mha_on_mfma"""
    if kind == 'bwd':
        fixed, per = 4 * Tk * (dk + 4), 2 * (dk + 4) + 3 * (Tk + 1) + 1
    else:
        fixed, per = 2 * Tk * (dk + 4), (dk + 4) + (Tk + 1) + 2
    ch = _mha_chunk(q_per_kv * Tq, fixed, per)
    wgs, scores = (Nq // q_per_kv) * h, ch * Tk
    if wgs < 256:
        threads = 1024 if scores >= 1024 else 512
    else:
        threads = 512 if scores >= 1536 else 256
    return ch, threads, int(ch >= 16), (fixed + ch * per) * 4


def mha_row(name, Nkv, qpk, Tq, Tk, h, dk, mask=None, causal=0, q_pos0=0, drop=True, layout='plain', acc=0, want_p=True, bwd=True,
            arms=()):
    return dict(name=name, Nkv=Nkv, qpk=qpk, Tq=Tq, Tk=Tk, h=h, dk=dk, mask=mask, causal=causal, q_pos0=q_pos0, drop=drop,
                layout=layout, acc=acc, want_p=want_p, bwd=bwd, arms=tuple(arms))


# mask: None | 'q1' (mask_per_q = 1, mask_tq = 1: AoA refiner) | 'kv1' (per kv row, mask_tq = 1) | 'qT' (per query row and position)
# layout: 'plain' | 'packed' (q | k | v column blocks of one [rows, 3D] matrix, gradients likewise) | 'vk' ([value | key] rows of
#         p_att, dk / dv into a [dv | dk] buffer of pitch 2D) | 'pitched' (every row pitch wider than D, gaps must survive)
# arms: what the row is in the table FOR; test_transformer_kernels_host.py checks each claim against mha_arms()
MHA = [
    mha_row('decode t=0: one key', 2, 5, 1, 1, 2, 8, causal=1, q_pos0=0, drop=False,
            arms=('decode_t0', 'fwd:vector', 'bwd:vector', 'no_drop', 'fwd:t512_small', 'bwd:t512_small')),
    mha_row('decode t=6', 2, 5, 1, 7, 2, 8, mask='kv1', causal=1, q_pos0=6, arms=('decode_t6', 'mask_kv1', 'drop')),
    mha_row('causality cuts inside the row block, vector loops, head size 12', 2, 2, 3, 9, 2, 12, causal=1, q_pos0=4,
            arms=('causal_cut', 'fwd:vector', 'dk_not32', 'd4_not_pow2')),
    mha_row('causality cuts inside the row block, MFMA with 17 rows', 1, 1, 17, 21, 2, 16, causal=1, q_pos0=4,
            arms=('causal_cut', 'fwd:mfma17', 'bwd:mfma17')),
    mha_row('16 rows x 16 keys, mask per query position', 3, 1, 16, 16, 2, 16, mask='qT', arms=('fwd:mfma16', 'bwd:mfma16', 'tk16', 'mask_qT')),
    mha_row('17 keys, refiner mask, head size 20', 2, 2, 8, 17, 2, 20, mask='q1', arms=('tk17', 'mask_q1', 'd4_not_pow2', 'dk_not32')),
    mha_row('64 keys: last size of the 16-lane softmax', 2, 1, 20, 64, 2, 32, mask='kv1', arms=('tk64', 'fwd:one_pass_80k', 'bwd:one_pass_80k')),
    mha_row('65 keys: first size of the wave softmax', 2, 1, 20, 65, 2, 32, mask='kv1', arms=('tk65',)),
    mha_row('120 rows, dk 128: forward in one 160 KB pass, backward in passes of 48', 1, 6, 20, 36, 1, 128, mask='kv1',
            arms=('fwd:one_pass_160k', 'bwd:passes_x16', 'fwd:t1024', 'bwd:t1024')),
    mha_row('40 rows, dk 128: backward in one 160 KB pass', 1, 2, 20, 36, 2, 128, arms=('bwd:one_pass_160k',)),
    mha_row('200 rows, dk 128: forward in passes of 112, backward in passes of 50', 1, 8, 25, 36, 1, 128, drop=False,
            arms=('fwd:passes_x16', 'bwd:passes_odd')),
    mha_row('136 keys, dk 128: forward passes of 16 + 3 rows on MFMA', 1, 1, 19, 136, 1, 128, bwd=False,
            arms=('fwd:short_last_mfma',)),
    mha_row('forward passes of 17 + 16 rows', 1, 1, 33, 128, 1, 128, bwd=False, drop=False, arms=('fwd:passes_odd',)),
    mha_row('60 keys, dk 128: backward passes of 16 + 5 rows on MFMA', 1, 1, 21, 60, 1, 128, mask='kv1', arms=('bwd:short_last_mfma',)),
    mha_row('256 workgroups, 720 scores: 4 waves', 32, 1, 20, 36, 8, 8, mask='qT', arms=('fwd:t256', 'bwd:t256')),
    mha_row('256 workgroups, 1728 scores: 8 waves', 32, 2, 24, 36, 8, 8, mask='kv1', arms=('fwd:t512_big', 'bwd:t512_big')),
    mha_row('packed q | k | v of the refiner', 3, 1, 9, 9, 2, 16, mask='q1', layout='packed', arms=('packed_qkv', 'mask_q1')),
    mha_row('packed q | k | v, 36 regions on MFMA', 2, 1, 36, 36, 2, 32, mask='q1', layout='packed', arms=('packed_qkv',)),
    mha_row('[value | key] rows, gradients accumulated into [dv | dk]', 3, 5, 1, 11, 2, 16, mask='kv1', layout='vk', acc=1,
            arms=('vk_layout', 'bwd_accumulate')),
    mha_row('[value | key] rows on MFMA, accumulate', 2, 4, 5, 36, 2, 32, mask='kv1', layout='vk', acc=1, drop=False,
            arms=('vk_layout', 'bwd_accumulate')),
    mha_row('every pitch wider than its row', 2, 3, 7, 10, 2, 24, mask='qT', layout='pitched', acc=1, arms=('pitched', 'bwd_accumulate')),
    mha_row('no probabilities wanted', 2, 2, 5, 13, 2, 16, want_p=False, arms=('no_p',)),
]

MHA_ARMS = tuple(k + ':' + a for k in ('fwd', 'bwd')
                 for a in ('vector', 'mfma16', 'mfma17', 'one_pass_80k', 'one_pass_160k', 'passes_x16', 'passes_odd', 'short_last_mfma',
                           't256', 't512_big', 't512_small', 't1024')) + \
    ('tk16', 'tk17', 'tk64', 'tk65', 'dk_not32', 'd4_not_pow2', 'decode_t0', 'decode_t6', 'causal_cut', 'mask_q1', 'mask_kv1',
     'mask_qT', 'packed_qkv', 'vk_layout', 'pitched', 'bwd_accumulate', 'no_p', 'drop', 'no_drop')


def mha_arms(r):
    """the arms a table row reaches, from mha_plan and its own settings"""
    out = set()
    Nq, total = r['Nkv'] * r['qpk'], r['qpk'] * r['Tq']
    for kind in ('fwd', 'bwd') if r['bwd'] else ('fwd',):
        ch, threads, mfma, lds = mha_plan(kind, Nq, r['qpk'], r['Tq'], r['Tk'], r['h'], r['dk'])
        wgs = r['Nkv'] * r['h']
        tags = ['mfma%d' % ch if mfma and ch in (16, 17) else None, None if mfma else 'vector']
        if ch == total:
            tags.append('one_pass_80k' if lds <= 80 * 1024 else 'one_pass_160k')
        else:
            tags.append('passes_x16' if ch % 16 == 0 else 'passes_odd')
            last = total - (total - 1) // ch * ch
            if mfma and 1 <= last <= 15:
                tags.append('short_last_mfma')
        tags.append({256: 't256', 1024: 't1024'}.get(threads, 't512_big' if wgs >= 256 else 't512_small'))
        out.update(kind + ':' + t for t in tags if t)
    if r['Tk'] in (16, 17, 64, 65):
        out.add('tk%d' % r['Tk'])
    if r['dk'] % 32:
        out.add('dk_not32')
    d4 = r['dk'] // 4
    if d4 & (d4 - 1):
        out.add('d4_not_pow2')
    if r['causal'] and r['Tq'] == 1 and r['Tk'] == r['q_pos0'] + 1:
        out.add('decode_t0' if r['q_pos0'] == 0 else 'decode_t%d' % r['q_pos0'])
    if r['causal'] and r['Tq'] > 1 and r['q_pos0'] > 0 and r['q_pos0'] + r['Tq'] - 1 < r['Tk']:
        out.add('causal_cut')
    if r['mask']:
        out.add('mask_' + r['mask'])
    out.add({'packed': 'packed_qkv', 'vk': 'vk_layout', 'pitched': 'pitched'}.get(r['layout'], 'plain'))
    if r['acc'] and r['bwd']:
        out.add('bwd_accumulate')
    if not r['want_p']:
        out.add('no_p')
    out.add('drop' if r['drop'] else 'no_drop')
    return out


def mha_floats(r):
    """floats of the largest set of buffers a row allocates (q, k, v, d_o, o, p, drop and the three gradients, at pitch 3D at most)"""
    D, Nq = r['h'] * r['dk'], r['Nkv'] * r['qpk']
    return 3 * 3 * D * (Nq * r['Tq'] + r['Nkv'] * r['Tk']) + 3 * Nq * r['h'] * r['Tq'] * r['Tk']


def mha_inputs(r, seed):
    g = gen(seed)
    Nkv, qpk, Tq, Tk, h, dk = (r[k] for k in ('Nkv', 'qpk', 'Tq', 'Tk', 'h', 'dk'))
    D, Nq = h * dk, Nkv * qpk
    d = dict(q=torch.randn(Nq, Tq, D, generator=g), k=torch.randn(Nkv, Tk, D, generator=g), v=torch.randn(Nkv, Tk, D, generator=g),
             d_o=torch.randn(Nq, Tq, D, generator=g), dk0=torch.randn(Nkv, Tk, D, generator=g), dv0=torch.randn(Nkv, Tk, D, generator=g))
    mask = None
    if r['mask']:
        rows, mtq = (Nq if r['mask'] in ('q1', 'qT') else Nkv), (Tq if r['mask'] == 'qT' else 1)
        mask = torch.rand(rows, mtq, Tk, generator=g) > 0.3
        mask[..., 0] = True                       # no fully masked row: NaN in the reference too, and the engines never make one
    d['mask'] = mask
    d['drop'] = ((torch.rand(Nq, h, Tq, Tk, generator=g) > 0.2).float() / 0.8) if r['drop'] else None
    return d


def mha_ref(r, d):
    """MultiHeadedAttention (TransformerModel.py:152-195) in float64 -> o [Nq,Tq,D], p [Nq,h,Tq,Tk], dq, dk, dv (dk / dv on top of
    dk0 / dv0 where the row accumulates)"""
    Nkv, qpk, Tq, Tk, h, dk = (r[k] for k in ('Nkv', 'qpk', 'Tq', 'Tk', 'h', 'dk'))
    D, Nq = h * dk, Nkv * qpk
    qd, kd, vd = (d64(d[k]).requires_grad_(True) for k in ('q', 'k', 'v'))
    qh = qd.view(Nq, Tq, h, dk).transpose(1, 2)
    kh = kd.view(Nkv, Tk, h, dk).transpose(1, 2).repeat_interleave(qpk, 0)
    vh = vd.view(Nkv, Tk, h, dk).transpose(1, 2).repeat_interleave(qpk, 0)
    sc = qh @ kh.transpose(-1, -2) / dk ** 0.5
    if d['mask'] is not None:
        m = d['mask'] if r['mask'] in ('q1', 'qT') else d['mask'].repeat_interleave(qpk, 0)
        sc = sc.masked_fill(~m.unsqueeze(1), float('-inf'))                    # [Nq, 1, 1 or Tq, Tk]
    if r['causal']:
        ok = torch.arange(Tk)[None, :] <= r['q_pos0'] + torch.arange(Tq)[:, None]
        sc = sc.masked_fill(~ok, float('-inf'))
    p = torch.softmax(sc, -1)
    o = ((p * d64(d['drop']) if d['drop'] is not None else p) @ vh).transpose(1, 2).reshape(Nq, Tq, D)
    o.backward(d64(d['d_o']))
    dk_, dv_ = kd.grad, vd.grad
    if r['acc']:
        dk_, dv_ = dk_ + d64(d['dk0']), dv_ + d64(d['dv0'])
    return o.detach(), p.detach(), qd.grad, dk_, dv_


# ------------------------------------------------------------------------------------------------ GLU / ctx / ReLU / split
CTX_GLU, CTX_RELU, CTX_LSTM = 0, 1, 2
CTX_G = {CTX_GLU: 2, CTX_RELU: 1, CTX_LSTM: 4}
FUSED_SHAPES = [(1, 4), (7, 36), (64, 36), (64, 4), (1, 36)]           # (M, R); M <= 64 everywhere: planes on every shape
FUSED_SPLITS = (1, 4, 5, 9)                                             # trips of 4: one short, one full, 4 + 1, 4 + 4 + 1
GLU_FUSED = [(M, R, s, masked) for M, R in FUSED_SHAPES for s in FUSED_SPLITS for masked in (False, True)]
CTX_FUSED = [(kind, M, R, s, masked) for kind in (CTX_GLU, CTX_RELU, CTX_LSTM) for M, R in FUSED_SHAPES for s in FUSED_SPLITS
             for masked in (False, True)]
ADD_SPLITS = (None, 1, 8, 9)                                            # no slabs; trips of 8: short, full, 8 + 1
RELU_BWD = [(M, R, s, am) for M, R in ((1, 4), (7, 37), (65, 36)) for s in ADD_SPLITS for am in (False, True) if s or not am]
GLU_BWD = [(M, R, s, am) for M, R in ((1, 4), (7, 37), (65, 36)) for s in ADD_SPLITS for am in (False, True) if s or not am]
SPLIT_HALVES = [(M, R, s, masked) for M, R in ((1, 4), (7, 37), (65, 36)) for s in (1, 8, 9) for masked in (False, True)]


def keep_mask(g, M, R, p=0.7):
    return ((torch.rand(M, R, generator=g) < p).float() / p)


def slabs_of(g, splits, M, W, pad=8):
    """`splits` slabs of an [M, W] matrix, `M W + pad` floats apart -> (raw [splits, stride] float32, stride, float64 sum [M, W])"""
    stride = M * W + pad
    raw = (torch.randn(splits, stride, generator=g) / splits ** 0.5).float()
    return raw, stride, d64(raw[:, :M * W]).view(splits, M, W).sum(0)


def fused_inputs(kind, M, R, splits, masked, seed):
    g = gen(seed)
    G = CTX_G[kind]
    raw, stride, tot = slabs_of(g, splits, M, G * R)
    d = dict(slabs=raw, stride=stride, bias=torch.randn(G * R, generator=g).float(),
             bias2=torch.randn(G * R, generator=g).float() if (kind == CTX_LSTM or masked) else None,
             c_prev=torch.randn(M, R, generator=g).float() if kind == CTX_LSTM else None,
             resid=torch.randn(M, R, generator=g).float() if masked or kind == CTX_RELU else None,
             mask_a=keep_mask(g, M, R) if masked else None, mask_b=keep_mask(g, M, R, 0.5) if masked else None)
    d['pre'] = tot + d64(d['bias']) + (d64(d['bias2']) if d['bias2'] is not None else 0.0)
    return d


def fused_ref(kind, d):
    """-> pre as the backward reads it (None: not written), c, out, out_a = mask_a (out + resid), out_b = mask_b out"""
    pre = d['pre']
    R = pre.shape[1] // CTX_G[kind]
    c = None
    if kind == CTX_RELU:
        out, saved = pre.clamp_min(0.0), None
    elif kind == CTX_GLU:
        out, saved = pre[:, :R] * torch.sigmoid(pre[:, R:]), pre
    else:
        i, f, gg, o = pre.chunk(4, 1)
        i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        c = f * d64(d['c_prev']) + i * gg
        out, saved = o * torch.tanh(c), torch.cat([i, f, gg, o], 1)
    oa = out + d64(d['resid']) if d.get('resid') is not None else out
    oa = oa * d64(d['mask_a']) if d['mask_a'] is not None else oa
    ob = out * d64(d['mask_b']) if d['mask_b'] is not None else out
    return saved, c, out, oa, ob


def add_inputs(M, R, splits, add_mask, seed, glu):
    g = gen(seed)
    d = dict(d_out=torch.randn(M, R, generator=g).float(), mask=keep_mask(g, M, R) if glu else None, slabs=None, stride=0, add=None,
             add_mask=keep_mask(g, M, R, 0.5) if add_mask else None)
    if splits:
        d['slabs'], d['stride'], d['add'] = slabs_of(g, splits, M, R)
    if glu:
        d['pre'] = (torch.randn(M, 2 * R, generator=g) * 2).float()
    else:
        out = torch.randn(M, R, generator=g).clamp_min(0.0).float()
        out.view(-1)[::3] = 0.0                    # planted zeros beside those of the ReLU itself
        out.view(-1)[1::7] = -0.0
        d['out'] = out
    return d


def add_grad(d):
    g = d64(d['d_out'])
    if d.get('mask') is not None:
        g = g * d64(d['mask'])
    if d['add'] is not None:
        g = g + (d['add'] * d64(d['add_mask']) if d['add_mask'] is not None else d['add'])
    return g


def relu_bwd_ref(d):
    return torch.where(d64(d['out']) > 0, add_grad(d), torch.zeros((), dtype=F64))


def glu_bwd_ref(d):
    g, pre = add_grad(d), d64(d['pre'])
    R = g.shape[1]
    a, sg = pre[:, :R], torch.sigmoid(pre[:, R:])
    return torch.cat([g * sg, g * a * sg * (1 - sg)], 1)


def split_inputs(M, R, splits, masked, seed):
    g = gen(seed)
    raw, stride, tot = slabs_of(g, splits, M, 2 * R)
    return dict(slabs=raw, stride=stride, tot=tot, mask_lo=keep_mask(g, M, R) if masked else None,
                mask_hi=keep_mask(g, M, R, 0.5) if masked else None)


def split_ref(d):
    R = d['tot'].shape[1] // 2
    lo, hi = d['tot'][:, :R], d['tot'][:, R:]
    return (lo * d64(d['mask_lo']) if d['mask_lo'] is not None else lo), (hi * d64(d['mask_hi']) if d['mask_hi'] is not None else hi)
