"""Float64 restatements, on the CPU, of the reduction, embedding, ReLU-Jacobian, Adam and dropout-mask kernels of csrc/pointwise.hip
and of the two token-embedding kernels of csrc/transformer.hip, plus the case tables and input builders that
test_reduce_kernels_host.py and test_reduce_kernels_gpu.py share.  Nothing of the package is imported here.

Every table row ends in the arm it is meant to reach, as a string of tokens; arm(entry, row) restates the HOST dispatch predicates of
pointwise.hip, transformer.hip and embed_bwd_det.h (and the loop bounds of the kernels where a row is about a loop tail) and returns
that string for the row.  REQUIRED lists, per entry point, the tokens that at least one row has to carry."""
import functools

import numpy as np
import torch

import optim_ref64 as O

F64 = torch.float64
NAN = float('nan')

# constants of the sources the predicates below restate
GRID_CAP = 2048                 # host_common.h grid_for: workgroups of a grid-stride launch
CS_R, CS_COLS = 64, 64          # colsum_kernel / colsum_item_body: row slices, columns per block
COLSUM_BATCH_GRID = 160         # capmi_colsum_batch: column blocks per item in the grid
COLSUM_ARGS_GRID = 64           # capmi_colsum_batch_args: at most this many
COLSUM_ARGS_MAX = 8             # capmi.h CAPMI_COLSUM_ARGS_MAX
GRS_PARTS = 4                   # group_rowsum_v4_kernel
EBD_THREADS, EBD_WAVES, EBD_MAX_ROWS = 1024, 16, 14336          # embed_bwd_det.h
LDS_DEFAULT = 64 * 1024         # dynamic + static LDS a kernel gets without the opt-in
FILL = 0.25                     # dE before every embedding-gradient call (+= semantics)

COLSUM_TOL = 2e-6               # rel_err, test_kernels_gpu.py
EMBED_TOL = 2e-6                # max|got - fill - ref| <= EMBED_TOL * max(1, max|ref|), test_kernels_gpu.py
ADAM_P_TOL = 1e-6               # rel_err(p), wd = 0 and scale = 1, test_adam_matches_torch
ADAM_FACTOR = 4.0               # every other Adam bound: this times the error of the float32 restatement (adam_bounds)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def d64(t):
    return None if t is None else t.detach().to(F64)


def rel_err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def bits(t):
    """float32 tensor -> its bit patterns (so that -0.0 != +0.0 and NaN == NaN)"""
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ column sums
def pitched(rows, cols, ld, seed, offset=0.5):
    """[rows, ld] float32, randn + offset in the first `cols` columns, NaN in the pad"""
    x = torch.full((rows, ld), NAN)
    x[:, :cols] = torch.randn(rows, cols, generator=gen(seed)) + offset
    return x


def colsum(x, cols, out0=None):
    """float64 column sums of the first `cols` columns of the pitched x, added to out0 when accumulating"""
    s = d64(x)[:, :cols].sum(0)
    return s if out0 is None else s + d64(out0)


def _why_scalar(off, ld, cols):
    why = [w for w, hit in (('align', off), ('ld%4', ld % 4), ('cols%4', cols % 4)) if hit]
    return 'scalar(%s)' % '+'.join(why) if why else 'vec'


def _trips(spans, steps):
    """which of the `steps`-rows-at-a-time loops (descending) some thread of a 64-slice walk over `span` rows enters"""
    taken = set()
    for span in spans:
        for ry in range(min(CS_R, span)):
            r = ry
            for k in steps:
                while r + (k - 1) * CS_R < span:
                    taken.add(k)
                    r += k * CS_R
    return ['%drow' % k for k in steps if k in taken]


# capmi_colsum: (rows, cols, ld, in one float off, accumulate, arm)
COLSUM = [
    (37, 5, 5, False, 0, 'scalar(ld%4+cols%4) rsplit=1 store'),
    (323, 8, 12, False, 0, 'vec 4row 1row rsplit=1 store pitched'),
    (323, 8, 9, False, 0, 'scalar(ld%4) rsplit=1 store pitched'),
    (323, 6, 8, False, 0, 'scalar(cols%4) rsplit=1 store pitched'),
    (323, 8, 8, True, 0, 'scalar(align) rsplit=1 store'),
    (200, 68, 68, False, 0, 'vec 4row 1row rsplit=1 store cblocks=2'),
    (1100, 8, 8, False, 0, 'vec 4row 1row rsplit=4 memset'),
    (1100, 8, 8, False, 1, 'vec 4row 1row rsplit=4 preloaded'),
    (1100, 6, 8, False, 0, 'scalar(cols%4) rsplit=4 memset pitched'),
    (1024, 4096, 4096, False, 0, 'vec 4row rsplit=1 store cblocks=64'),
    (64, 8, 8, False, 1, 'vec 1row rsplit=1 acc'),
]


def colsum_rsplit(rows, cols):
    cblocks = (cols + CS_COLS - 1) // CS_COLS
    if cblocks < 64 and rows >= 4 * CS_R * 4:
        return max(1, min(128 // cblocks, rows // (CS_R * 4)))
    return 1


def _arm_colsum(c):
    rows, cols, ld, off, acc = c[:5]
    if rows <= 0 or cols <= 0:
        return 'EINVAL'
    t = [_why_scalar(off, ld, cols)]
    rs = colsum_rsplit(rows, cols)
    if t[0] == 'vec':
        t += _trips([rows * (y + 1) // rs - rows * y // rs for y in range(rs)], (4, 1))
    t.append('rsplit=%d' % rs)
    t.append(('preloaded' if acc else 'memset') if rs > 1 else ('acc' if acc else 'store'))
    if ld > cols:
        t.append('pitched')
    cblocks = (cols + CS_COLS - 1) // CS_COLS
    if cblocks > 1:
        t.append('cblocks=%d' % cblocks)
    return ' '.join(t)


# one launch of capmi_colsum_batch / capmi_colsum_batch_args: (rows, cols, ld, in one float off, accumulate, out2, arm).  `wrap`: the
# item has more column blocks than the grid has (160 in _batch; _args launches min(64, most blocks of any item)).
COLSUM_BATCH = [
    (837, 8, 8, False, 0, False, 'vec 8row 4row 1row'),
    (70, 6, 7, False, 0, False, 'scalar(ld%4+cols%4) pitched'),
    (3, 10244, 10244, False, 0, False, 'vec 1row wrap(batch) wrap(args)'),
    (3, 4100, 4100, False, 0, False, 'vec 1row wrap(args)'),
    (70, 8, 8, False, 0, True, 'vec 1row out2'),
    (300, 12, 12, False, 1, False, 'vec 4row 1row acc'),
    (100, 8, 12, False, 0, False, 'vec 1row pitched'),
    (50, 8, 8, True, 1, True, 'scalar(align) acc out2'),
]


def _arm_colsum_batch(c):
    rows, cols, ld, off, acc, out2 = c[:6]
    if rows <= 0 or cols <= 0:
        return 'EINVAL'
    t = [_why_scalar(off, ld, cols)]
    if t[0] == 'vec':
        t += _trips([rows], (8, 4, 1))
    if acc:
        t.append('acc')
    if out2:
        t.append('out2')
    if ld > cols:
        t.append('pitched')
    cblocks = (cols + CS_COLS - 1) // CS_COLS
    if cblocks > COLSUM_BATCH_GRID:
        t.append('wrap(batch)')
    if cblocks > COLSUM_ARGS_GRID:
        t.append('wrap(args)')
    return ' '.join(t)


# ------------------------------------------------------------------------------------------------ grouped row sum
# (T, groups, group, cols, pad rows per slab, pad floats per slab, in off, out off, arm); slab = (groups * group + pad rows) * cols + pad floats
GROUP_ROWSUM = [
    (1, 1, 1, 4, 0, 0, False, False, 'v4 clamped empty wg=1 dead'),
    (4, 3, 9, 8, 0, 0, False, False, 'v4 batch8 clamped wg=1 dead'),
    (3, 17, 2, 20, 5, 0, False, False, 'v4 clamped empty wg=2 dead slab>'),
    (4, 3, 9, 6, 0, 2, False, False, 'scalar(cols%4) slab>'),
    (4, 3, 9, 8, 0, 1, False, False, 'scalar(slab%4) slab>'),
    (4, 3, 9, 8, 0, 0, True, False, 'scalar(align in)'),
    (4, 3, 9, 8, 0, 0, False, True, 'scalar(align out)'),
]


def group_rowsum_slab(c):
    T, groups, group, cols, pad_rows, pad_floats = c[:6]
    return (groups * group + pad_rows) * cols + pad_floats


def group_rowsum_input(c, seed):
    """[T, slab] float32: randn + 0.5 in the live rows, NaN in the pad rows and pad floats"""
    T, groups, group, cols = c[:4]
    live = groups * group * cols
    x = torch.full((T, group_rowsum_slab(c)), NAN)
    x[:, :live] = torch.randn(T, live, generator=gen(seed)) + 0.5
    return x


def group_rowsum(x, c):
    T, groups, group, cols = c[:4]
    return d64(x)[:, :groups * group * cols].view(T, groups, group, cols).sum((0, 2))


def _arm_group_rowsum(c):
    T, groups, group, cols, pad_rows, pad_floats, off_in, off_out = c[:8]
    slab = group_rowsum_slab(c)
    why = [w for w, hit in (('cols%4', cols % 4), ('slab%4', slab % 4), ('align in', off_in), ('align out', off_out)) if hit]
    if why:
        t = ['scalar(%s)' % '+'.join(why)]
    else:
        rows = T * group
        per = (rows + GRS_PARTS - 1) // GRS_PARTS
        spans = [max(0, min(rows, (p + 1) * per) - p * per) for p in range(GRS_PARTS)]
        nq = groups * (cols // 4)
        t = ['v4']
        if max(spans) >= 8:
            t.append('batch8')
        if any(s % 8 for s in spans):
            t.append('clamped')
        if min(spans) == 0:
            t.append('empty')
        t.append('wg=%d' % ((nq + 63) // 64))
        if nq % 64:
            t.append('dead')
    if slab > groups * group * cols:
        t.append('slab>')
    return ' '.join(t)


# ------------------------------------------------------------------------------------------------ token embedding (decoders)
# capmi_embed_fwd(_pl): (N, Ed, it_stride, it_save, relu, mask, planes, arm)
EMBED_FWD = ([(7, 5, s) + f for s in (1, 3) for f in ((True, False, False, False, 'it_save'), (False, True, False, False, 'relu'),
                                                       (False, False, True, False, 'mask'), (True, True, True, False, 'it_save relu mask'))] +
             [(64, 8, 1, True, True, True, True, 'it_save relu mask planes'),
              (65, 8, 1, False, True, True, True, 'EINVAL')])
EMBED_V = 11


def _arm_embed_fwd(c):
    N, Ed, stride, it_save, relu, mask, planes = c[:7]
    if planes and N > 64:
        return 'EINVAL'
    return ' '.join(k for k, on in (('it_save', it_save), ('relu', relu), ('mask', mask), ('planes', planes)) if on)


def embed_fwd_inputs(c, seed):
    N, Ed, stride = c[:3]
    g = gen(seed)
    it = torch.full((N, stride), EMBED_V - 1, dtype=torch.long)           # the columns the stride skips hold another, valid token
    it[:, 0] = torch.randint(0, EMBED_V - 1, (N,), generator=g)
    E = torch.randn(EMBED_V, Ed, generator=g)
    mask = (torch.rand(N, Ed, generator=g) < 0.5).float() * 2
    return it, E, mask


def embed_fwd(it, E, mask, relu):
    """x = relu(E[it[:, 0]]) * mask in the dtype of E (float32: the kernel's own three operations, float64: the reference)"""
    x = E[it[:, 0]]
    if relu:
        x = x.clamp_min(0.0)
    return x if mask is None else x * mask.to(x.dtype)


def embed_tokens(rows, V, hot, seed):
    """token ids of `rows` positions: uniform over [0, V - 1), a share `hot` of them token 3; token V - 1 only where a case plants it:
    past position 1024 when there are that many (its leader is found in the scan's second pass), else nowhere"""
    g = gen(seed)
    tok = torch.randint(0, V - 1, (rows,), generator=g)
    if hot > 0:
        tok[torch.rand(rows, generator=g) < hot] = 3
    if rows > 1080:
        tok[1050] = V - 1
        tok[1077] = V - 1
    return tok


# capmi_embed_bwd: (rows, Ed, V, relu, mask, operand one float off or None, hot, arm)
EMBED_BWD = [
    (7, 8, 5, 1, True, None, 0.0, 'det idle'),
    (1100, 260, 9, 1, True, None, 0.4, 'det loop8 idle scan2 late y=2'),
    (1100, 260, 9, 0, True, None, 0.4, 'det loop8 idle scan2 late y=2 norelu'),
    (1100, 260, 9, 1, False, None, 0.4, 'det loop8 idle scan2 late y=2 nomask'),
    (7, 6, 5, 1, True, None, 0.0, 'atomic(Ed%4)'),
    (7, 8, 5, 1, True, 'dx', 0.0, 'atomic(align dx)'),
    (7, 8, 5, 1, True, 'dE', 0.0, 'atomic(align dE)'),
    (14337, 4, 7, 1, True, None, 0.0, 'atomic(rows>max)'),
    (12272, 4, 7, 1, True, None, 0.0, 'det loop8 idle scan2 late'),
    (12273, 4, 7, 1, True, None, 0.0, 'det loop8 idle scan2 late lds>64K'),
    (14336, 4, 7, 1, True, None, 0.0, 'det loop8 idle scan2 late lds>64K'),
]


def embed_bwd_det_lds(rows):
    return ((rows + 3) & ~3) * 4 + EBD_WAVES * 64 * 16


def _det_tokens(tok, rows, D):
    """tokens of the deterministic kernel for the flat token list `tok`"""
    t = ['det']
    counts = torch.bincount(tok)
    counts = counts[counts > 0]
    if int(counts.max()) > 8 * EBD_WAVES:            # some wave's share holds eight rows
        t.append('loop8')
    if int(counts.min()) < EBD_WAVES:                # a list shorter than the waves: some have lo >= hi
        t.append('idle')
    if rows > EBD_THREADS:
        t.append('scan2')
        first = {}
        for i, k in enumerate(tok.tolist()):
            first.setdefault(k, i)
        if max(first.values()) >= EBD_THREADS:
            t.append('late')
    if D > 256:
        t.append('y=%d' % ((D + 255) // 256))
    if embed_bwd_det_lds(rows) + 4 * EBD_WAVES > LDS_DEFAULT:
        t.append('lds>64K')
    return t


def _arm_embed_bwd(c, i):
    rows, Ed, V, relu, mask, off, hot = c[:7]
    why = [w for w, hit in (('Ed%4', Ed % 4), ('rows>max', rows > EBD_MAX_ROWS), ('align %s' % off, off in ('dx', 'x_saved', 'mask', 'dE')))
           if hit]
    if why:
        return 'atomic(%s)' % '+'.join(why)
    t = _det_tokens(embed_tokens(rows, V, hot, 400 + i), rows, Ed)
    if not relu:
        t.append('norelu')
    if not mask:
        t.append('nomask')
    return ' '.join(t)


def embed_bwd_inputs(i):
    """tok [rows], dx, x_saved, mask [rows, Ed] of row i of EMBED_BWD"""
    rows, Ed, V, relu, mask, off, hot = EMBED_BWD[i][:7]
    tok = embed_tokens(rows, V, hot, 400 + i)
    g = gen(500 + i)
    dx, xs = torch.randn(rows, Ed, generator=g), torch.randn(rows, Ed, generator=g)
    m = (torch.rand(rows, Ed, generator=g) < 0.5).float() * 2
    return tok, dx, (xs if relu else None), (m if mask else None)


def embed_bwd(tok, dx, x_saved, mask, V):
    """float64 scatter-add of dx * mask * (x_saved > 0) into [V, Ed] zeros"""
    gr = d64(dx)
    if mask is not None:
        gr = gr * d64(mask)
    if x_saved is not None:
        gr = gr * (x_saved > 0).to(F64)
    dE = torch.zeros(V, dx.shape[-1], dtype=F64)
    for r, k in enumerate(tok.reshape(-1).tolist()):
        dE[k] += gr.reshape(-1, dx.shape[-1])[r]
    return dE


# ------------------------------------------------------------------------------------------------ token embedding (Transformer)
# capmi_embed_pe_fwd: (N, T, D, tok_ld, pos0, drop, arm)
EMBED_PE_FWD = [(3, 5, 8, 7, p0, dr, 'pos0=%d%s' % (p0, ' drop' if dr else '')) for p0 in (0, 2) for dr in (True, False)]
# capmi_embed_pe_bwd: (N, T, D, tok_ld, drop, V, arm)
EMBED_PE_BWD = [
    (3, 5, 8, 7, True, 5, 'det idle'),
    (3, 5, 8, 7, False, 5, 'det idle nodrop'),
    (3, 5, 6, 7, True, 5, 'atomic(D%4)'),
    (3, 4091, 4, 4092, True, 7, 'det loop8 idle scan2 late lds>64K'),
    (7, 2048, 4, 2049, True, 7, 'det loop8 idle scan2 late lds>64K'),
    (3, 4779, 4, 4780, True, 7, 'atomic(rows>max)'),
]


def _arm_embed_pe_fwd(c):
    return 'pos0=%d%s' % (c[4], ' drop' if c[5] else '')


def _arm_embed_pe_bwd(c, i):
    N, T, D, tok_ld, drop, V = c[:6]
    why = [w for w, hit in (('D%4', D % 4), ('rows>max', N * T > EBD_MAX_ROWS)) if hit]
    if why:
        return 'atomic(%s)' % '+'.join(why)
    t = _det_tokens(embed_tokens(N * T, V, 0.0, 600 + i), N * T, D)
    if not drop:
        t.append('nodrop')
    return ' '.join(t)


def embed_pe_inputs(N, T, D, tok_ld, V, seed, pos_rows):
    """tok [N, tok_ld] (the pad columns hold token 0, valid but wrong), E [V, D], pe [pos_rows, D], drop / dx [N, T, D]"""
    tok = torch.zeros(N, tok_ld, dtype=torch.long)
    tok[:, :T] = embed_tokens(N * T, V, 0.0, seed).view(N, T)
    g = gen(seed + 100)
    E, pe = torch.randn(V, D, generator=g), torch.randn(pos_rows, D, generator=g)
    drop = (torch.rand(N, T, D, generator=g) < 0.5).float() * 2
    dx = torch.randn(N, T, D, generator=g)
    return tok, E, pe, drop, dx


def pe_scale(D):
    """sqrtf((float)D) as the host passes it to the kernels"""
    return float(np.sqrt(np.float32(D)))


def embed_pe_fwd(tok, E, pe, drop, T, pos0):
    """float64 x = (E[tok] * sqrt(float32(D)) + pe[pos0 + t]) * drop, and the magnitude |E| s + |pe| (times drop) its roundings scale with"""
    D = E.shape[1]
    e, p = d64(E)[tok[:, :T]] * pe_scale(D), d64(pe)[pos0:pos0 + T].unsqueeze(0)
    x, mag = e + p, e.abs() + p.abs()
    if drop is not None:
        x, mag = x * d64(drop), mag * d64(drop)
    return x, mag


def embed_pe_bwd(tok, dx, drop, T, V):
    gr = d64(dx) * pe_scale(dx.shape[-1])
    if drop is not None:
        gr = gr * d64(drop)
    return embed_bwd(tok[:, :T].reshape(-1), gr.reshape(-1, dx.shape[-1]), None, None, V)


# ------------------------------------------------------------------------------------------------ ReLU / dropout Jacobians
RELU_COUNT = 1000
# capmi_relu_mask_bwd: (y_ref given, mask given, arm)
RELU_MASK_BWD = [(True, True, 'gate mask'), (True, False, 'gate'), (False, True, 'mask'), (False, False, 'copy')]


def _arm_relu_mask_bwd(c):
    return {(True, True): 'gate mask', (True, False): 'gate', (False, True): 'mask', (False, False): 'copy'}[c[:2]]


def _arm_relu_scale_bwd(c):
    count, off = c[:2]
    return 'EINVAL' if (count <= 0 or count % 4 or off) else 'quads'


# capmi_relu_scale_bwd: (count, an operand one float off, arm)
RELU_SCALE_BWD = [(1000, False, 'quads'), (1002, False, 'EINVAL'), (1000, True, 'EINVAL')]


def relu_inputs(count, seed):
    """dy, y_ref, mask; y_ref carries +0.0, -0.0 and a tiny positive value among its first elements"""
    g = gen(seed)
    dy, y = torch.randn(count, generator=g), torch.randn(count, generator=g)
    y[0], y[1], y[2] = 0.0, -0.0, 1e-30
    dy[0], dy[1], dy[2] = 1.5, -2.5, -3.5
    mask = (torch.rand(count, generator=g) < 0.5).float() * 2
    mask[:3] = 2.0
    return dy, y, mask


def relu_mask_bwd(dy, y_ref, mask):
    """dx = dy * mask where y_ref > 0, else +0.0, in the dtype of dy"""
    gr = dy if mask is None else dy * mask.to(dy.dtype)
    return gr if y_ref is None else torch.where(y_ref > 0, gr, torch.zeros_like(gr))


def relu_scale_bwd(dy, y_ref, scale):
    return torch.where(y_ref > 0, dy * torch.tensor(scale, dtype=dy.dtype), torch.zeros_like(dy))


# ------------------------------------------------------------------------------------------------ clip + Adam
ADAM_HP = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8)
ADAM_SETS = {'clip': dict(clip=0.1, wd=0.0, scale=1.0), 'decay': dict(clip=0.0, wd=0.01, scale=0.5),
             'all': dict(clip=0.1, wd=0.01, scale=2.0)}
ADAM_STEPS = 3
# capmi_adam_step: (count, arm).  adam2_kernel runs grid_for(quads / 2 + 1) workgroups of 256: its second quad index is live (`two`)
# only from 257 quads on, and its outer loop would take a second trip only past the 2048-workgroup cap, 2 * 2048 * 256 quads: see
# test_reduce_kernels_gpu.test_adam_step.
ADAM = [
    (4, 'adam2 clamped'),
    (8, 'adam2 clamped'),
    (1024, 'adam2 clamped'),
    (1544, 'adam2 two clamped'),
    (1, 'adam_kernel tail'),
    (3, 'adam_kernel tail'),
    (1003, 'adam_kernel quads tail'),
]


def _grid_for(work, per_block=256, cap=GRID_CAP):
    return max(1, min(cap, (work + per_block - 1) // per_block))


def _arm_adam(c):
    count = c[0]
    if count <= 0:
        return 'EINVAL'
    if count % 4 == 0:
        quads = count // 4
        stride = _grid_for(quads // 2 + 1) * 256
        t = ['adam2']
        if quads > stride:
            t.append('two')
        if quads % (2 * stride):                     # the last trip is not full: some first index has no second
            t.append('clamped')
        if quads > 2 * stride:
            t.append('trip2')
        return ' '.join(t)
    t = ['adam_kernel']
    if count // 4:
        t.append('quads')
    t.append('tail')
    return ' '.join(t)


def adam_inputs(count, seed=6):
    """p0 and the gradients of the three steps (0.3 randn: the 0.1 clamp bites on three quarters of them)"""
    g = gen(seed + count)
    return torch.randn(count, generator=g), [torch.randn(count, generator=g) * 0.3 for _ in range(ADAM_STEPS)]


def adam64(p0, grads, clip, wd, scale):
    """capmi.h: scale, clamp, L2 decay into the gradient, then the bias-corrected moments (optim_ref64.step 'adam'), with the
    hyper-parameters as the float32 values the C ABI receives -> p, m, v after every step"""
    p, st, out = p0.double().clone(), O.new_state('adam', p0), []
    for t, gr in enumerate(grads, 1):
        O.step('adam', p, gr, st, O.f32(ADAM_HP['lr']), t, O.f32(ADAM_HP['b1']), O.f32(ADAM_HP['b2']), O.f32(ADAM_HP['eps']),
               O.f32(wd), O.f32(clip), O.f32(scale))
        out.append((p.clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()))
    return out


def adam32(p0, grads, clip, wd, scale):
    """the same formula in float32 torch arithmetic, in the order adam_kernel writes it -> p, m, v after the last step"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)       # noqa: E731
    lr, b1, b2, eps = (f(ADAM_HP[k]) for k in ('lr', 'b1', 'b2', 'eps'))
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t, gr in enumerate(grads, 1):
        bc1 = f(1.0 - float(b1) ** t)
        bc2_sqrt = f((1.0 - float(b2) ** t) ** 0.5)
        x = gr * f(scale)
        if clip > 0:
            x = x.clamp(-float(f(clip)), float(f(clip)))
        if wd:
            x = x + f(wd) * p
        m = b1 * m + (1 - b1) * x
        v = b2 * v + (1 - b2) * x * x
        p = p - (lr / bc1) * m / (v.sqrt() / bc2_sqrt + eps)
    return p, m, v


@functools.lru_cache(None)
def adam_f32_error(name):
    """rel_err of adam32 against adam64 for p, m, v after 3 steps: the largest over the counts of ADAM, same inputs as the GPU test"""
    worst = [0.0, 0.0, 0.0]
    for count, _ in ADAM:
        p0, grads = adam_inputs(count)
        ref, got = adam64(p0, grads, **ADAM_SETS[name])[-1], adam32(p0, grads, **ADAM_SETS[name])
        worst = [max(w, rel_err(a, b)) for w, a, b in zip(worst, got, ref)]
    return tuple(worst)


def adam_bounds(name):
    """(p, m, v) bounds of a parameter set: ADAM_FACTOR x the float32 restatement's error, but the project's 1e-6 for p where it has one"""
    p, m, v = (ADAM_FACTOR * e for e in adam_f32_error(name))
    return (ADAM_P_TOL if name == 'clip' else p), m, v


def step_record(steps, lr=ADAM_HP['lr'], b1=ADAM_HP['b1'], b2=ADAM_HP['b2']):
    """capmi_step_state after capmi_step_set_lr(lr) and `steps` capmi_step_advance(b1, b2) from a zeroed record"""
    b1, b2 = O.f32(b1), O.f32(b2)
    return {'epoch': steps, 'adam_step': steps, 'lr': np.float32(lr), 'bc1': np.float32(1.0 - b1 ** steps),
            'bc2_sqrt': np.float32((1.0 - b2 ** steps) ** 0.5)}


# ------------------------------------------------------------------------------------------------ dropout masks
# one capmi_dropout_masks launch beside what test_dropout_masks_one_launch_equals_four_and_eval_rows reaches (aligned segments of whole
# quads): (count, mask one float off, arm)
DROPOUT_MASKS = [
    (43, False, 'vec tail'),
    (48, True, 'scalar(align)'),
    (43, True, 'scalar(align)'),
    (3, False, 'tail'),
]


def _arm_dropout_masks(c):
    count, off = c[:2]
    if off:
        return 'scalar(align)'
    return ' '.join((['vec'] if count >= 4 else []) + (['tail'] if count % 4 else []))


# ------------------------------------------------------------------------------------------------ arms
TABLES = {'colsum': COLSUM, 'colsum_batch': COLSUM_BATCH, 'group_rowsum': GROUP_ROWSUM, 'embed_fwd': EMBED_FWD, 'embed_bwd': EMBED_BWD,
          'embed_pe_fwd': EMBED_PE_FWD, 'embed_pe_bwd': EMBED_PE_BWD, 'relu_mask_bwd': RELU_MASK_BWD, 'relu_scale_bwd': RELU_SCALE_BWD,
          'adam': ADAM, 'dropout_masks': DROPOUT_MASKS}

# tokens (or whole arms) that some row of the entry's table has to name
REQUIRED = {
    'colsum': ['vec', '4row', '1row', 'scalar(ld%4)', 'scalar(cols%4)', 'scalar(align)', 'scalar(ld%4+cols%4)', 'pitched', 'cblocks=2',
               'cblocks=64', 'rsplit=1', 'rsplit=4', 'memset', 'preloaded', 'acc', 'scalar(cols%4) rsplit=4 memset pitched'],
    'colsum_batch': ['vec', '8row', '4row', '1row', 'scalar(ld%4+cols%4)', 'scalar(align)', 'wrap(batch)', 'wrap(args)', 'out2', 'acc',
                     'pitched'],
    'group_rowsum': ['v4', 'batch8', 'clamped', 'empty', 'wg=2', 'dead', 'slab>', 'scalar(cols%4)', 'scalar(slab%4)', 'scalar(align in)',
                     'scalar(align out)'],
    'embed_fwd': ['it_save', 'relu', 'mask', 'it_save relu mask', 'planes', 'EINVAL'],
    'embed_bwd': ['det', 'idle', 'loop8', 'scan2', 'late', 'y=2', 'norelu', 'nomask', 'lds>64K', 'atomic(Ed%4)', 'atomic(align dx)',
                  'atomic(align dE)', 'atomic(rows>max)'],
    'embed_pe_fwd': ['pos0=0', 'pos0=2', 'drop', 'pos0=0 drop', 'pos0=2'],
    'embed_pe_bwd': ['det', 'nodrop', 'lds>64K', 'atomic(D%4)', 'atomic(rows>max)'],
    'relu_mask_bwd': ['gate mask', 'gate', 'mask', 'copy'],
    'relu_scale_bwd': ['quads', 'EINVAL'],
    'adam': ['adam2', 'two', 'clamped', 'adam_kernel', 'quads', 'tail', 'adam_kernel tail'],
    'dropout_masks': ['vec tail', 'scalar(align)'],
}


def arm(entry, case):
    """the arm that row `case` of TABLES[entry] reaches, from the dispatch predicates of the sources"""
    if entry in ('embed_bwd', 'embed_pe_bwd'):              # the token lists are drawn by the row's index
        i = TABLES[entry].index(case)
        return (_arm_embed_bwd if entry == 'embed_bwd' else _arm_embed_pe_bwd)(case, i)
    return {'colsum': _arm_colsum, 'colsum_batch': _arm_colsum_batch, 'group_rowsum': _arm_group_rowsum, 'embed_fwd': _arm_embed_fwd,
            'embed_pe_fwd': _arm_embed_pe_fwd, 'relu_mask_bwd': _arm_relu_mask_bwd, 'relu_scale_bwd': _arm_relu_scale_bwd,
            'adam': _arm_adam, 'dropout_masks': _arm_dropout_masks}[entry](case)


def names(entry, token):
    """does some row of the entry's table name `token` (a single token, or a whole arm)?"""
    return any(token == row[-1] or token in row[-1].split() for row in TABLES[entry])
