"""float64 restatement of capmi_gemm_f32 (include/capmi.h, "fp32 MFMA GEMM") and the case table that walks every route of its
dispatcher (csrc/gemm_f32.hip).  Shared by tests/test_gemm_routes_host.py (no GPU), tests/test_gemm_routes_gpu.py and
tests/gemm_routes_child.py.  Importing this module needs torch only; the package is imported by descriptor() and run().

The contract restated by evaluate():

    C[M,N] = epi( sum_s opA(A_s)[M,K_s] * opB(B_s)[K_s,N] )
    a_layout 0: A_s stored [M / a_row_div][K_s], operand row r reads stored row r // a_row_div      1: A_s stored [K_s][M]
    b_layout 0: B_s stored [N][K_s]                                                               1: B_s stored [K_s][N]
    v = acc + bias[n] + bias2[n] + row_bias[(m // row_bias_div) * N + n];  relu;  v *= mul_mask[m * N + n];
    v += addend[m * ldc + n]   or, with accumulate and no addend, the previous content of C[m * ldc + n]

How the rows reach their routes: the rules of gemm_plan (csrc/gemm_f32.hip: skinny_ok, plan_lc, plan_ares, plan_tiled), worked out
for this table.  tests/test_gemm_routes_host.py asks capmi_gemm_plan for every row's route without a GPU; the census test in
test_gemm_routes_gpu.py holds the launches to it.
T = sum over segments of ceil(K_s / 32) K tiles, nblk = ceil(N / 128), S = the descriptor's `splits`:

  lc        planes for every segment, M <= 64, a_layout 0, every operand 16-byte aligned, K_s % 4 == 0, a_row_div 1 (b_layout 1:
            N % 4 == 0).  lc_plan with S forced: sl = max(2, ceil(T / S)) chunks per slice, splits = ceil(T / sl).
  ares_*    the same without planes (a_row_div allowed).  ares_ts_cap = 6 chunks per wave with bf16x3 and M > 32, else 9;
            ares_plan(want = nblk * S): ts = min(cap, ceil(ceil(T / S) / 2)), splits = ceil(T / (2 ts)).
            ares_x3       splits <= S, i.e. ceil(T / S) <= 2 * cap.
            ares_f32      M > 32 and 12 S < T <= 18 S: the bf16x3 plan overflows its grid (splits > S), the half-slice plan
                          (cap 3, 2 S slices) needs T <= 12 S and cannot take it, the fp32 image (cap 9) fits.
            ares_x3_half  needs nblk * ceil(T / 12) > want >= ... and nblk * ceil(T / 6) <= 2 * want.  With S forced want is
                          nblk * S exactly and the two conditions contradict (T > 12 S and T <= 12 S); with S = 0 want is 256 and
                          only the floors of 256 / nblk and 512 / nblk leave a gap: nblk = 24, 121 <= T <= 126 is the smallest
                          (nblk * T ~ 3072 always), M > 32.  That is 2 * 33 * 2945 * 3844 = 747 MFLOP, the one shape of this
                          route below 1 GFLOP; its splits are 21, so the route never owns an epilogue (epi is reduce or slabs).
  t32x128   M <= 32 and not eligible above (K % 4 != 0, a_layout 1, or a misaligned operand).
  t64x64    33 <= M <= 64 not eligible above, or M > 64 with M * N < 256 K.
  t64x128   as t64x64 with b_layout 0, T >= 64 and N >= 1024.  M >= 33, N >= 1024, K >= 63 * 32 + 1: at least 136 MFLOP.
  t128      M > 64, M * N >= 256 K, bf16x3 not eligible (K % 4 != 0, a_row_div > 1, a_layout 1 with M % 4 != 0, b_layout 1 with
            N % 4 != 0, or a misaligned operand).
  x3 / x3w / x3w_swap  the planner costs rounds * ceil(T / sp) * step (+ slab traffic, equal for the three) with
            rounds = ceil(out_tiles * sp / 256), step 1 for 128 x 128 tiles and 1.65 for 256 x 128: a wide tiling wins exactly when
            the narrow one needs two rounds and the wide one a single round.  Four segments of K = 4 give T = 4 K tiles for 16 k:
            x3w        >= four 256-row tiles: (1540, 516) has 65 narrow / 35 wide tiles, S = 4 -> 260 vs 140 units; without a split
                       (2052, 2048, K = 4): 272 vs 144.
            x3w_swap   a_layout 0, < four 256-row tiles, >= four 256-column tiles: (68, 8196) 65 vs 33 tiles with S = 4; without a
                       split (68, 32772, K = 4): 257 vs 129 -- the planner does choose it with epi=kernel.
            x3         everything else that is bf16x3-eligible; (516, 512, 36) has three 256-row and two 256-column tiles.

No row exceeds FLOP_CAP except the rows of CAP_EXEMPT: the two routes whose smallest shape is larger, as derived above.
"""
import torch

COUNTER_FLOATS = 16384            # capmi.h CAPMI_WS_COUNTER_FLOATS
MAX_SEG = 4                       # capmi.h CAPMI_MAX_SEG
WS_FLOATS = 4 * 1024 * 1024       # slab floats of the workspace the tests allocate
FLOP_CAP = 64e6
WINDOW_PAD = 12                   # ldc = N + 12 (+ 1 on the rows that ask for ldc % 4 != 0)
ROUTES = ('lc', 'ares_x3', 'ares_x3_half', 'ares_f32', 't32x128', 't64x64', 't64x128', 't128', 'x3', 'x3w', 'x3w_swap')
# routes whose kernel can apply the epilogue itself (ares_x3_half: see the module docstring)
OWNS_EPILOGUE = tuple(r for r in ROUTES if r != 'ares_x3_half')
# route -> smallest FLOP count at which the dispatcher takes it (module docstring); rows of these routes may reach 1.1 x that
CAP_EXEMPT = {'t64x128': 2.0 * 33 * 1024 * (63 * 32 + 1), 'ares_x3_half': 2.0 * 33 * 2945 * 3844}

FULL = dict(bias=True, bias2=True, row_bias=5, relu=True, mask=True)
CASES = []


def make_case(name, route, epi, M, N, Ks, al=0, bl=0, divs=None, lda_pad=0, ldb_pad=0, a_off=0, splits=1, planes=False, bcols=None,
              bias=False, bias2=False, row_bias=0, relu=False, mask=False, acc=None, eoff=0, c_off=8, ldc_pad=WINDOW_PAD,
              allow_wide=False, seed=0):
    """acc: None, 'C' (accumulate into the window's previous content) or 'addend'.  eoff: element offset of the bias / bias2 /
    row_bias / mask / addend pointers off their 16-byte aligned buffers.  divs: a_row_div per segment.  row_bias: its divisor, 0 = none.
    epi 'slabs' is a deferred call (defer_reduce)."""
    Ks = (Ks,) if isinstance(Ks, int) else tuple(Ks)
    return dict(name=name, route=route, epi=epi, M=M, N=N, Ks=Ks, al=al, bl=bl, divs=tuple(divs or (1,) * len(Ks)),
                lda_pad=lda_pad, ldb_pad=ldb_pad, a_off=a_off, splits=splits, planes=planes, bcols=bcols, bias=bias, bias2=bias2,
                row_bias=row_bias, relu=relu, mask=mask, acc=acc, eoff=eoff, c_off=c_off, ldc=N + ldc_pad,
                defer=epi == 'slabs', allow_wide=allow_wide, seed=seed)


def _case(*args, **kw):
    CASES.append(make_case(*args, seed=1000 + len(CASES), **kw))


K4x4 = (4, 4, 4, 4)
MIS = dict(eoff=1, c_off=5, ldc_pad=WINDOW_PAD + 1)        # epilogue operands one float off 16 bytes, ldc % 4 != 0 where N % 4 == 0

# ---- LDS-tiled fp32 MFMA, 32 x 128 (M <= 32) -------------------------------------------------------------------------------------
_case('t32_tiny', 't32x128', 'kernel', 3, 5, 7)
_case('t32_edge_full_acc', 't32x128', 'kernel', 32, 129, 33, acc='C', **FULL)
_case('t32_nn_full_add', 't32x128', 'kernel', 17, 130, 35, bl=1, acc='addend', **FULL)
_case('t32_tt', 't32x128', 'kernel', 13, 6, 9, al=1, bl=1, bias=True)
_case('t32_tn_pitch', 't32x128', 'kernel', 31, 127, 36, al=1, lda_pad=3, ldb_pad=5, mask=True, acc='C')
_case('t32_reduce_full_add', 't32x128', 'reduce', 31, 127, 67, splits=2, acc='addend', **FULL)
_case('t32_slabs', 't32x128', 'slabs', 31, 127, 67, splits=2)
# ---- 64 x 64 ---------------------------------------------------------------------------------------------------------------------
_case('t64_full_acc', 't64x64', 'kernel', 33, 70, 50, acc='C', **FULL)
_case('t64_fat_full_add', 't64x64', 'kernel', 131, 257, 100, acc='addend', **FULL)
_case('t64_misaligned_a', 't64x64', 'kernel', 40, 64, 64, a_off=1, bias=True, relu=True)
_case('t64_rowdiv', 't64x64', 'kernel', 66, 65, (40, 31), divs=(3, 1), row_bias=5, acc='C')
_case('t64_tn', 't64x64', 'kernel', 100, 63, 37, al=1, bias2=True, mask=True)
_case('t64_tt', 't64x64', 'kernel', 65, 129, 33, al=1, bl=1, acc='C')
_case('t64_reduce_full_acc', 't64x64', 'reduce', 63, 65, 131, splits=2, acc='C', **FULL)
_case('t64_slabs', 't64x64', 'slabs', 65, 63, 97, splits=3)
# ---- 64 x 128: long-K weight streams with N >= 1024 (CAP_EXEMPT) --------------------------------------------------------------------
_case('t64w_full_acc', 't64x128', 'kernel', 33, 1025, 2017, acc='C', **FULL)
_case('t64w_reduce_full_add', 't64x128', 'reduce', 33, 1025, 2017, splits=2, acc='addend', **FULL)
_case('t64w_slabs', 't64x128', 'slabs', 33, 1024, 2017, splits=2)
# ---- 128 x 128 -------------------------------------------------------------------------------------------------------------------
_case('t128_full_acc', 't128', 'kernel', 516, 512, 34, acc='C', **FULL)
_case('t128_tn_odd_m_full_add', 't128', 'kernel', 517, 512, 36, al=1, acc='addend', **FULL)
_case('t128_rowdiv', 't128', 'kernel', 516, 512, 36, divs=(3,), bias=True, acc='C')
_case('t128_nn_odd_n', 't128', 'kernel', 516, 513, 36, bl=1, mask=True)
_case('t128_reduce_full_acc', 't128', 'reduce', 513, 515, 67, splits=2, acc='C', **FULL)
_case('t128_slabs', 't128', 'slabs', 513, 515, 67, splits=3)
# ---- persistent bf16x3, 128 x 128 ------------------------------------------------------------------------------------------------
_case('x3_nt_full_acc', 'x3', 'kernel', 516, 512, 36, acc='C', **FULL)
_case('x3_nn_full_add', 'x3', 'kernel', 516, 512, 36, bl=1, lda_pad=4, ldb_pad=8, acc='addend', **FULL)
_case('x3_tn_bias_relu', 'x3', 'kernel', 516, 512, 36, al=1, bias=True, bias2=True, relu=True)
_case('x3_tt_mask_acc', 'x3', 'kernel', 516, 512, 36, al=1, bl=1, lda_pad=8, ldb_pad=4, mask=True, acc='C')
_case('x3_wide_n', 'x3', 'kernel', 260, 1028, 36, bias=True, mask=True, acc='addend')
_case('x3_max_seg', 'x3', 'kernel', 516, 512, (36, 4, 32, 8), relu=True, mask=True, acc='C')
_case('x3_reduce_full_acc', 'x3', 'reduce', 516, 512, 36, splits=2, acc='C', **FULL)
_case('x3_reduce_full_acc_misaligned', 'x3', 'reduce', 516, 512, 36, splits=2, acc='C', **FULL, **MIS)
_case('x3_reduce_full_add_misaligned', 'x3', 'reduce', 516, 512, 36, splits=2, acc='addend', **FULL, **MIS)
_case('x3_slabs', 'x3', 'slabs', 516, 512, 68, al=1, bl=1, splits=3)
# ---- bf16x3, 256 x 128 -----------------------------------------------------------------------------------------------------------
_case('x3w_full_acc', 'x3w', 'kernel', 2052, 2048, 4, splits=0, acc='C', **FULL)
_case('x3w_reduce_full_add', 'x3w', 'reduce', 1541, 516, K4x4, splits=4, acc='addend', **FULL)
_case('x3w_tt_weight_grad', 'x3w', 'reduce', 1540, 516, K4x4, al=1, bl=1, splits=4, acc='C')
_case('x3w_slabs', 'x3w', 'slabs', 1540, 516, K4x4, al=1, bl=1, splits=4, allow_wide=True)
# ---- bf16x3, 256 x 128 on the swapped product (x3_epilogue_t) ---------------------------------------------------------------------
_case('x3ws_full_add', 'x3w_swap', 'kernel', 68, 32772, 4, splits=0, acc='addend', **FULL)
_case('x3ws_full_acc_misaligned', 'x3w_swap', 'kernel', 68, 32772, 4, splits=0, acc='C', **FULL, **MIS)
_case('x3ws_odd_n_full_acc', 'x3w_swap', 'kernel', 68, 32771, 4, splits=0, acc='C', **FULL)
_case('x3ws_reduce_full_acc', 'x3w_swap', 'reduce', 68, 8196, K4x4, splits=4, acc='C', **FULL)
_case('x3ws_reduce_full_acc_misaligned', 'x3w_swap', 'reduce', 68, 8196, K4x4, splits=4, acc='C', **FULL, **MIS)
_case('x3ws_nn_reduce', 'x3w_swap', 'reduce', 68, 8196, K4x4, bl=1, splits=4, bias=True, relu=True)
_case('x3ws_slabs', 'x3w_swap', 'slabs', 68, 8196, K4x4, splits=4)
_case('x3ws_slabs_odd_n', 'x3w_swap', 'slabs', 68, 8197, K4x4, splits=4)
# ---- A-resident (M <= 64, aligned, K % 4 == 0, no planes) ---------------------------------------------------------------------------
_case('ares_x3_full_acc', 'ares_x3', 'kernel', 33, 129, 36, acc='C', **FULL)
_case('ares_x3_nn_full_add', 'ares_x3', 'kernel', 64, 132, 68, bl=1, lda_pad=4, ldb_pad=4, acc='addend', **FULL)
_case('ares_x3_small', 'ares_x3', 'kernel', 5, 40, 8, bias=True)
_case('ares_x3_rowdiv', 'ares_x3', 'kernel', 34, 130, (36, 32), divs=(1, 3), row_bias=5, mask=True, acc='C')
_case('ares_x3_max_seg', 'ares_x3', 'kernel', 31, 127, (4, 36, 8, 32), divs=(1, 2, 1, 1), bias2=True, relu=True)
_case('ares_x3_reduce_full_acc', 'ares_x3', 'reduce', 33, 132, 100, splits=2, acc='C', **FULL)
_case('ares_x3_slabs', 'ares_x3', 'slabs', 33, 129, 100, splits=2)
_case('ares_f32_full_acc', 'ares_f32', 'kernel', 41, 200, 420, acc='C', **FULL)
_case('ares_f32_nn_full_add', 'ares_f32', 'kernel', 64, 132, 420, bl=1, acc='addend', **FULL)
_case('ares_f32_reduce_full_add', 'ares_f32', 'reduce', 41, 200, 804, splits=2, acc='addend', **FULL)
_case('ares_f32_slabs', 'ares_f32', 'slabs', 41, 200, 804, splits=2)
_case('ares_x3_half_full_acc', 'ares_x3_half', 'reduce', 33, 2945, 3844, splits=0, acc='C', **FULL)      # (CAP_EXEMPT)
# ---- loader / consumer (the same with planes from ops.planes_from_f32) --------------------------------------------------------------
_case('lc_full_acc', 'lc', 'kernel', 33, 129, 36, planes=True, acc='C', **FULL)
_case('lc_nn_full_add', 'lc', 'kernel', 64, 132, 68, bl=1, planes=True, lda_pad=4, ldb_pad=4, acc='addend', **FULL)
_case('lc_small_two_seg', 'lc', 'kernel', 7, 37, (8, 36), planes=True, bias=True, relu=True)
_case('lc_colseg_full_add', 'lc', 'kernel', 40, 200, 68, bl=1, planes=True, bcols=(132, 64, 4), acc='addend', **FULL)
_case('lc_reduce_full_acc', 'lc', 'reduce', 33, 132, 100, splits=2, planes=True, acc='C', **FULL)
_case('lc_slabs', 'lc', 'slabs', 33, 129, 100, splits=2, planes=True)

BY_NAME = {c['name']: c for c in CASES}


def flops(c):
    return 2.0 * c['M'] * c['N'] * sum(c['Ks'])


def k_tiles(c):
    return sum((k + 31) // 32 for k in c['Ks'])


def slab_floats_bound(c):
    """upper bound of the slab floats a row can ask for: the library never writes more K slices than K tiles, and the auto plans
    (splits 0) of this table stay at or below 21 (ares_x3_half)"""
    sp = min(c['splits'] if c['splits'] > 0 else 21, k_tiles(c))
    return sp * c['M'] * c['N'] if sp > 1 or c['defer'] else 0


def sentinel(n):
    """finite, exactly representable, small enough not to drown an accumulate row's error: (i * 37 % 101 - 50) / 64"""
    i = torch.arange(n, dtype=torch.int64)
    return ((i * 37 % 101 - 50).to(torch.float32)) / 64


def draw(c):
    """host tensors of a row, drawn as the kernel tests draw theirs (activations N(0,1), weights scaled by 0.1, mask in {0, 2}).  Every
    operand lives in a flat buffer at its element offset, pitch padding included (finite values: a kernel that reads it is wrong)."""
    g = torch.Generator().manual_seed(c['seed'])
    M, N, al, bl = c['M'], c['N'], c['al'], c['bl']
    t = dict(A=[], B=[], Bc=[])
    for K, div in zip(c['Ks'], c['divs']):
        rows, cols = ((M + div - 1) // div, K) if al == 0 else (K, M)
        t['A'].append(torch.randn(c['a_off'] + rows * (cols + c['lda_pad']), generator=g))
        rows, cols = (N, K) if bl == 0 else (K, N)
        t['B'].append(torch.randn(rows * (cols + c['ldb_pad']), generator=g) * 0.1)
    if c['bcols']:
        K = c['Ks'][0]
        t['Bc'] = [torch.randn(K * (n + 4), generator=g) * 0.1 for n in c['bcols']]
    e = c['eoff']
    if c['bias']:
        t['bias'] = torch.randn(e + N, generator=g)
    if c['bias2']:
        t['bias2'] = torch.randn(e + N, generator=g)
    if c['row_bias']:
        t['row_bias'] = torch.randn(e + (M + c['row_bias'] - 1) // c['row_bias'] * N, generator=g)
    if c['mask']:
        t['mask'] = (torch.rand(e + M * N, generator=g) < 0.5).float() * 2
    if c['acc'] == 'addend':
        t['addend'] = torch.randn(e + M * c['ldc'], generator=g)
    t['C'] = sentinel(c['c_off'] + M * c['ldc'] + 64)
    return t


def to_device(t, dev):
    return {k: [x.to(dev) for x in v] if isinstance(v, list) else v.to(dev) for k, v in t.items()}


def _view(buf, off, rows, cols, ld):
    return torch.as_strided(buf, (rows, cols), (ld, 1), off)


def operands(c, t):
    """[(A [M, K_s], B [K_s, N])] as the descriptor defines them, in the dtype of t"""
    M, N, al, bl = c['M'], c['N'], c['al'], c['bl']
    out = []
    for s, (K, div) in enumerate(zip(c['Ks'], c['divs'])):
        if al == 0:
            A = _view(t['A'][s], c['a_off'], (M + div - 1) // div, K, K + c['lda_pad'])
            A = A[torch.arange(M, device=A.device) // div]              # operand row r reads stored row r // a_row_div
        else:
            A = _view(t['A'][s], c['a_off'], K, M, M + c['lda_pad']).t()
        if c['bcols']:
            B = torch.cat([_view(b, 0, K, n, n + 4) for b, n in zip(t['Bc'], c['bcols'])], 1)
        elif bl == 0:
            B = _view(t['B'][s], 0, N, K, K + c['ldb_pad']).t()
        else:
            B = _view(t['B'][s], 0, K, N, N + c['ldb_pad'])
        out.append((A, B))
    return out


def window(c, buf):
    return _view(buf, c['c_off'], c['M'], c['N'], c['ldc'])


def evaluate(c, t, dtype, raw=False):
    """the contract in `dtype`, and the same formula on absolute values.  raw: the product alone (what the slabs of a deferred call sum
    to).  t['C'] is the buffer BEFORE the call."""
    M, N, e = c['M'], c['N'], c['eoff']
    t = {k: [x.to(dtype) for x in v] if isinstance(v, list) else v.to(dtype) for k, v in t.items()}
    v = torch.zeros(M, N, dtype=dtype, device=t['C'].device)
    mag = torch.zeros_like(v)
    for A, B in operands(c, t):
        v = v + A @ B
        mag = mag + A.abs() @ B.abs()
    if raw:
        return v, mag
    for key in ('bias', 'bias2'):
        if c[key]:
            v = v + t[key][e:e + N]
            mag = mag + t[key][e:e + N].abs()
    if c['row_bias']:
        rb = t['row_bias'][e:].view(-1, N)[torch.arange(M, device=v.device) // c['row_bias']]
        v, mag = v + rb, mag + rb.abs()
    if c['relu']:
        v = torch.relu(v)
    if c['mask']:
        mk = t['mask'][e:e + M * N].view(M, N)
        v, mag = v * mk, mag * mk.abs()
    if c['acc'] == 'addend':
        ad = _view(t['addend'], e, M, N, c['ldc'])
        v, mag = v + ad, mag + ad.abs()
    elif c['acc'] == 'C':
        ad = window(c, t['C'])
        v, mag = v + ad, mag + ad.abs()
    return v, mag


def gemm64(c, t):
    """(reference, mag) in float64"""
    return evaluate(c, t, torch.float64)


def measure(out, ref, mag):
    """max over the window of |out - ref| / mag.  Where mag is 0 (a masked element without an addend) every term of the formula
    is 0 and the output has to be exactly 0: such an element counts as infinite error unless it is."""
    err = (out.double() - ref).abs()
    zero = mag == 0
    ratio = torch.where(zero, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float('inf'))),
                        err / torch.where(zero, torch.ones_like(mag), mag))
    return float(ratio.max())


def descriptor(c, buf, planes, ws):
    """the capmi_gemm_desc of a row, filled by ops.gemm.  buf(key, s=None): the flat buffer of draw()'s t[key] (t[key][s] for the
    per-segment lists) -- a device tensor, or anything else with a data_ptr(): the planner reads the descriptor only, so an address
    that nothing dereferences will do; planes: one per segment, or None; ws: an ops.Workspace (or its .buf / .capacity)."""
    from imagecaptioning.pytorch_amd import ops
    M, N, al, bl, e = c['M'], c['N'], c['al'], c['bl'], c['eoff']
    segs = []
    for s, (K, div) in enumerate(zip(c['Ks'], c['divs'])):
        lda = (K if al == 0 else M) + c['lda_pad']
        ldb = (K if bl == 0 else N) + c['ldb_pad']
        segs.append(((buf('A', s), c['a_off']), lda, None if c['bcols'] else buf('B', s), ldb, K, div))
    epi = lambda key, on: Shifted(buf(key), e) if on else None                      # noqa: E731
    return ops.gemm(segs, M, N, (buf('C'), c['c_off']), ldc=c['ldc'], a_layout=al, b_layout=bl, bias=epi('bias', c['bias']),
                    bias2=epi('bias2', c['bias2']), row_bias=epi('row_bias', c['row_bias']), row_bias_div=c['row_bias'] or 1,
                    mul_mask=epi('mask', c['mask']), relu=c['relu'], accumulate=c['acc'] == 'C',
                    addend=epi('addend', c['acc'] == 'addend'), ws=ws, splits=c['splits'], defer_reduce=c['defer'],
                    a_planes=planes, allow_wide=c['allow_wide'],
                    b_cols=[(buf('Bc', i), n + 4, n) for i, n in enumerate(c['bcols'])] if c['bcols'] else None, desc_only=True)


class Shifted:
    """a buffer from its element `off` on (what buf[off:] is for a tensor), for buffers that only have a data_ptr()"""

    def __init__(self, buf, off):
        self.addr = buf.data_ptr() + 4 * off

    def data_ptr(self):
        return self.addr


def device_descriptor(c, t, ws):
    """descriptor() on device tensors t, with A planes made from the activations where the row asks for them"""
    from imagecaptioning.pytorch_amd import ops
    planes = None
    if c['planes']:
        planes = [ops.planes_from_f32(_view(t['A'][s], c['a_off'], c['M'], K, K + c['lda_pad'])) for s, K in enumerate(c['Ks'])]
    d = descriptor(c, lambda key, s=None: t[key] if s is None else t[key][s], planes, ws)
    d.keep = planes                   # (the descriptor holds addresses only)
    return d


def run(d):
    """capmi_gemm_f32 on the current stream (t['C'] is written).  Returns splits_used."""
    import ctypes
    from imagecaptioning.pytorch_amd import _lib
    _lib.check(_lib.lib.capmi_gemm_f32(ctypes.byref(d), _lib.stream_ptr()), 'capmi_gemm_f32')
    return d.splits_used


def run_case(c, t, ws):
    """the call itself, on device tensors t.  Returns splits_used."""
    return run(device_descriptor(c, t, ws))
