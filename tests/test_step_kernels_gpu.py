"""The per-step kernels through the C ABI against the float64 references of step_kernels_ref64.py, one case per dispatch branch
(16-byte vs scalar, register-resident vs streaming, rows per workgroup, column splits, fused vs separate slab reduce): the case
tables there say which branch a row is meant to reach.  Metric and bounds are those of test_kernels_gpu.py: rel_err =
max|got - ref| / max|ref| with cell forward 2e-6, cell backward 5e-6, attention forward 5e-6, attention backward 2e-5; the planted
row of extremes of every cell case is left out of that maximum (its 1e4 entries would set the scale) and compared elementwise as
|got - ref| <= tol * (1 + |ref|) instead.  The sentinel attention of AdaAtt (three entry points, each fed float64-derived inputs so that
no kernel absorbs another's error) holds the plain attention's bounds unwidened; every output of those tests is NaN-filled and
followed by a guard tail that the launch must leave alone."""
import numpy as np
import pytest
import torch

import step_kernels_ref64 as S
from oracle import planes as PL

pytestmark = pytest.mark.gpu

CELL_FWD, CELL_BWD, ATT_FWD, ATT_BWD = 2e-6, 5e-6, 5e-6, 2e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def L():
    from imagecaptioning.pytorch_amd import _lib
    return _lib


def put(dev, t, off=False):
    """the tensor on the device; off: in a view that starts one float past a 16-byte boundary"""
    if t is None:
        return None
    if not off:
        return t.to(dev).contiguous()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def ptr(t):
    return None if t is None else t.data_ptr()


class Keep:
    """device copies handed to a call as bare pointers stay alive here until the test ends"""
    def __init__(self, dev):
        self.dev, self.held = dev, []

    def __call__(self, t):
        self.held.append(put(self.dev, t))
        return ptr(self.held[-1])


def nan(dev, *shape):
    return torch.full(shape, float('nan'), device=dev)


def rel_err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


def check(name, got, ref, tol, plant=None, skip=None):
    torch.cuda.synchronize()
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    if skip is not None:
        err = err.masked_fill(skip, 0.0)
    rows = [r for r in range(ref.shape[0]) if r != plant] if (plant is not None and ref.shape[0] > 1) else list(range(ref.shape[0]))
    e = float(err[rows].max() / (ref[rows].abs().max() + 1e-30))
    print('%s rel_err %.2e (bound %.0e)' % (name, e, tol))
    assert e < tol, (name, e)
    if plant is not None:
        over = err[plant] - tol * (1.0 + ref[plant].abs())
        assert float(over.max()) <= 0.0, (name, 'planted row', int(over.argmax()), float(err[plant].max()))


def planes_buf(dev, k):
    return torch.zeros(int(L().lib.capmi_planes_bytes(k)), dtype=torch.uint8, device=dev)


def same_planes(pl, x):
    torch.cuda.synchronize()
    assert np.array_equal(pl.cpu().numpy(), PL.planes_from_f32(x.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ LSTM cell
@pytest.mark.parametrize('i', range(len(S.LSTM_FWD)))
def test_lstm_cell_fwd(dev, i):
    N, R, s1, s2, flags, _ = S.LSTM_FWD[i]
    fl = set(flags.split())
    d = S.cell_inputs('lstm', N, R, s1, s2, flags, seed=i)
    t = {k: put(dev, d[k], 'off:' + k in fl) for k in ('partial', 'partial2', 'b1', 'b2', 'row_bias', 'c_prev', 'mask')}
    idx = put(dev, d['row_idx'])
    h, c, hd = nan(dev, N, R), nan(dev, N, R), nan(dev, N, R)
    ga = None if 'noga' in fl else nan(dev, N, 4 * R)
    pl_h, pl_hd = (planes_buf(dev, R), planes_buf(dev, R)) if 'planes' in fl else (None, None)
    lib = L().lib
    L().check(lib.capmi_lstm_cell_fwd_pl2(ptr(t['partial']), s1, ptr(t['partial2']), s2, ptr(t['b1']), ptr(t['b2']), ptr(t['row_bias']),
                                          d['row_div'], ptr(idx), ptr(t['c_prev']), ptr(h), ptr(c), ptr(ga), ptr(t['mask']), ptr(hd),
                                          N, R, ptr(pl_h), ptr(pl_hd), L().stream_ptr()), 'lstm_cell_fwd_pl2')
    h_ref, c_ref, g_ref = S.lstm_point(d['pre'], d['c_prev'].double())
    p = d['plant']
    check('h', h, h_ref, CELL_FWD, p)
    check('c', c, c_ref, CELL_FWD, p)
    check('h_drop', hd, h_ref * d['mask'].double() if d['mask'] is not None else h_ref, CELL_FWD, p)
    if ga is not None:
        check('gates_act', ga, g_ref, CELL_FWD, p)
    if pl_h is not None:
        same_planes(pl_h, h)
        same_planes(pl_hd, hd)


def test_lstm_cell_planes_need_at_most_64_rows(dev):
    N, R = 65, 36
    z = torch.zeros(N, 4 * R, device=dev)
    o = [torch.zeros(N, R, device=dev) for _ in range(4)]
    lib = L().lib
    rc = lib.capmi_lstm_cell_fwd_pl2(ptr(z), 1, None, 0, None, None, None, 1, None, ptr(o[0]), ptr(o[1]), ptr(o[2]), None, None, ptr(o[3]),
                                     N, R, ptr(planes_buf(dev, R)), None, L().stream_ptr())
    assert rc == L().EINVAL
    rc = lib.capmi_lstm_cell_bwd_partial_pl(ptr(o[0]), R, None, None, 0, 1, 0, None, 0, 1, 0, None, ptr(z), ptr(o[1]), ptr(o[2]),
                                            ptr(torch.zeros_like(z)), ptr(o[3]), N, R, ptr(planes_buf(dev, 4 * R)), L().stream_ptr())
    assert rc == L().EINVAL


def slab_operand(g, dev, splits, N, R, pad, off=False):
    """`splits` slabs of a [N, R] matrix with row pitch R + pad and slab stride N * (R + pad) + 8 floats -> (device, ld, stride, sum)"""
    ld = R + pad
    stride = N * ld + 8
    raw = (torch.randn(splits, stride, generator=g) / splits ** 0.5).float()
    val = raw[:, :N * ld].view(splits, N, ld)[:, :, :R].double().sum(0)
    return put(dev, raw, off), ld, stride, val


@pytest.mark.parametrize('i', range(len(S.LSTM_BWD)))
def test_lstm_cell_bwd(dev, i):
    kp = Keep(dev)
    N, R, pad_a, mask_a, nb, nc, pad_bc, has_dc, flags, _ = S.LSTM_BWD[i]
    fl = set(flags.split())
    d = S.cell_inputs('lstm', N, R, 1, 0, 'bih', seed=50 + i)
    g = S.gen(500 + i)
    cp = d['c_prev'].double()
    _, c_ref, g_ref = S.lstm_point(d['pre'], cp)
    dh = torch.zeros(N, R, dtype=torch.float64)
    a = am = None
    if 'noa' not in fl:
        a = torch.randn(N, R + pad_a, generator=g).float()
        am = ((torch.rand(N, R, generator=g) < 0.5).float() * 2) if mask_a else None
        dh = dh + a[:, :R].double() * (am.double() if mask_a else 1.0)
    b = ldb = sb = c_ = ldc = sc = None
    if nb:
        b, ldb, sb, v = slab_operand(g, dev, nb, N, R, pad_bc, 'off:dh_b' in fl)
        dh = dh + v
    if nc:
        c_, ldc, sc, v = slab_operand(g, dev, nc, N, R, pad_bc)
        dh = dh + v
    dc = torch.randn(N, R, generator=g).float() if has_dc else None
    ref_dg, ref_dcp = S.cell_backward(S.lstm_point, d['pre'], cp, dh, None if dc is None else dc.double())
    dg, dcp = nan(dev, N, 4 * R), nan(dev, N, R)
    pl = planes_buf(dev, 4 * R) if 'planes' in fl else None
    L().check(L().lib.capmi_lstm_cell_bwd_partial_pl(kp(a), R + pad_a, kp(am), ptr(b), ldb or 0, nb or 1, sb or 0,
                                                     ptr(c_), ldc or 0, nc or 1, sc or 0, kp(dc), kp(g_ref.float()),
                                                     kp(d['c_prev']), kp(c_ref.float()), ptr(dg), ptr(dcp), N, R,
                                                     ptr(pl), L().stream_ptr()), 'lstm_cell_bwd_partial_pl')
    check('d_gates', dg, ref_dg, CELL_BWD, d['plant'])
    check('dc_prev', dcp, ref_dcp, CELL_BWD, d['plant'])
    if pl is not None:
        same_planes(pl, dg)
    if i == 1:      # the same operands through the entry point without planes
        dg2, dcp2 = nan(dev, N, 4 * R), nan(dev, N, R)
        L().check(L().lib.capmi_lstm_cell_bwd_partial(kp(a), R + pad_a, kp(am), ptr(b), ldb, nb, sb, None, 0, 1, 0,
                                                      kp(dc), kp(g_ref.float()), kp(d['c_prev']),
                                                      kp(c_ref.float()), ptr(dg2), ptr(dcp2), N, R, L().stream_ptr()), 'bwd_partial')
        check('d_gates (no planes)', dg2, ref_dg, CELL_BWD, d['plant'])


# ------------------------------------------------------------------------------------------------ maxout / att2in2 cell
@pytest.mark.parametrize('i', range(len(S.MAXOUT_FWD)))
def test_maxout_cell_fwd(dev, i):
    N, R, s1, s2, flags, _ = S.MAXOUT_FWD[i]
    fl = set(flags.split())
    d = S.cell_inputs('maxout', N, R, s1, s2, flags, seed=100 + i)
    t = {k: put(dev, d[k]) for k in ('partial', 'partial2', 'b1', 'b2', 'addend', 'ba2c', 'c_prev', 'mask')}
    h, c, hd, sv = nan(dev, N, R), nan(dev, N, R), nan(dev, N, R), nan(dev, N, 5 * R)
    lib = L().lib
    if s2 == 0 and not (fl & {'addend', 'ba2c'}):
        L().check(lib.capmi_maxout_cell_fwd(ptr(t['partial']), s1, ptr(t['b1']), ptr(t['b2']), ptr(t['c_prev']), ptr(h), ptr(c), ptr(sv),
                                            ptr(t['mask']), ptr(hd), N, R, L().stream_ptr()), 'maxout_cell_fwd')
    else:
        L().check(lib.capmi_att2in2_cell_fwd(ptr(t['partial']), s1, ptr(t['partial2']), s2, ptr(t['addend']), ptr(t['b1']), ptr(t['b2']),
                                             ptr(t['ba2c']), ptr(t['c_prev']), ptr(h), ptr(c), ptr(sv), ptr(t['mask']), ptr(hd), N, R,
                                             L().stream_ptr()), 'att2in2_cell_fwd')
    h_ref, c_ref, s_ref = S.maxout_point(d['pre'], d['c_prev'].double())
    p = d['plant']
    check('h', h, h_ref, CELL_FWD, p)
    check('c', c, c_ref, CELL_FWD, p)
    check('saved', sv, s_ref, CELL_FWD, p)
    check('h_drop', hd, h_ref * d['mask'].double() if d['mask'] is not None else h_ref, CELL_FWD, p)


def tie_skip(pre, R, blocks):
    tie = S.tie_mask(pre, R)
    assert float(tie.double().mean()) <= S.TIE_CAP
    skip = torch.zeros(pre.shape[0], blocks * R, dtype=torch.bool)
    skip[:, 3 * R:4 * R] = tie
    skip[:, 4 * R:5 * R] = tie
    return skip


@pytest.mark.parametrize('i', range(len(S.MAXOUT_BWD)))
def test_maxout_cell_bwd(dev, i):
    kp = Keep(dev)
    N, R, nb, mask_a, has_dc, entry, _ = S.MAXOUT_BWD[i]
    d = S.cell_inputs('maxout', N, R, 1, 0, 'bih', seed=200 + i)
    g = S.gen(600 + i)
    cp = d['c_prev'].double()
    _, c_ref, s_ref = S.maxout_point(d['pre'], cp)
    a = torch.randn(N, R, generator=g).float()
    am = ((torch.rand(N, R, generator=g) < 0.5).float() * 2) if mask_a else None
    dh = a.double() * (am.double() if mask_a else 1.0)
    b = None
    stride = N * R + (0 if entry == 'maxout' else 8)
    if nb:
        raw = (torch.randn(nb, stride, generator=g) / nb ** 0.5).float()
        dh = dh + raw[:, :N * R].double().sum(0).view(N, R)
        b = put(dev, raw)
    dc = torch.randn(N, R, generator=g).float() if has_dc else None
    ref_ds, ref_dcp = S.cell_backward(S.maxout_point, d['pre'], cp, dh, None if dc is None else dc.double())
    ds, dcp = nan(dev, N, 5 * R), nan(dev, N, R)
    common = (kp(dc), kp(s_ref.float()), kp(d['c_prev']), kp(c_ref.float()), ptr(ds), ptr(dcp),
              N, R, L().stream_ptr())
    lib = L().lib
    if entry == 'maxout':
        L().check(lib.capmi_maxout_cell_bwd(kp(a), kp(am), ptr(b), *common), 'maxout_cell_bwd')
    else:
        L().check(lib.capmi_att2in2_cell_bwd(kp(a), kp(am), ptr(b), nb or 1, stride, *common), 'att2in2_cell_bwd')
        if nb:
            assert lib.capmi_att2in2_cell_bwd(kp(a), kp(am), ptr(b), nb, N * R - 1, *common) == L().EINVAL
    check('d_sums', ds, ref_ds, CELL_BWD, d['plant'], tie_skip(d['pre'], R, 5))
    check('dc_prev', dcp, ref_dcp, CELL_BWD, d['plant'])


# ------------------------------------------------------------------------------------------------ adaatt cell
@pytest.mark.parametrize('i', range(len(S.ADAATT)))
def test_adaatt_cell_fwd_bwd(dev, i):
    kp = Keep(dev)
    N, R, mo, splits, flags, _ = S.ADAATT[i]
    d = S.cell_inputs('adaattmo' if mo else 'adaatt', N, R, splits, 0, flags, seed=300 + i)
    W, p = d['W'], d['plant']
    t = {k: put(dev, d[k]) for k in ('partial', 'addend', 'fc_gates', 'c_prev', 'mask', 'mask2')}
    h, c, hd, fd, sv = nan(dev, N, R), nan(dev, N, R), nan(dev, N, R), nan(dev, N, R), nan(dev, N, W)
    lib = L().lib
    L().check(lib.capmi_adaatt_cell_fwd(ptr(t['partial']), splits, ptr(t['addend']), ptr(t['fc_gates']), d['n'], ptr(t['c_prev']), ptr(h),
                                        ptr(c), ptr(sv), ptr(t['mask']), ptr(t['mask2']), ptr(hd), ptr(fd), N, R, mo, L().stream_ptr()),
              'adaatt_cell_fwd')
    cp = d['c_prev'].double()
    point = lambda a, b: S.adaatt_point(a, b, mo)      # noqa: E731
    h_ref, c_ref, f_ref, s_ref = point(d['pre'], cp)
    m1 = d['mask'].double() if d['mask'] is not None else 1.0
    m2 = d['mask2'].double() if d['mask2'] is not None else 1.0
    for name, got, ref in (('h', h, h_ref), ('c', c, c_ref), ('saved', sv, s_ref), ('h_drop', hd, h_ref * m1), ('fake_drop', fd, f_ref * m2)):
        check(name, got, ref, CELL_FWD, p)
    if d['fc_gates'] is not None and N % 5:
        assert lib.capmi_adaatt_cell_fwd(ptr(t['partial']), splits, None, ptr(t['fc_gates']), 5, ptr(t['c_prev']), ptr(h), ptr(c), ptr(sv),
                                         None, None, ptr(hd), ptr(fd), N, R, mo, L().stream_ptr()) == L().EINVAL
    # backward on the float32 roundings of the reference's saved activations
    g = S.gen(700 + i)
    a, df, dc = (torch.randn(N, R, generator=g).float() for _ in range(3))
    dh = a.double() * m1
    b, nb, stride = None, 2 * (i % 2), N * R + 8
    if nb:
        raw = (torch.randn(nb, stride, generator=g) / nb ** 0.5).float()
        dh = dh + raw[:, :N * R].double().sum(0).view(N, R)
        b = put(dev, raw)
    ref_ds, ref_dcp = S.cell_backward(point, d['pre'], cp, dh, dc.double(), df.double() * m2)
    ds, dcp = nan(dev, N, W), nan(dev, N, R)
    L().check(lib.capmi_adaatt_cell_bwd(kp(a), ptr(t['mask']), kp(df), ptr(t['mask2']), ptr(b), nb or 1, stride,
                                        kp(dc), kp(s_ref.float()), ptr(t['c_prev']), kp(c_ref.float()),
                                        ptr(ds), ptr(dcp), N, R, mo, L().stream_ptr()), 'adaatt_cell_bwd')
    check('d_sums', ds, ref_ds, CELL_BWD, p, tie_skip(d['pre'], R, 6) if mo else None)
    check('dc_prev', dcp, ref_dcp, CELL_BWD, p)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize('i', range(len(S.ATT_FWD)))
def test_attention_fwd(dev, i):
    B, n, K, A, R, hs, flags, _ = S.ATT_FWD[i]
    fl = set(flags.split())
    d = S.attention_case(B, n, K, A, R, hs, flags, seed=i)
    N = d['N']
    t = {k: put(dev, d[k], 'off:' + k in fl) for k in ('h_slabs', 'h_bias', 'p_att', 'att', 'w', 'b', 'mask')}
    row_img = put(dev, d['img'].int()) if 'rowimg' in fl else None
    ctx, alpha, aho = nan(dev, N, R), nan(dev, N, K), nan(dev, N, A)
    lib = L().lib
    tail = (ptr(t['p_att']), ptr(t['att']), ptr(t['mask']), ptr(t['w']), ptr(t['b']), ptr(ctx), ptr(alpha), B, n, K, A, R, ptr(row_img), N,
            L().stream_ptr())
    if hs == 0:
        L().check(lib.capmi_attention_fwd(ptr(t['h_slabs']), *tail), 'attention_fwd')
    else:
        L().check(lib.capmi_attention_fwd_partial(ptr(t['h_slabs']), hs, N * A + d['h_pad'], ptr(t['h_bias']), ptr(aho), *tail),
                  'attention_fwd_partial')
        check('att_h_out', aho, d['att_h'], ATT_FWD)
    check('alpha', alpha, d['alpha'], ATT_FWD)
    check('ctx', ctx, d['ctx'], ATT_FWD)
    if d['mask'] is not None:      # masked regions get exactly nothing; the single-region image puts all its weight there
        torch.cuda.synchronize()
        dead = d['mask'][d['img']] == 0
        assert float(alpha.cpu()[dead].abs().max()) == 0.0
        assert float((alpha.cpu()[d['img'] == 0, 0] - 1).abs().max()) < 1e-6


@pytest.mark.parametrize('i', range(len(S.ATT_BWD)))
def test_attention_bwd(dev, i):
    B, n, K, A, R, xs, extra, flags, _ = S.ATT_BWD[i]
    fl = set(flags.split())
    g = S.gen(800 + i)
    N, cols = B * n, R + extra
    if xs:
        stride = N * cols + (8 if cols % 4 == 0 else 0)      # the reduce-then-run fallback takes dense slabs only
        raw = (torch.randn(xs, stride, generator=g) / xs ** 0.5).float()
        x_ref = raw[:, :N * cols].double().sum(0).view(N, cols)
    else:
        raw = torch.randn(1, N * cols, generator=g).float()
        x_ref = raw.double().view(N, cols)
    d = S.attention_case(B, n, K, A, R, 0, flags, seed=40 + i, d_ctx=x_ref[:, :R].contiguous())
    t = {k: put(dev, d[k]) for k in ('p_att', 'att', 'w', 'mask')}
    att_h = put(dev, d['h_slabs'][0, :N * A].view(N, A))
    alpha = put(dev, d['alpha'].float())
    row_img = put(dev, d['img'].int()) if 'rowimg' in fl else None
    dah, de = nan(dev, N, A), nan(dev, N, K)
    tail = (ptr(dah), ptr(de), B, n, K, A, R, ptr(row_img), N, L().stream_ptr())
    x = put(dev, raw)
    lib = L().lib
    if xs == 0:
        L().check(lib.capmi_attention_bwd(ptr(x), cols, ptr(att_h), ptr(alpha), ptr(t['p_att']), ptr(t['att']), ptr(t['mask']), ptr(t['w']),
                                          *tail), 'attention_bwd')
    else:
        x_out = nan(dev, N, cols)
        L().check(lib.capmi_attention_bwd_partial(ptr(x), xs, stride, cols, ptr(x_out), ptr(att_h), ptr(alpha), ptr(t['p_att']),
                                                  ptr(t['att']), ptr(t['w']), *tail), 'attention_bwd_partial')
        check('x_out', x_out, x_ref, CELL_FWD)
    check('d_e', de, d['d_e'], ATT_BWD)
    check('d_att_h', dah, d['d_att_h'], ATT_BWD)


@pytest.mark.parametrize('i', range(len(S.ATT_BATCHED)))
def test_attention_bwd_batched(dev, i):
    T, B, n, K, A, R, pad, _ = S.ATT_BATCHED[i]
    g = S.gen(900 + i)
    Ns, ld = B * n + pad, R + 3
    # every row of the buffers is drawn, the rows past B * n of a slab too: they belong to another rollout and no output, d_b
    # included, may depend on them
    d_ctx = torch.randn(T, Ns, ld, generator=g).float()
    att_h = torch.randn(T, Ns, A, generator=g).float()
    alpha = torch.softmax(torch.randn(T, Ns, K, generator=g), 2).float()
    d_e = (torch.randn(T, Ns, K, generator=g) * 0.1).float()
    p_att, w = torch.randn(B, K, A, generator=g).float(), torch.randn(A, generator=g).float()
    r_att, r_patt, r_w, r_b, r_rows = S.attention_batched(d_ctx[:, :, :R], att_h, alpha, d_e, p_att, w, B, n)
    t = [put(dev, x) for x in (d_ctx, att_h, alpha, d_e, p_att, w)]
    lib = L().lib
    for partial in (False, True):
        o_att, o_patt, o_w, o_b, o_rows = nan(dev, B, K, R), nan(dev, B, K, A), nan(dev, A), nan(dev, 1), nan(dev, B * K, A)
        L().check(lib.capmi_attention_bwd_batched_ws(ptr(t[0]), ld, ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]), ptr(t[5]), ptr(o_att),
                                                     ptr(o_patt), None if partial else ptr(o_w), ptr(o_b), T, B, n, Ns, K, A, R,
                                                     ptr(o_rows) if partial else None, L().stream_ptr()), 'attention_bwd_batched_ws')
        check('d_att', o_att, r_att, ATT_BWD)
        check('d_p_att', o_patt, r_patt, ATT_BWD)
        if partial:     # one row per (image, region), [B * K, A]; d_w is their column sum, taken here in float64
            check('dw_partial', o_rows.view(B, K, A), r_rows, ATT_BWD)
            assert rel_err(o_rows.double().cpu().sum(0), r_w) < ATT_BWD
        else:
            check('d_w', o_w, r_w, ATT_BWD)
        # d_b is a sum of T * B * n * K terms of either sign and may cancel to next to nothing, so max|ref| is no scale for it: the
        # rounding of a float32 sum grows with sum|d_e| over the rows that count, and the bound is taken against that
        torch.cuda.synchronize()
        scale = float(d_e[:, :B * n].double().abs().sum())
        print('d_b err %.2e of sum|d_e| (bound %.0e)' % (abs(float(o_b.cpu()) - float(r_b)) / scale, ATT_BWD))
        assert abs(float(o_b.cpu()) - float(r_b)) < ATT_BWD * scale


# ------------------------------------------------------------------------------------------------ small ones
@pytest.mark.parametrize('N,V1,T', [(1, 7, 3), (6, 7, 2), (1, 9488, 2), (6, 9488, 3)])
def test_logsoftmax_bwd_dense(dev, N, V1, T):
    kp = Keep(dev)
    g = S.gen(N + V1)
    Lc = 3
    gr = torch.randn(N, Lc, V1, generator=g).float()
    lp = torch.log_softmax(torch.randn(N, Lc, V1, generator=g) * 3, 2).float()
    live = torch.ones(N, Lc, dtype=torch.uint8)
    live[N - 1, 1] = 0                                   # one dead row
    out = nan(dev, T, N, V1)
    L().check(L().lib.capmi_logsoftmax_bwd(kp(gr), kp(lp), kp(live), ptr(out), N, Lc, T, V1,
                                           L().stream_ptr()), 'logsoftmax_bwd')
    ref = (gr.double() - lp.double().exp() * gr.double().sum(2, keepdim=True)) * live.double().unsqueeze(2)
    check('dlogits', out, ref.transpose(0, 1)[:T].contiguous(), CELL_BWD)      # time-major, the first T steps
    assert float(out[1, N - 1].abs().max()) == 0.0


@pytest.mark.parametrize('B,n', [(7, 1), (6, 5)])
def test_scst_advantage(dev, B, n):
    N = B * n
    scores = torch.rand(N + B, generator=S.gen(B), dtype=torch.float64)
    ref = scores[:N] - scores[N:].repeat_interleave(n)
    sc = put(dev, scores)
    r1, r2, mean = nan(dev, N), nan(dev, N), nan(dev, 1)
    L().check(L().lib.capmi_scst_advantage(ptr(sc), N, n, ptr(r1), L().stream_ptr()), 'scst_advantage')
    L().check(L().lib.capmi_scst_advantage_mean(ptr(sc), N, n, ptr(r2), ptr(mean), L().stream_ptr()), 'scst_advantage_mean')
    torch.cuda.synchronize()
    assert torch.equal(r1.cpu(), ref.float()) and torch.equal(r2.cpu(), ref.float())      # one float64 subtraction, rounded once
    assert abs(float(mean.cpu()) - float(ref.float().double().mean())) < 1e-6


def test_rollout_init(dev):
    lib = L().lib
    for N, count, four in ((6, 20, True), (6, 20, False), (6, 6, True)):
        bufs = [torch.full((count + 3,), 7.0, device=dev) for _ in range(4)]
        it = torch.full((N + 2,), 9, dtype=torch.long, device=dev)
        unf = torch.full((N + 2,), 5, dtype=torch.uint8, device=dev)
        L().check(lib.capmi_rollout_init(ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]) if four else None, ptr(bufs[3]) if four else None, count,
                                         ptr(it), ptr(unf), N, L().stream_ptr()), 'rollout_init')
        torch.cuda.synchronize()
        for k, b in enumerate(bufs):
            want = 0.0 if (k < 2 or four) else 7.0
            assert float(b[:count].abs().max()) == want and float(b[count:].min()) == 7.0      # nothing past `count`
        assert it.cpu().tolist() == [0] * N + [9, 9] and unf.cpu().tolist() == [1] * N + [5, 5]
    b = torch.zeros(8, device=dev)
    assert lib.capmi_rollout_init(ptr(b), ptr(b), None, None, 4, ptr(it), ptr(unf), 6, L().stream_ptr()) == L().EINVAL      # count < N


# fp32 pointwise maths and sums of <= 260 terms: a few roundings of 6e-8 each, the bounds of the cell kernels
@pytest.mark.parametrize('B,K,D', [(4, 8, 64), (3, 7, 33)])
def test_meanpool_fwd_bwd(dev, B, K, D):
    kp = Keep(dev)
    g = S.gen(B + D)
    x, dm = torch.randn(B, K, D, generator=g).float(), torch.randn(B, D, generator=g).float()
    mask = (torch.arange(K).unsqueeze(0) < torch.tensor([K, 1, 3, K][:B]).unsqueeze(1)).float()
    lib = L().lib
    for m in (mask, None):
        md = torch.ones(B, K, dtype=torch.float64) if m is None else m.double()
        cnt = md.sum(1, keepdim=True)
        mean = nan(dev, B, D)
        L().check(lib.capmi_meanpool_fwd(kp(x), kp(m), ptr(mean), B, K, D, L().stream_ptr()), 'meanpool_fwd')
        check('mean', mean, (x.double() * md.unsqueeze(2)).sum(1) / cnt, CELL_FWD)
        ref_dx = (md / cnt).unsqueeze(2) * dm.double().unsqueeze(1)
        for acc in (0, 1):
            dx = put(dev, x) if acc else nan(dev, B, K, D)
            L().check(lib.capmi_meanpool_bwd(kp(dm), kp(m), ptr(dx), acc, B, K, D, L().stream_ptr()), 'meanpool_bwd')
            check('dx', dx, ref_dx + (x.double() if acc else 0.0), CELL_FWD)


@pytest.mark.parametrize('M,R', [(8, 64), (7, 33)])
def test_glu_fwd(dev, M, R):
    kp = Keep(dev)
    g = S.gen(M + R)
    pre = (torch.randn(M, 2 * R, generator=g) * 3).float()
    mask, res = ((torch.rand(M, R, generator=g) < 0.5).float() * 2), torch.randn(M, R, generator=g).float()
    for m, r in ((mask, res), (None, None)):
        out = nan(dev, M, R)
        L().check(L().lib.capmi_glu_fwd(kp(pre), kp(m), kp(r), ptr(out), M, R, L().stream_ptr()), 'glu_fwd')
        ref = pre[:, :R].double() * torch.sigmoid(pre[:, R:].double())
        check('glu', out, ref if m is None else res.double() + mask.double() * ref, CELL_FWD)


@pytest.mark.parametrize('M,D', [(8, 256), (7, 261)])
def test_layernorm_fwd(dev, M, D):
    kp = Keep(dev)
    g = S.gen(M + D)
    x = (torch.randn(M, D, generator=g) * 2 + 0.5).float()
    a, b = torch.randn(D, generator=g).float(), torch.randn(D, generator=g).float()
    y, mean, inv = nan(dev, M, D), nan(dev, M), nan(dev, M)
    eps = 1e-6
    L().check(L().lib.capmi_layernorm_fwd(kp(x), kp(a), kp(b), ptr(y), ptr(mean), ptr(inv), M, D, eps,
                                          L().stream_ptr()), 'layernorm_fwd')
    xd = x.double()
    mu, sd = xd.mean(1, keepdim=True), xd.std(1, keepdim=True)         # unbiased, TransformerModel.py:76-87
    check('mean', mean.view(M, 1), mu, CELL_FWD)
    check('inv', inv.view(M, 1), 1.0 / (sd + eps), CELL_FWD)
    check('y', y, a.double() * (xd - mu) / (sd + eps) + b.double(), CELL_BWD)


# ------------------------------------------------------------------------------------------------ sentinel attention (AdaAtt)
# Each of the three entry points alone against S.sentinel_case: the backward is fed the float32 rounding of the float64 pi, the
# time-batched pass those of pi and d_e, so no kernel's error is absorbed by the next.  Bounds: ATT_FWD for pi, ctx, fre_out, hoe_out,
# ATT_BWD for every gradient -- those of the plain attention, the same operation over K instead of K + 1 rows.
GUARD = 777.0


class Out:
    """an output: NaN where the kernel must write, a guard value in the 8 floats behind it (and in the float before it with off,
    where the output starts one float past a 16-byte boundary)"""
    def __init__(self, dev, *shape, off=False):
        cnt = int(np.prod(shape))
        self.buf = torch.full((cnt + 9,), GUARD, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = (1 if off else 0), (1 if off else 0) + cnt
        self.buf[self.lo:self.hi] = float('nan')
        self.t = self.buf[self.lo:self.hi].view(shape)

    @property
    def p(self):
        return self.t.data_ptr()

    def guarded(self):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        return bool((b[:self.lo] == GUARD).all()) and bool((b[self.hi:] == GUARD).all()) and b[self.hi:].numel() >= 8

    def untouched(self):
        return self.guarded() and bool(torch.isnan(self.t).all())


def check_out(name, out, ref, tol):
    check(name, out.t, ref, tol)
    assert out.guarded(), name + ': wrote outside its buffer'


def tile_drop(mask=None, p=0.0, seed=0, row0=0):
    import ctypes
    td = L().TileDrop()
    td.mask, td.p, td.seed, td.row0 = ptr(mask), float(p), int(seed), int(row0)
    return ctypes.byref(td)


def sent_fwd(dev, t, drop, pi, ctx, fo, ho_, fs, hs, strides, B, n, K, A, R):
    return L().lib.capmi_sentinel_attention_fwd(ptr(t['fre_slabs']), fs, strides[0], ptr(t.get('fre_bias')), ptr(t['hoe_slabs']), hs, strides[1],
                                                ptr(t.get('hoe_bias')), fo and fo.p, ho_ and ho_.p, ptr(t['fr']), ptr(t['ho']), ptr(t['p_att']),
                                                ptr(t['att']), ptr(t.get('mask')), ptr(t['w']), ptr(t['b']), drop, pi.p, ctx.p, B, n, K, A, R,
                                                L().stream_ptr())


@pytest.mark.parametrize('i', range(len(S.SENT_FWD)))
def test_sentinel_fwd(dev, i):
    B, n, K, A, R, fs, hs, flags, _ = S.SENT_FWD[i]
    fl = set(flags.split())
    d = S.sentinel_case(1, B, n, K, A, R, fs, hs, flags, seed=1000 + i)
    N = d['N']
    t = {k: put(dev, d[k], 'off:' + k in fl) for k in ('fre_slabs', 'hoe_slabs', 'fre_bias', 'hoe_bias', 'fr', 'ho', 'p_att', 'att', 'w', 'b',
                                                         'mask', 'tile')}
    pi, ctx = Out(dev, N, K + 1), Out(dev, N, R, off='off:ctx' in fl)
    fo, ho_ = (None, None) if 'noout' in fl else (Out(dev, N, A), Out(dev, N, A))
    L().check(sent_fwd(dev, t, tile_drop(t['tile']), pi, ctx, fo, ho_, fs, hs, (d['fre_stride'], d['hoe_stride']), B, n, K, A, R), 'sentinel_fwd')
    if fo is not None:
        check_out('fre_out', fo, d['fre'][0], ATT_FWD)
        check_out('hoe_out', ho_, d['hoe'][0], ATT_FWD)
    check_out('pi', pi, d['pi'][0], ATT_FWD)
    check_out('ctx', ctx, d['ctx'][0], ATT_FWD)
    if d['mask'] is not None:      # dead regions get exactly nothing; the single-region image splits its weight between sentinel and region 0
        got = pi.t.cpu()
        m = d['mask'][d['img']]
        assert float(got[torch.cat([m[:, :1], m], 1) == 0].abs().max()) == 0.0
        assert float((got[d['img'] == 0, :2].sum(1) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize('i', range(len(S.SENT_BWD)))
def test_sentinel_bwd(dev, i):
    T, B, n, K, A, R, flags, _ = S.SENT_BWD[i]
    fl = set(flags.split())
    d = S.sentinel_case(T, B, n, K, A, R, 0, 0, flags, seed=1100 + i)
    N = d['N']
    src = dict(d, fre=d['fre'].float(), hoe=d['hoe'].float(), pi=d['pi'].float())        # fre / hoe were float32 to begin with: exact
    t = {k: put(dev, src[k], 'off:' + k in fl) for k in ('d_ctx', 'fr', 'fre', 'hoe', 'pi', 'p_att', 'att', 'w', 'tile')}
    de, dh, df, dfr = Out(dev, T, N, K + 1), Out(dev, T, N, A), Out(dev, T, N, A), Out(dev, T, N, R)
    L().check(L().lib.capmi_sentinel_attention_bwd(ptr(t['d_ctx']), ptr(t['fr']), ptr(t['fre']), ptr(t['hoe']), ptr(t['pi']), ptr(t['p_att']),
                                                   ptr(t['att']), ptr(t['w']), tile_drop(t['tile']), de.p, dh.p, df.p, dfr.p, T, B, n, K, A, R,
                                                   L().stream_ptr()), 'sentinel_bwd')
    for name, out in (('d_e', de), ('d_hoe', dh), ('d_fre', df), ('d_fr', dfr)):
        check_out(name, out, d[name], ATT_BWD)


def d_b_bound(count, d_e):
    """d_b = sum(d_e) is zero in exact arithmetic; sum_all_kernel adds ceil(count / 1024) values per thread, then a ten-level tree:
    (that run length + 16) roundings of 2^-24 each, relative to sum|d_e|"""
    return (-(-count // 1024) + 16) * 2.0 ** -24 * float(d_e.double().abs().sum())


@pytest.mark.parametrize('i', range(len(S.SENT_BATCHED)))
def test_sentinel_bwd_batched(dev, i):
    T, B, n, K, A, R, flags, _ = S.SENT_BATCHED[i]
    d = S.sentinel_case(T, B, n, K, A, R, 0, 0, flags, seed=1200 + i)
    src = dict(d, fre=d['fre'].float(), hoe=d['hoe'].float(), pi=d['pi'].float(), d_e=d['d_e'].float())
    t = {k: put(dev, src[k]) for k in ('d_ctx', 'fre', 'hoe', 'pi', 'd_e', 'p_att', 'w', 'tile')}
    assert float(d['d_b'].abs()) < 1e-12
    for partial in (True, False):      # dw_partial rows, then d_w by atomicAdd (any order: compared by bound only)
        o_att, o_patt, o_w, o_b, o_rows = Out(dev, B, K, R), Out(dev, B, K, A), Out(dev, A), Out(dev, 1), Out(dev, B, K + 1, A)
        L().check(L().lib.capmi_sentinel_attention_bwd_batched(ptr(t['d_ctx']), ptr(t['fre']), ptr(t['hoe']), ptr(t['pi']), ptr(t['d_e']),
                                                               ptr(t['p_att']), ptr(t['w']), tile_drop(t['tile']), o_att.p, o_patt.p,
                                                               None if partial else o_w.p, o_b.p, T, B, n, K, A, R,
                                                               o_rows.p if partial else None, L().stream_ptr()), 'sentinel_bwd_batched')
        check_out('d_att', o_att, d['d_att'], ATT_BWD)
        check_out('d_p_att', o_patt, d['d_p_att'], ATT_BWD)
        if partial:
            check_out('dw_partial', o_rows, d['dw_rows'], ATT_BWD)
            e = rel_err(o_rows.t.double().cpu().sum((0, 1)), d['d_w'])
            print('column sum of dw_partial rel_err %.2e (bound %.0e)' % (e, ATT_BWD))
            assert e < ATT_BWD and o_w.untouched()
        else:
            check_out('d_w (atomic)', o_w, d['d_w'], ATT_BWD)
            assert o_rows.untouched()
        bound = d_b_bound(T * B * n * (K + 1), src['d_e'])
        got = abs(float(o_b.t.cpu()))
        print('|d_b| %.2e (bound %.2e)' % (got, bound))
        assert got <= bound and o_b.guarded()


def sent_chain(dev, t, T, B, n, K, A, R, tile=None, p=0.0, seed=0):
    """forward of every step (row0 = step * N), backward and time-batched pass of all steps, each fed by the one before"""
    N = B * n
    o = {k: Out(dev, *s) for k, s in (('pi', (T, N, K + 1)), ('ctx', (T, N, R)), ('d_e', (T, N, K + 1)), ('d_hoe', (T, N, A)), ('d_fre', (T, N, A)),
                                      ('d_fr', (T, N, R)), ('d_att', (B, K, R)), ('d_p_att', (B, K, A)), ('dw_rows', (B, K + 1, A)), ('d_b', (1,)))}
    lib = L().lib
    for s in range(T):
        drop = tile_drop(None if tile is None else tile[s], p, seed, s * N)
        L().check(lib.capmi_sentinel_attention_fwd(ptr(t['fre'][s]), 0, 0, None, ptr(t['hoe'][s]), 0, 0, None, None, None, ptr(t['fr'][s]),
                                                   ptr(t['ho'][s]), ptr(t['p_att']), ptr(t['att']), None, ptr(t['w']), ptr(t['b']), drop,
                                                   o['pi'].t[s].data_ptr(), o['ctx'].t[s].data_ptr(), B, n, K, A, R, L().stream_ptr()), 'fwd')
    drop = tile_drop(tile, p, seed, 0)
    L().check(lib.capmi_sentinel_attention_bwd(ptr(t['d_ctx']), ptr(t['fr']), ptr(t['fre']), ptr(t['hoe']), o['pi'].p, ptr(t['p_att']),
                                               ptr(t['att']), ptr(t['w']), drop, o['d_e'].p, o['d_hoe'].p, o['d_fre'].p, o['d_fr'].p, T, B, n, K,
                                               A, R, L().stream_ptr()), 'bwd')
    L().check(lib.capmi_sentinel_attention_bwd_batched(ptr(t['d_ctx']), ptr(t['fre']), ptr(t['hoe']), o['pi'].p, o['d_e'].p, ptr(t['p_att']),
                                                       ptr(t['w']), drop, o['d_att'].p, o['d_p_att'].p, None, o['d_b'].p, T, B, n, K, A, R,
                                                       o['dw_rows'].p, L().stream_ptr()), 'batched')
    assert all(v.guarded() for v in o.values())
    return {k: v.t for k, v in o.items()}


# (B, K, A, R): vec draw forward and scalar draw backward; scalar draw of words 1..3 of the 4-tuple; forward rpb = 2 (258 rows)
@pytest.mark.parametrize('B,K,A,R', [(4, 5, 64, 16), (4, 5, 10, 16), (86, 3, 12, 8)])
def test_sentinel_philox_row_numbering(dev, B, K, A, R):
    """p > 0 without a mask at n = 3 rows per image and T = 2 steps.  The draw index is (row, score row, column), so a launch of B * n
    single-row images with p_att / att repeated per row draws the same bits; there, step by step, the backward kernels expose every
    bit (d_fre != 0: the sentinel's row, d_p_att != 0: a region's row).  Those bits, injected as a mask, must reproduce the Philox run of
    all three kernels at (B, n): a wrong row number in any of them, or in the chunks of rpb > 1, draws other bits."""
    T, n, p, seed = 2, 3, 0.5, 4321
    N, K1 = B * n, K + 1
    d = S.sentinel_case(T, B, n, K, A, R, 0, 0, '', seed=1300 + A + B)
    src = dict(d, fre=d['fre'].float(), hoe=d['hoe'].float())
    t = {k: put(dev, src[k]) for k in ('fre', 'hoe', 'fr', 'ho', 'p_att', 'att', 'w', 'b', 'd_ctx')}
    tile = torch.zeros(T, N, K1, A, device=dev)
    rep = dict(t, p_att=t['p_att'].repeat_interleave(n, 0).contiguous(), att=t['att'].repeat_interleave(n, 0).contiguous())
    for s in range(T):
        one = {k: (v if k in ('p_att', 'att', 'w', 'b') else v[s:s + 1].contiguous()) for k, v in rep.items()}
        N1 = N
        o = {k: Out(dev, *sh) for k, sh in (('pi', (N1, K1)), ('ctx', (N1, R)), ('d_e', (N1, K1)), ('d_hoe', (N1, A)), ('d_fre', (N1, A)),
                                            ('d_fr', (N1, R)), ('d_att', (N1, K, R)), ('d_p_att', (N1, K, A)), ('dw', (N1, K1, A)), ('d_b', (1,)))}
        drop = tile_drop(None, p, seed, s * N)
        lib = L().lib
        L().check(lib.capmi_sentinel_attention_fwd(ptr(one['fre']), 0, 0, None, ptr(one['hoe']), 0, 0, None, None, None, ptr(one['fr']),
                                                   ptr(one['ho']), ptr(one['p_att']), ptr(one['att']), None, ptr(one['w']), ptr(one['b']), drop,
                                                   o['pi'].p, o['ctx'].p, N1, 1, K, A, R, L().stream_ptr()), 'fwd')
        L().check(lib.capmi_sentinel_attention_bwd(ptr(one['d_ctx']), ptr(one['fr']), ptr(one['fre']), ptr(one['hoe']), o['pi'].p,
                                                   ptr(one['p_att']), ptr(one['att']), ptr(one['w']), drop, o['d_e'].p, o['d_hoe'].p, o['d_fre'].p,
                                                   o['d_fr'].p, 1, N1, 1, K, A, R, L().stream_ptr()), 'bwd')
        L().check(lib.capmi_sentinel_attention_bwd_batched(ptr(one['d_ctx']), ptr(one['fre']), ptr(one['hoe']), o['pi'].p, o['d_e'].p,
                                                           ptr(one['p_att']), ptr(one['w']), drop, o['d_att'].p, o['d_p_att'].p, None, o['d_b'].p,
                                                           1, N1, 1, K, A, R, o['dw'].p, L().stream_ptr()), 'batched')
        assert all(v.guarded() for v in o.values())
        tile[s, :, 0] = (o['d_fre'].t != 0).float() * 2
        tile[s, :, 1:] = (o['d_p_att'].t != 0).float() * 2
    rate = float((tile != 0).float().mean())
    assert abs(rate - (1 - p)) < 5 * (p * (1 - p) / tile.numel()) ** 0.5, rate           # five binomial sigmas
    assert not torch.equal(tile[0], tile[1])
    drawn = sent_chain(dev, t, T, B, n, K, A, R, p=p, seed=seed)
    given = sent_chain(dev, t, T, B, n, K, A, R, tile=tile.contiguous())
    for k in drawn:
        if k == 'd_b':
            continue
        check(k, drawn[k], given[k].double().cpu(), ATT_FWD if k in ('pi', 'ctx') else ATT_BWD)
    # and the injected run is the float64 forward under those bits
    ref = S.sentinel_fwd(*(S.d64(src[k]).flatten(0, 1) for k in ('fre', 'hoe', 'fr', 'ho')), S.d64(d['p_att']), S.d64(d['att']), None,
                         S.d64(d['w']), S.d64(d['b']), tile.double().cpu().flatten(0, 1), d['img'])
    check('pi vs float64', drawn['pi'].flatten(0, 1), ref[0], ATT_FWD)
    check('ctx vs float64', drawn['ctx'].flatten(0, 1), ref[1], ATT_FWD)


def test_sentinel_refusals(dev):
    """each refused before any launch: CAPMI_EINVAL and not one output element written"""
    B, n, K, A, R = 2, 2, 3, 8, 8
    d = S.sentinel_case(1, B, n, K, A, R, 1, 1, '', seed=1400)
    N = B * n
    t = {k: put(dev, d[k]) for k in ('fre_slabs', 'hoe_slabs', 'fre_bias', 'hoe_bias', 'fr', 'ho', 'p_att', 'att', 'w', 'b', 'd_ctx')}
    st = (d['fre_stride'], d['hoe_stride'])
    outs = [Out(dev, N, K + 1), Out(dev, N, R), Out(dev, N, A), Out(dev, N, A)]
    assert sent_fwd(dev, t, tile_drop(None, 1.0, 1, 0), *outs, 1, 1, st, B, n, K, A, R) == L().EINVAL         # p = 1 without a mask
    assert all(o.untouched() for o in outs)
    # forward LDS: 1800 rows go eight to a workgroup, and at A = 1024 those need 8 * (2 * 1024 + K + 1) floats > 64 KB
    Bw, nw, Aw, Rw = 225, 8, 1024, 4
    z = lambda *s: torch.zeros(*s, device=dev)          # noqa: E731
    wide = {'fre_slabs': z(Bw * nw, Aw), 'hoe_slabs': z(Bw * nw, Aw), 'fr': z(Bw * nw, Rw), 'ho': z(Bw * nw, Rw), 'p_att': z(Bw, 1, Aw),
            'att': z(Bw, 1, Rw), 'w': z(Aw), 'b': z(1)}
    outs = [Out(dev, Bw * nw, 2), Out(dev, Bw * nw, Rw), Out(dev, Bw * nw, Aw), Out(dev, Bw * nw, Aw)]
    assert sent_fwd(dev, wide, None, *outs, 0, 0, (0, 0), Bw, nw, 1, Aw, Rw) == L().EINVAL
    assert all(o.untouched() for o in outs)
    lib = L().lib
    x = {k: put(dev, d[k].float()) for k in ('fre', 'hoe', 'pi', 'd_e')}
    bw = [Out(dev, N, K + 1), Out(dev, N, A), Out(dev, N, A), Out(dev, N, R)]
    assert lib.capmi_sentinel_attention_bwd(ptr(t['d_ctx']), ptr(t['fr']), ptr(x['fre']), ptr(x['hoe']), ptr(x['pi']), ptr(t['p_att']),
                                            ptr(t['att']), ptr(t['w']), None, *(o.p for o in bw), 65536, B, n, K, A, R,
                                            L().stream_ptr()) == L().EINVAL                                      # T past the grid's y limit
    assert all(o.untouched() for o in bw)
    bt = [Out(dev, B, K, R), Out(dev, B, K, A), Out(dev, A), Out(dev, 1), Out(dev, B, K + 1, A)]

    def batched(T, n_, d_w, rows):
        return lib.capmi_sentinel_attention_bwd_batched(ptr(t['d_ctx']), ptr(x['fre']), ptr(x['hoe']), ptr(x['pi']), ptr(x['d_e']),
                                                        ptr(t['p_att']), ptr(t['w']), None, bt[0].p, bt[1].p, d_w, bt[3].p, T, B, n_, K, A, R,
                                                        rows, L().stream_ptr())
    assert batched(1366, 1, bt[2].p, bt[4].p) == L().EINVAL              # T * n * 12 floats of pi pass 64 KB of LDS
    assert batched(1, n, None, None) == L().EINVAL                       # nowhere to put d_w
    assert all(o.untouched() for o in bt)


def test_attention_bwd_batched_refuses_more_rows_than_lds_holds(dev):
    """T * n * 12 floats of alpha go through LDS: 1366 rows pass 64 KB.  CAPMI_EINVAL before any launch, as the sentinel twin"""
    T, A, R = 1366, 4, 4
    z = torch.zeros(T, 4, device=dev)
    al = torch.ones(T, 1, device=dev)
    o = [Out(dev, 1, 1, R), Out(dev, 1, 1, A), Out(dev, A), Out(dev, 1), Out(dev, 1, A)]
    lib = L().lib
    for d_w, rows in ((o[2].p, None), (None, o[4].p), (o[2].p, o[4].p)):
        assert lib.capmi_attention_bwd_batched_ws(ptr(z), R, ptr(z), ptr(al), ptr(al), ptr(z), ptr(z), o[0].p, o[1].p, d_w, o[3].p, T, 1, 1, 0, 1,
                                                  A, R, rows, L().stream_ptr()) == L().EINVAL
    assert lib.capmi_attention_bwd_batched(ptr(z), R, ptr(z), ptr(al), ptr(al), ptr(z), ptr(z), o[0].p, o[1].p, o[2].p, o[3].p, T, 1, 1, 0, 1, A, R,
                                           L().stream_ptr()) == L().EINVAL
    assert all(v.untouched() for v in o)
