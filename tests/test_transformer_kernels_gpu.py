"""The Transformer / AoA kernels (csrc/transformer.hip, csrc/aoa_ctx.hip) through the C ABI against the float64 references of
transformer_ref64.py, one case per launch arm: the tables there say which arm a row is meant to reach, and capmi_mha_plan says
which one it did reach.  Metric rel_err = max|got - ref| / max|ref| with the bounds listed in transformer_ref64.py.  Every output
lives in a buffer filled with a guard value, NaN where the kernel must write: what the launch leaves of the NaN, or takes of the
guard (the tail behind the buffer, the gaps of a pitched output), fails the case.  Each kernel is fed float64-derived inputs
(saved mean / inv, probabilities), so that no kernel absorbs another's error."""
import ctypes

import numpy as np
import pytest
import torch

import transformer_ref64 as T
from oracle import planes as PL

pytestmark = pytest.mark.gpu

LN_STAT, LN_Y, MHA_FWD, MHA_BWD, POINT = 2e-6, 5e-6, 2e-6, 5e-6, 2e-6
GUARD = -777.25


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def L():
    from imagecaptioning.pytorch_amd import _lib
    return _lib


class Keep:
    """device copies handed to a call as bare pointers stay alive here until the test ends"""
    def __init__(self, dev):
        self.dev, self.held = dev, []

    def __call__(self, t):
        if t is None:
            return None
        self.held.append(t.to(self.dev).contiguous())
        assert self.held[-1].data_ptr() % 16 == 0
        return self.held[-1].data_ptr()


class Buf:
    """`n` floats of guard value and 8 more behind them; view() marks the part a launch must write (NaN) or add to (fill)"""
    def __init__(self, dev, n):
        self.buf = torch.full((n + 8,), GUARD, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.views = []

    def view(self, shape, strides=None, offset=0, fill=None):
        shape = tuple(shape)
        if strides is None:
            strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        assert offset + sum((n - 1) * s for n, s in zip(shape, strides)) < self.buf.numel() - 8
        v = torch.as_strided(self.buf, shape, strides, offset)
        v.copy_(fill.to(self.buf.device)) if fill is not None else v.fill_(float('nan'))
        self.views.append((shape, strides, offset))
        return v

    def ptr(self, offset=0):
        return self.buf.data_ptr() + 4 * offset

    def guarded(self):
        """nothing outside the views was written"""
        torch.cuda.synchronize()
        b = self.buf.clone()
        for shape, strides, offset in self.views:
            torch.as_strided(b, shape, strides, offset).fill_(GUARD)
        return bool((b == GUARD).all())

    def untouched(self):
        """the views are still NaN and nothing outside them was written"""
        return self.guarded() and all(bool(torch.isnan(torch.as_strided(self.buf, *v)).all()) for v in self.views)


def out(dev, *shape):
    b = Buf(dev, int(np.prod(shape)))
    b.t = b.view(shape)
    return b


def check(name, got, ref, tol, plant=None, plant_scale=0.0):
    """rel_err over the rows other than `plant` below tol; the planted row elementwise, |got - ref| <= tol (1 + |ref| + plant_scale).
    plant_scale is 0 for every output that is pointwise in its row.  The planted dx is inv (g - mean g) with inv = 1e6: float32
    carries g - mean g to tol max|g| at best, whatever the element's own size, so that row takes plant_scale = inv max|g|
    (plant_dx_scale) -- still element by element, still outside the case's maximum.  Under the plain form the kernels measure
    up to 8.6e-5 on that row (absolute 0.5 on elements of a row whose maximum is 3e6), a float32 limit and not a defect."""
    torch.cuda.synchronize()
    got = got.double().cpu()
    assert got.shape == ref.shape, name
    if plant is not None:
        assert bool(torch.isfinite(got[plant]).all()), (name, 'planted row is not finite')
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    rows = [r for r in range(ref.shape[0]) if r != plant] if (plant is not None and ref.shape[0] > 1) else list(range(ref.shape[0]))
    e = float(err[rows].max() / (ref[rows].abs().max() + 1e-30))
    if plant is None:
        print('%s rel_err %.2e (bound %.0e)' % (name, e, tol))
    else:
        print('%s rel_err %.2e (bound %.0e), planted row max err / (1 + |ref|) %.2e' %
              (name, e, tol, float((err[plant] / (1.0 + ref[plant].abs())).max())))
    assert e < tol, (name, e)
    if plant is not None:
        over = err[plant] - tol * (1.0 + ref[plant].abs() + plant_scale)
        assert float(over.max()) <= 0.0, (name, 'planted row', int(over.argmax()), float(err[plant].max()))


def planes_buf(dev, k):
    return torch.zeros(int(L().lib.capmi_planes_bytes(k)), dtype=torch.uint8, device=dev)


def same_planes(pl, x):
    torch.cuda.synchronize()
    assert np.array_equal(pl.cpu().numpy(), PL.planes_from_f32(x.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize('M,D', T.LN_FWD)
def test_layernorm_fwd(dev, M, D):
    kp = Keep(dev)
    d = T.ln_inputs(M, D, seed=1000 + 3 * D + M)
    y, mean, inv = out(dev, M, D), out(dev, M), out(dev, M)
    L().check(L().lib.capmi_layernorm_fwd(kp(d['x']), kp(d['a']), kp(d['b']), y.ptr(), mean.ptr(), inv.ptr(), M, D, T.EPS,
                                          L().stream_ptr()), 'layernorm_fwd')
    y_ref, m_ref, i_ref = T.ln_fwd_ref(d['x'], d['a'], d['b'])
    p = d['plant']
    check('y', y.t, y_ref, LN_Y, p)
    check('mean', mean.t, m_ref, LN_STAT, p)
    check('inv', inv.t, i_ref, LN_STAT, p)
    assert y.guarded() and mean.guarded() and inv.guarded()


def plant_dx_scale(dy, a, plant):
    return float((T.d64(dy[plant]) * T.d64(a)).abs().max()) / T.EPS


def ln_case(M, D, seed):
    d = T.ln_inputs(M, D, seed)
    _, mean, inv = T.ln_fwd_ref(d['x'], d['a'], d['b'])
    d['mean'], d['inv'] = mean.float(), inv.float()
    d['ref'] = T.ln_bwd_ref(d['dy'], d['x'], d['a'])
    d['dx_scale'] = plant_dx_scale(d['dy'], d['a'], d['plant'])
    return d


@pytest.mark.parametrize('M,D', T.LN_BWD)
def test_layernorm_bwd(dev, M, D):
    kp = Keep(dev)
    d = ln_case(M, D, seed=2000 + 3 * D + M)
    dx_ref, gs_ref, da_ref, db_ref = d['ref']
    p = d['plant']
    ins = [kp(d[k]) for k in ('dy', 'x', 'a', 'mean', 'inv')]
    for acc in (0, 1):
        for want_gs in (False, True):
            b = Buf(dev, M * D)
            dx = b.view((M, D), fill=d['dx0'] if acc else None)
            gs = out(dev, M, D) if want_gs else None
            L().check(L().lib.capmi_layernorm_bwd(*ins, b.ptr(), acc, gs.ptr() if gs else None, M, D, T.EPS, L().stream_ptr()),
                      'layernorm_bwd')
            check('dx acc=%d' % acc, dx, dx_ref + T.d64(d['dx0']) if acc else dx_ref, T.LN_BWD_TOL, p, d['dx_scale'])
            assert b.guarded()
            if gs:
                check('g_scaled', gs.t, gs_ref, T.LN_BWD_TOL, p)
                assert gs.guarded()
                # the parameter gradients are the column sums of g_scaled and dy (capmi.h)
                check('d_a', gs.t.double().sum(0)[None], da_ref[None], T.LN_BWD_TOL)


@pytest.mark.parametrize('M,D,acc', T.LN_PARTS)
def test_layernorm_bwd_parts(dev, M, D, acc):
    kp = Keep(dev)
    d = ln_case(M, D, seed=3000 + 3 * D + M)
    dx_ref, _, da_ref, db_ref = d['ref']
    rows = T.ln_parts_rows(M)
    assert rows == L().lib.capmi_layernorm_bwd_parts_rows(M)
    b = Buf(dev, M * D)
    dx = b.view((M, D), fill=d['dx0'] if acc else None)
    pa, pb = out(dev, rows, D), out(dev, rows, D)
    L().check(L().lib.capmi_layernorm_bwd_parts(*[kp(d[k]) for k in ('dy', 'x', 'a', 'mean', 'inv')], b.ptr(), acc, pa.ptr(), pb.ptr(),
                                                M, D, T.EPS, L().stream_ptr()), 'layernorm_bwd_parts')
    check('dx', dx, dx_ref + T.d64(d['dx0']) if acc else dx_ref, T.LN_BWD_TOL, d['plant'], d['dx_scale'])
    check('d_a', pa.t.double().sum(0)[None], da_ref[None], T.LN_BWD_TOL)
    check('d_b', pb.t.double().sum(0)[None], db_ref[None], T.LN_BWD_TOL)
    assert b.guarded() and pa.guarded() and pb.guarded()


@pytest.mark.parametrize('M,D,s_dy,s_acc', T.LN_SLABS)
def test_layernorm_bwd_slabs(dev, M, D, s_dy, s_acc):
    kp = Keep(dev)
    d = T.ln_inputs(M, D, seed=4000 + 3 * D + s_dy)
    g = T.gen(4500 + D + s_acc)
    dy_raw, dy_stride, dy = T.slabs_of(g, s_dy, M, D)
    acc_raw, acc_stride, cat = T.slabs_of(g, s_acc, M, 2 * D)               # [att | query] halves: the query half is the running gradient
    _, mean, inv = T.ln_fwd_ref(d['x'], d['a'], d['b'])
    dx_ref, gs_ref, _, _ = T.ln_bwd_ref(dy, d['x'], d['a'])
    acc_dev = acc_raw.to(dev)
    dy_out = out(dev, M, D) if s_dy != 3 else None
    gs = out(dev, M, D) if s_dy != 5 else None
    dx = out(dev, M, D)
    L().check(L().lib.capmi_layernorm_bwd_slabs(kp(dy_raw), s_dy, dy_stride, dy_out.ptr() if dy_out else None, kp(d['x']), kp(d['a']),
                                                kp(mean.float()), kp(inv.float()), acc_dev.data_ptr() + 4 * D, s_acc, acc_stride, 2 * D,
                                                dx.ptr(), gs.ptr() if gs else None, M, D, T.EPS, L().stream_ptr()), 'layernorm_bwd_slabs')
    p = d['plant']
    check('dx', dx.t, dx_ref + cat[:, D:], T.LN_BWD_TOL, p, plant_dx_scale(dy, d['a'], p))
    if dy_out:
        check('dy_out', dy_out.t, dy, POINT, p)
    if gs:
        check('g_scaled', gs.t, gs_ref, T.LN_BWD_TOL, p)
    assert dx.guarded() and (dy_out is None or dy_out.guarded()) and (gs is None or gs.guarded())
    assert torch.equal(acc_dev.cpu(), acc_raw), 'the pitched input changed'


# ------------------------------------------------------------------------------------------------ multi-head attention
def c_plan(bwd, Nq, qpk, Tq, Tk, h, dk):
    ch, th, mf, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    rc = L().lib.capmi_mha_plan(bwd, Nq, qpk, Tq, Tk, h, dk, ctypes.byref(ch), ctypes.byref(th), ctypes.byref(mf), ctypes.byref(lds))
    return rc, (ch.value, th.value, mf.value, lds.value)


def nan_padded(dev, t, shape, strides, n):
    """the tensor inside a NaN-filled buffer of n floats, behind the given strides: a kernel that reads a gap shows it"""
    buf = torch.full((n,), float('nan'), device=dev)
    torch.as_strided(buf, shape, strides).copy_(t.to(dev))
    return buf


@pytest.mark.parametrize('i', range(len(T.MHA)))
def test_mha(dev, i):
    r = T.MHA[i]
    lib, st = L().lib, L().stream_ptr()
    Nkv, qpk, Tq, Tk, h, dk = (r[k] for k in ('Nkv', 'qpk', 'Tq', 'Tk', 'h', 'dk'))
    D, Nq = h * dk, Nkv * qpk
    for kind in ('fwd', 'bwd') if r['bwd'] else ('fwd',):
        rc, plan = c_plan(int(kind == 'bwd'), Nq, qpk, Tq, Tk, h, dk)
        assert rc == 0 and plan == T.mha_plan(kind, Nq, qpk, Tq, Tk, h, dk), (r['name'], kind, plan)
    d = T.mha_inputs(r, seed=5000 + i)
    o_ref, p_ref, dq_ref, dk_ref, dv_ref = T.mha_ref(r, d)
    kp = Keep(dev)
    lay = r['layout']
    qs = ks = dqs = dkvs = dkvld = 0
    ldkv = Tk * D
    if lay == 'plain':
        qp, kptr, vptr = kp(d['q']), kp(d['k']), kp(d['v'])
    elif lay == 'packed':                       # Nq == Nkv, Tq == Tk
        qkv = torch.cat([d[k].reshape(Nq * Tq, D) for k in ('q', 'k', 'v')], 1)
        qp = kp(qkv)
        kptr, vptr, qs, ks, ldkv = qp + 4 * D, qp + 8 * D, 3 * D, 3 * D, Tk * 3 * D
    elif lay == 'vk':
        vptr = kp(torch.cat([d['v'], d['k']], 2))
        qp, kptr, ks, ldkv = kp(d['q']), vptr + 4 * D, 2 * D, Tk * 2 * D
    else:
        qs, ks, ldkv = D + 4, D + 4, Tk * (D + 4) + 8
        bq = nan_padded(dev, d['q'].view(Nq * Tq, D), (Nq * Tq, D), (qs, 1), Nq * Tq * qs)
        bk = nan_padded(dev, d['k'], (Nkv, Tk, D), (ldkv, ks, 1), Nkv * ldkv)
        bv = nan_padded(dev, d['v'], (Nkv, Tk, D), (ldkv, ks, 1), Nkv * ldkv)
        kp.held += [bq, bk, bv]
        qp, kptr, vptr = bq.data_ptr(), bk.data_ptr(), bv.data_ptr()
    mask = None if d['mask'] is None else kp(d['mask'].to(torch.uint8))
    mtq, mpq = (Tq if r['mask'] == 'qT' else 1), int(r['mask'] in ('q1', 'qT'))
    drop = kp(d['drop'])
    o = out(dev, Nq, Tq, D)
    p = out(dev, Nq, h, Tq, Tk) if r['want_p'] else None
    pp = p.ptr() if p else None
    if lay in ('plain', 'vk'):
        rc = lib.capmi_mha_fwd(qp, kptr, vptr, ldkv, ks, mask, mtq, mpq, r['causal'], r['q_pos0'], drop, o.ptr(), pp, Nq, qpk, Tq, Tk, h, dk, st)
    else:
        rc = lib.capmi_mha_fwd_s(qp, qs, kptr, vptr, ldkv, ks, mask, mtq, mpq, r['causal'], r['q_pos0'], drop, o.ptr(), pp, Nq, qpk, Tq, Tk,
                                 h, dk, st)
    L().check(rc, 'mha_fwd')
    check('o', o.t, o_ref, MHA_FWD)
    assert o.guarded()
    if p:
        check('p', p.t, p_ref, MHA_FWD)
        assert p.guarded()
        assert bool((p.t.cpu()[p_ref == 0] == 0).all()), 'a masked key has probability'
    if not r['bwd']:
        return
    # backward from the float64 probabilities
    do_p, p_in = kp(d['d_o']), kp(p_ref.float())
    acc = r['acc']
    fill_k, fill_v = (d['dk0'], d['dv0']) if acc else (None, None)
    if lay == 'plain':
        bufs = [out(dev, Nq, Tq, D), Buf(dev, Nkv * Tk * D), Buf(dev, Nkv * Tk * D)]
        dq, dk_, dv_ = bufs[0].t, bufs[1].view((Nkv, Tk, D), fill=fill_k), bufs[2].view((Nkv, Tk, D), fill=fill_v)
        ptrs = [b.ptr() for b in bufs]
    elif lay == 'packed':
        b = Buf(dev, Nq * Tq * 3 * D)
        dq, dk_, dv_ = (b.view((Nq, Tq, D), (Tq * 3 * D, 3 * D, 1), c * D, f) for c, f in ((0, None), (1, fill_k), (2, fill_v)))
        bufs, ptrs, dqs, dkvs, dkvld = [b], [b.ptr(0), b.ptr(D), b.ptr(2 * D)], 3 * D, 3 * D, Tk * 3 * D
    elif lay == 'vk':
        b = Buf(dev, Nkv * Tk * 2 * D)
        dv_, dk_ = (b.view((Nkv, Tk, D), (Tk * 2 * D, 2 * D, 1), c * D, f) for c, f in ((0, fill_v), (1, fill_k)))
        bufs = [out(dev, Nq, Tq, D), b]
        dq, ptrs, dkvs, dkvld = bufs[0].t, [bufs[0].ptr(), b.ptr(D), b.ptr(0)], 2 * D, Tk * 2 * D
    else:
        dqs, dkvs, dkvld = D + 8, D + 4, Tk * (D + 4) + 8
        bufs = [Buf(dev, Nq * Tq * dqs), Buf(dev, Nkv * dkvld), Buf(dev, Nkv * dkvld)]
        dq = bufs[0].view((Nq, Tq, D), (Tq * dqs, dqs, 1))
        dk_, dv_ = bufs[1].view((Nkv, Tk, D), (dkvld, dkvs, 1), 0, fill_k), bufs[2].view((Nkv, Tk, D), (dkvld, dkvs, 1), 0, fill_v)
        ptrs = [b.ptr() for b in bufs]
    if lay == 'plain':
        rc = lib.capmi_mha_bwd(do_p, qp, kptr, vptr, ldkv, ks, p_in, drop, *ptrs, dkvld, dkvs, acc, Nq, qpk, Tq, Tk, h, dk, st)
    else:
        rc = lib.capmi_mha_bwd_s(do_p, qp, qs, kptr, vptr, ldkv, ks, p_in, drop, ptrs[0], dqs, ptrs[1], ptrs[2], dkvld, dkvs, acc, Nq, qpk,
                                 Tq, Tk, h, dk, st)
    L().check(rc, 'mha_bwd')
    check('dq', dq, dq_ref, MHA_BWD)
    check('dk', dk_, dk_ref, MHA_BWD)
    check('dv', dv_, dv_ref, MHA_BWD)
    assert all(b.guarded() for b in bufs), 'wrote into a gap or behind a buffer'


# ------------------------------------------------------------------------------------------------ fused GLU / ctx forwards
def fused_outputs(dev, kind, M, R, d, want_a, want_b, want_pre):
    G = T.CTX_G[kind]
    o = dict(pre=out(dev, M, G * R) if want_pre else None, out=out(dev, M, R), c=out(dev, M, R) if kind == T.CTX_LSTM else None,
             out_a=out(dev, M, R) if want_a else None, out_b=out(dev, M, R) if want_b else None)
    o['pl_a'] = planes_buf(dev, R) if want_a else None
    o['pl_b'] = planes_buf(dev, R) if want_b else None
    return o


def optr(b):
    return None if b is None else (b.data_ptr() if torch.is_tensor(b) else b.ptr())


def run_ctx(dev, kp, kind, M, R, splits, d, o):
    s = L().CtxStep()
    for k in ('slabs', 'bias', 'bias2', 'c_prev', 'resid', 'mask_a', 'mask_b'):
        setattr(s, k, kp(d.get(k)))
    s.pre, s.c, s.out, s.out_a, s.planes_a, s.out_b, s.planes_b = (optr(o[k]) for k in ('pre', 'c', 'out', 'out_a', 'pl_a', 'out_b', 'pl_b'))
    s.stride, s.kind, s.splits, s.M, s.R = d['stride'], kind, splits, M, R
    return L().lib.capmi_ctx_fwd_fused(ctypes.byref(s), L().stream_ptr())


def check_fused(kind, d, o, resid):
    saved, c_ref, out_ref, oa_ref, ob_ref = T.fused_ref(kind, dict(d, resid=d['resid'] if resid else None))
    if o['pre'] is not None:
        if saved is None:
            assert o['pre'].untouched(), 'the ReLU kind wrote pre'
        else:
            check('pre', o['pre'].t, saved, POINT)
    check('out', o['out'].t, out_ref, POINT)
    if c_ref is not None:
        check('c', o['c'].t, c_ref, POINT)
    for k, ref, pl in (('out_a', oa_ref, 'pl_a'), ('out_b', ob_ref, 'pl_b')):
        if o[k] is not None:
            check(k, o[k].t, ref, POINT)
            same_planes(o[pl], o[k].t)
    assert all(b.guarded() for b in o.values() if isinstance(b, Buf))


@pytest.mark.parametrize('M,R', T.FUSED_SHAPES)
def test_glu_fwd_fused(dev, M, R):
    for (m, r_, splits, masked) in [c for c in T.GLU_FUSED if c[:2] == (M, R)]:
        kp = Keep(dev)
        d = T.fused_inputs(T.CTX_GLU, M, R, splits, masked, seed=6000 + 10 * M + splits + masked)
        d['bias2'] = None
        d['pre'] = d['pre'] if not masked else T.slab_sum(d['slabs'][:, :M * 2 * R].reshape(splits, M, 2 * R)) + T.d64(d['bias'])
        want_a, want_b = not (splits == 5 and not masked), not (splits == 4 and not masked)
        o = fused_outputs(dev, T.CTX_GLU, M, R, d, want_a, want_b, True)
        L().check(L().lib.capmi_glu_fwd_fused(kp(d['slabs']), splits, d['stride'], kp(d['bias']), o['pre'].ptr(), o['out'].ptr(),
                                              kp(d['mask_a']), optr(o['out_a']), optr(o['pl_a']), kp(d['mask_b']), optr(o['out_b']),
                                              optr(o['pl_b']), M, R, L().stream_ptr()), 'glu_fwd_fused')
        check_fused(T.CTX_GLU, d, o, resid=False)
        # bit for bit the att2ctx stage of the GLU kind
        o2 = fused_outputs(dev, T.CTX_GLU, M, R, d, want_a, want_b, True)
        L().check(run_ctx(dev, kp, T.CTX_GLU, M, R, splits, dict(d, resid=None), o2), 'ctx_fwd_fused')
        torch.cuda.synchronize()
        for k in ('pre', 'out', 'out_a', 'out_b'):
            assert o[k] is None or torch.equal(o[k].t, o2[k].t), k
        for k in ('pl_a', 'pl_b'):
            assert o[k] is None or torch.equal(o[k], o2[k]), k


@pytest.mark.parametrize('M,R,splits', [(7, 36, 5), (64, 36, 9), (1, 4, 1)])
def test_glu_fwd_fused_equals_reduce_then_glu(dev, M, R, splits):
    lib, st = L().lib, L().stream_ptr()
    g = T.gen(M + splits)
    slabs = torch.randn(splits, M, 2 * R, generator=g).to(dev)
    bias, ma = torch.randn(2 * R, generator=g).to(dev), T.keep_mask(g, M, R).to(dev)
    pre, o, oa = (torch.empty(M, w, device=dev) for w in (2 * R, R, R))
    L().check(lib.capmi_splitk_reduce(slabs.data_ptr(), splits, pre.data_ptr(), 2 * R, M, 2 * R, bias.data_ptr(), None, None, 1, None, 0, 0, st),
              'reduce')
    L().check(lib.capmi_glu_fwd(pre.data_ptr(), None, None, o.data_ptr(), M, R, st), 'glu')
    L().check(lib.capmi_glu_fwd(pre.data_ptr(), ma.data_ptr(), None, oa.data_ptr(), M, R, st), 'glu')
    f = fused_outputs(dev, T.CTX_GLU, M, R, None, True, False, True)
    L().check(lib.capmi_glu_fwd_fused(slabs.data_ptr(), splits, M * 2 * R, bias.data_ptr(), f['pre'].ptr(), f['out'].ptr(), ma.data_ptr(),
                                      f['out_a'].ptr(), None, None, None, None, M, R, st), 'glu_fwd_fused')
    torch.cuda.synchronize()
    assert torch.equal(f['pre'].t, pre) and torch.equal(f['out'].t, o) and torch.equal(f['out_a'].t, oa)


@pytest.mark.parametrize('M,R', T.FUSED_SHAPES)
@pytest.mark.parametrize('kind', [T.CTX_GLU, T.CTX_RELU, T.CTX_LSTM])
def test_ctx_fwd_fused(dev, kind, M, R):
    for (_, _, _, splits, masked) in [c for c in T.CTX_FUSED if c[:3] == (kind, M, R)]:
        kp = Keep(dev)
        d = T.fused_inputs(kind, M, R, splits, masked, seed=7000 + 100 * kind + 10 * M + splits + masked)
        want_b = not (splits == 4 and not masked)
        want_pre = not (kind == T.CTX_LSTM and splits == 9)                      # the LSTM kind may go without its saved gates
        o = fused_outputs(dev, kind, M, R, d, True, want_b, want_pre)
        L().check(run_ctx(dev, kp, kind, M, R, splits, d, o), 'ctx_fwd_fused')
        check_fused(kind, d, o, resid=True)


# ------------------------------------------------------------------------------------------------ pointwise backwards, split
@pytest.mark.parametrize('M,R', [(1, 4), (7, 37), (65, 36)])
def test_relu_bwd_add(dev, M, R):
    for (_, _, splits, am) in [c for c in T.RELU_BWD if c[:2] == (M, R)]:
        kp = Keep(dev)
        d = T.add_inputs(M, R, splits, am, seed=8000 + M + (splits or 0) + am, glu=False)
        dp = out(dev, M, R)
        L().check(L().lib.capmi_relu_bwd_add(kp(d['d_out']), kp(d['slabs']), splits or 0, d['stride'], kp(d['add_mask']), kp(d['out']),
                                             dp.ptr(), M, R, L().stream_ptr()), 'relu_bwd_add')
        check('d_pre', dp.t, T.relu_bwd_ref(d), POINT)
        assert dp.guarded() and bool((dp.t.cpu()[d['out'] <= 0] == 0).all())


@pytest.mark.parametrize('M,R', [(1, 4), (7, 37), (65, 36)])
def test_glu_bwd_add(dev, M, R):
    for (_, _, splits, am) in [c for c in T.GLU_BWD if c[:2] == (M, R)]:
        kp = Keep(dev)
        d = T.add_inputs(M, R, splits, am, seed=8500 + M + (splits or 0) + am, glu=True)
        dp = out(dev, M, 2 * R)
        if splits:
            rc = L().lib.capmi_glu_bwd_add(kp(d['d_out']), kp(d['mask']), kp(d['slabs']), splits, d['stride'], kp(d['add_mask']), kp(d['pre']),
                                           dp.ptr(), M, R, L().stream_ptr())
        else:
            rc = L().lib.capmi_glu_bwd(kp(d['d_out']), kp(d['mask']), kp(d['pre']), dp.ptr(), M, R, L().stream_ptr())
        L().check(rc, 'glu_bwd')
        check('d_pre', dp.t, T.glu_bwd_ref(d), POINT)
        assert dp.guarded()


@pytest.mark.parametrize('M,R', [(1, 4), (7, 37), (65, 36)])
def test_split_halves(dev, M, R):
    for (_, _, splits, masked) in [c for c in T.SPLIT_HALVES if c[:2] == (M, R)]:
        kp = Keep(dev)
        d = T.split_inputs(M, R, splits, masked, seed=9000 + M + splits + masked)
        lo, hi = out(dev, M, R), out(dev, M, R)
        L().check(L().lib.capmi_split_halves(kp(d['slabs']), splits, d['stride'], kp(d['mask_lo']), kp(d['mask_hi']), lo.ptr(), hi.ptr(), M, R,
                                             L().stream_ptr()), 'split_halves')
        lo_ref, hi_ref = T.split_ref(d)
        check('lo', lo.t, lo_ref, POINT)
        check('hi', hi.t, hi_ref, POINT)
        assert lo.guarded() and hi.guarded()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    lib, st, EINVAL = L().lib, L().stream_ptr(), L().EINVAL
    z = torch.zeros(1 << 16, device=dev)
    zp = z.data_ptr()
    outs = []

    def o(*shape):
        outs.append(out(dev, *shape))
        return outs[-1].ptr()

    def fwd(Nq, qpk, Tq, Tk, h, dk, mask_tq=1, mask=None, q=zp):
        return lib.capmi_mha_fwd(q, zp, zp, Tk * h * dk, 0, mask, mask_tq, 0, 0, 0, None, o(Nq, Tq, h * dk), o(Nq, h, Tq, Tk), Nq, qpk, Tq, Tk,
                                 h, dk, st)

    def bwd(Nq, qpk, Tq, Tk, h, dk, q=zp):
        D = h * dk
        return lib.capmi_mha_bwd(zp, q, zp, zp, Tk * D, 0, zp, None, o(Nq, Tq, D), o(Nq // qpk or 1, Tk, D), o(Nq // qpk or 1, Tk, D), 0, 0, 0, Nq,
                                 qpk, Tq, Tk, h, dk, st)

    m8 = torch.ones(64, dtype=torch.uint8, device=dev).data_ptr()
    assert fwd(1, 1, 4, 200, 1, 128) == EINVAL and bwd(1, 1, 4, 200, 1, 128) == EINVAL            # more than 160 KB of LDS
    assert c_plan(0, 1, 1, 4, 200, 1, 128)[0] == EINVAL and c_plan(1, 1, 1, 4, 200, 1, 128)[0] == EINVAL
    assert fwd(2, 1, 3, 5, 2, 6) == EINVAL and bwd(2, 1, 3, 5, 2, 6) == EINVAL                      # dk % 4
    assert fwd(2, 1, 3, 5, 2, 8, mask_tq=2, mask=m8) == EINVAL                                      # mask_tq not in {1, Tq}
    assert fwd(3, 2, 3, 5, 2, 8) == EINVAL and bwd(3, 2, 3, 5, 2, 8) == EINVAL                      # Nq % q_per_kv
    assert fwd(2, 1, 3, 5, 2, 8, q=zp + 4) == EINVAL and bwd(2, 1, 3, 5, 2, 8, q=zp + 4) == EINVAL  # a misaligned pointer
    # LayerNorm
    for D in (1, ):
        assert lib.capmi_layernorm_fwd(zp, zp, zp, o(3, D), o(3), o(3), 3, D, T.EPS, st) == EINVAL
        assert lib.capmi_layernorm_bwd(zp, zp, zp, zp, zp, o(3, D), 0, o(3, D), 3, D, T.EPS, st) == EINVAL
    assert lib.capmi_layernorm_bwd_parts(zp, zp, zp, zp, zp, o(3, 2052), 0, o(1, 2052), o(1, 2052), 3, 2052, T.EPS, st) == EINVAL
    assert lib.capmi_layernorm_bwd_parts(zp, zp, zp, zp, zp, o(3, 1), 0, o(1, 1), o(1, 1), 3, 1, T.EPS, st) == EINVAL
    for D in (2052, 262, 1):
        assert lib.capmi_layernorm_bwd_slabs(zp, 1, 3 * D, o(3, D), zp, zp, zp, zp, zp, 1, 3 * D, D, o(3, D), o(3, D), 3, D, T.EPS, st) == EINVAL
    assert lib.capmi_layernorm_bwd_slabs(zp + 4, 1, 24, o(3, 8), zp, zp, zp, zp, zp, 1, 24, 8, o(3, 8), o(3, 8), 3, 8, T.EPS, st) == EINVAL
    # planes hold at most 64 rows
    M, R = 65, 4
    assert lib.capmi_glu_fwd_fused(zp, 1, M * 2 * R, None, o(M, 2 * R), o(M, R), None, o(M, R), planes_buf(dev, R).data_ptr(), None, None, None,
                                   M, R, st) == EINVAL
    assert lib.capmi_glu_fwd_fused(zp + 4, 1, 8, None, o(1, 8), o(1, 4), None, None, None, None, None, None, 1, 4, st) == EINVAL

    def ctx(kind, M, **kw):
        s = L().CtxStep()
        s.slabs, s.out, s.kind, s.splits, s.M, s.R, s.stride = zp, o(M, R), kind, 1, M, R, M * 4 * R
        for k, v in kw.items():
            setattr(s, k, v)
        return lib.capmi_ctx_fwd_fused(ctypes.byref(s), st)

    assert ctx(T.CTX_RELU, 65, out_a=o(65, R), planes_a=planes_buf(dev, R).data_ptr()) == EINVAL
    assert ctx(T.CTX_GLU, 3) == EINVAL                                                # the GLU kind without pre
    assert ctx(T.CTX_LSTM, 3, c_prev=zp, pre=o(3, 4 * R)) == EINVAL                   # the LSTM kind without c
    assert ctx(T.CTX_LSTM, 3, c=o(3, R)) == EINVAL                                    # ... without c_prev
    assert ctx(T.CTX_RELU, 3, resid=zp) == EINVAL                                     # a residual with no out_a to add it to
    assert ctx(3, 3, pre=o(3, 2 * R)) == EINVAL
    assert all(b.untouched() for b in outs)
