"""The grid-stride kernels past their launch cap on a real MI355X -- the second trip of the loop that carries almost all the bytes
of a training step at config size -- and the alignment arms of the same family that no caller takes: every row of
grid_wrap_ref64.CASES against the float64 reference its kernel already has, under the bound its existing parity test uses
(test_grid_wrap_host.py holds the rows to the launch arithmetic).  Kernels that are a single multiply, a select or a replayed
generator are compared bit for bit.  Every output is compared in full: a quad that trip 2 skipped, updated twice or updated with
another quad's state shows in the float64 parity."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid_wrap_ref64 as W
import optim_ref64 as O
import reduce_ref64 as R
import transformer_ref64 as T
from test_optim_gpu import HP, TOL
from test_step_kernels_gpu import CELL_FWD, L, dev, nan, ptr, put          # noqa: F401  (dev: the module's fixture)
from test_transformer_kernels_gpu import POINT

pytestmark = pytest.mark.gpu
GUARD = 4                            # floats in front of and behind every optimizer range
SENT = -24680.5


def ok(rc, what):
    assert rc == 0, (what, rc)


def same_bits(got, want):
    torch.cuda.synchronize()
    return torch.equal(R.bits(got), R.bits(want))


def guarded(dev, n, off=0, src=None):
    """a range of n floats that starts GUARD + off floats into a 16-byte aligned allocation of sentinels, GUARD more behind it
    -> (allocation, range)"""
    whole = torch.full((GUARD + off + n + GUARD,), SENT, device=dev)
    assert whole.data_ptr() % 16 == 0
    r = whole[GUARD + off:GUARD + off + n]
    r.copy_(src) if src is not None else r.zero_()
    return whole, r


def guards_intact(whole, n, off=0):
    lead = GUARD + off
    edge = torch.cat([whole[:lead], whole[lead + n:]])
    return bool((edge == SENT).all())


def clipped_some(g, scale, clip):
    hit = int(((g * scale).abs() > clip).sum())
    return 0 < hit < g.numel()


# ------------------------------------------------------------------------------------------------ (a) Adam
def adam_args(s):
    hp = R.ADAM_HP
    return (hp['lr'], hp['b1'], hp['b2'], hp['eps'], s['wd'], s['clip'], s['scale'])


@pytest.mark.parametrize('cid', ['adam2', 'adam tail'])
def test_adam_wraps(dev, cid):
    """capmi_adam_step at a count whose quad loop takes a second trip: adam2_kernel with q1 live on 300 threads of trip 2 and dead on
    the rest, adam_kernel with trip 2 and the scalar tail.  Two steps from zero moments under the 'all' set (clip, decay, scale), p,
    m and v after each against the float64 formula; the gradient and 4 guard floats around every range keep their bits.  At the
    adam2 count capmi_adam_step_dyn gives the same bits.  Bounds (rel_err): ADAM_FACTOR = 4 x the error of the float32 torch
    restatement (reduce_ref64.adam32 against adam64) on these same inputs after the two steps -- measured (p, m, v) and the bounds:
      adam2      6 292 656  7.964e-08 1.100e-07 1.731e-07 -> 3.19e-07, 4.40e-07, 6.92e-07
      adam tail  2 098 355  8.760e-08 1.092e-07 1.854e-07 -> 3.50e-07, 4.37e-07, 7.42e-07"""
    count = W.shape_of(cid)['count']
    s, hp = R.ADAM_SETS['all'], R.ADAM_HP
    g = R.gen(77 + count % 1000)
    p0 = torch.randn(count, generator=g)
    grads = [torch.randn(count, generator=g) * 0.3 for _ in range(2)]
    assert all(clipped_some(gr, s['scale'], s['clip']) for gr in grads)
    refs = R.adam64(p0, grads, **s)
    f32 = R.adam32(p0, grads, **s)
    errs = [R.rel_err(a, b) for a, b in zip(f32, refs[-1])]
    bounds = [R.ADAM_FACTOR * e for e in errs]
    print('adam wrap[%s, %d] float32 restatement rel_err p %.3e m %.3e v %.3e -> bounds %.2e %.2e %.2e' % ((cid, count) + tuple(errs) + tuple(bounds)))
    assert all(1e-9 < e < 1e-6 for e in errs), errs
    lib, st = L().lib, L().stream_ptr()
    bufs = [guarded(dev, count, src=p0.to(dev)), guarded(dev, count), guarded(dev, count)]
    (pw, p), (mw, m), (vw, v) = bufs
    gw, g_d = guarded(dev, count)
    dyn = cid == 'adam2'
    if dyn:
        twin = [p.clone(), m.clone(), v.clone()]
        state = torch.zeros(32, dtype=torch.uint8, device=dev)
        ok(lib.capmi_step_set_lr(ptr(state), hp['lr'], st), 'step_set_lr')
    for t, gr in enumerate(grads, 1):
        g_d.copy_(gr)
        ok(lib.capmi_adam_step(ptr(p), ptr(g_d), ptr(m), ptr(v), count, *adam_args(s), t, st), 'adam_step')
        if dyn:
            ok(lib.capmi_step_advance(ptr(state), hp['b1'], hp['b2'], st), 'step_advance')
            ok(lib.capmi_adam_step_dyn(ptr(twin[0]), ptr(g_d), ptr(twin[1]), ptr(twin[2]), count, ptr(state), hp['b1'], hp['b2'], hp['eps'],
                                       s['wd'], s['clip'], s['scale'], st), 'adam_step_dyn')
        torch.cuda.synchronize()
        assert torch.equal(g_d.cpu(), gr)
        assert all(guards_intact(w, count) for w in (pw, mw, vw, gw))
        for what, got, ref, bound in zip('pmv', (p, m, v), refs[t - 1], bounds):
            e = R.rel_err(got, ref)
            print('adam wrap[%s] step %d %s rel_err %.2e (bound %.2e)' % (cid, t, what, e, bound))
            assert bool(torch.isfinite(got).all()) and e < bound, (what, t, e, bound)
        if dyn:
            for x, y in zip((p, m, v), twin):
                assert same_bits(x, y), t


# ------------------------------------------------------------------------------------------------ (a) the other rules
def optim_run(dev, rule, n, offs, steps=2, dyn=False, seed=0):
    """`steps` steps of capmi_optim_step (or _dyn) under the 'all' setting on guarded ranges at the given element offsets ->
    per step (p, states...) on the CPU; asserts the gradient and the guards after every step"""
    from imagecaptioning.pytorch_amd import ops
    alpha, beta, eps = HP[rule]
    keys = O.STATE_KEYS[rule]
    g = torch.Generator().manual_seed(1000 + n % 997 + seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.3 for _ in range(steps)]
    assert n < 100 or all(clipped_some(gr, 0.5, 0.1) for gr in grads)
    bufs = [guarded(dev, n, off) for off in offs[:2 + len(keys)]]
    assert len(bufs) == 2 + len(keys)
    (pw, p), (gw, gd), state = bufs[0], bufs[1], [b[1] for b in bufs[2:]]
    for (w, r), off in zip(bufs, offs):
        assert r.data_ptr() % 16 == (4 * off) % 16
    p.copy_(p0)
    st = ops.StepState(torch.device(dev), lr=0.0) if dyn else None
    out = []
    for t in range(1, steps + 1):
        lr = 1e-2 / t
        gd.copy_(grads[t - 1])
        s2 = state[1] if len(state) > 1 else None
        if dyn:
            st.set_lr(lr)
            st.advance(alpha, beta)
            ops.optim_step_dyn(rule, p, gd, state[0], s2, st, alpha, beta, eps, 0.01, 0.1, 0.5)
        else:
            ops.optim_step(rule, p, gd, state[0], s2, lr, alpha, beta, eps, 0.01, 0.1, 0.5, t)
        torch.cuda.synchronize()
        assert torch.equal(gd.cpu(), grads[t - 1]), (rule, n, t, 'the gradient was written')
        assert all(guards_intact(w, n, off) for (w, _), off in zip(bufs, offs)), (rule, n, t, 'a guard float was written')
        out.append([p.cpu()] + [x.cpu() for x in state])
    return p0, grads, out


def optim_replay(rule, p0, grads):
    alpha, beta, eps = HP[rule]
    p64, st64, out = p0.double(), O.new_state(rule, p0), []
    for t, gr in enumerate(grads, 1):
        O.step(rule, p64, gr, st64, O.f32(1e-2 / t), t, alpha=O.f32(alpha), beta=O.f32(beta), eps=O.f32(eps), weight_decay=O.f32(0.01),
               clip=O.f32(0.1), grad_scale=O.f32(0.5))
        out.append([p64.clone()] + [st64[k].clone() for k in O.STATE_KEYS[rule]])
    return out


OPTIM_SHAPES = [('quads wrap', W.OPT_ALIGNED['n'], W.OPT_ALIGNED['offs']), ('scalar wrap', W.T + 300, W.OPT_MIXED)] + \
               [('scalar single', n, offs) for n, offs in W.OPTIM_SCALAR_SINGLE]


@pytest.mark.parametrize('rule', O.RULES)
@pytest.mark.parametrize('what,n,offs', OPTIM_SHAPES, ids=['%s-%d' % (w, n) for w, n, _ in OPTIM_SHAPES])
def test_optim_wraps(dev, rule, what, n, offs):
    """capmi_optim_step, two steps (the state carry crosses the wrap) with clip 0.1, decay 0.01 and scale 0.5 on 0.3 randn gradients:
    p and every state buffer after each step within TOL = 1e-6 of the float64 replay (test_optim_gpu.py's bound), the gradient and
    the 4 guard floats around every range untouched.
      quads wrap     the range starts 1 element into its allocation: head 3, 3 T + 300 quads (trip 2 of the quad loop with q1 live
                     on 300 threads, dead on the rest), tail 2
      scalar wrap    buffers at pairwise different offsets: no common quad grid, scalar throughout, T + 300 elements: trip 2 of the
                     scalar loop
      scalar single  the same offsets at 1, 5 and 1023 elements
    capmi_optim_step_dyn gives the bits of the stepped form at the two wrap shapes."""
    p0, grads, got = optim_run(dev, rule, n, offs)
    ref = optim_replay(rule, p0, grads)
    names = ('p',) + O.STATE_KEYS[rule]
    for t, (gs, rs) in enumerate(zip(got, ref), 1):
        for k, a, b in zip(names, gs, rs):
            e = float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))
            print('optim wrap[%s, %s, %d] step %d %s rel_err %.2e (bound %.0e)' % (rule, what, n, t, k, e, TOL))
            assert bool(torch.isfinite(a).all()) and e < TOL, (rule, what, t, k, e)
    if 'wrap' in what:
        _, _, twin = optim_run(dev, rule, n, offs, dyn=True)
        for gs, ts in zip(got, twin):
            for k, a, b in zip(names, gs, ts):
                assert torch.equal(R.bits(a), R.bits(b)), (rule, what, k)


# ------------------------------------------------------------------------------------------------ (b) pointwise.hip
def test_relu_jacobians_wrap(dev):
    """relu_mask_bwd (a thread per element) and relu_scale_bwd (a thread per quad) 300 items past 2048 x 256: bit for bit, as
    test_reduce_kernels_gpu.py compares them, and nothing behind the count"""
    lib, st = L().lib, L().stream_ptr()
    count = W.shape_of('relu_mask_bwd')['count']
    dy, y, mask = R.relu_inputs(count, seed=3)
    keep = [put(dev, t) for t in (dy, y, mask)]
    for with_y, with_mask in ((True, True), (False, False)):
        dx = nan(dev, count + 1)
        ok(lib.capmi_relu_mask_bwd(ptr(keep[0]), ptr(keep[1]) if with_y else None, ptr(keep[2]) if with_mask else None, ptr(dx), count, st),
           'relu_mask_bwd')
        assert same_bits(dx[:count], R.relu_mask_bwd(dy, y if with_y else None, mask if with_mask else None))
        assert bool(torch.isnan(dx[count:]).all())
    count = W.shape_of('relu_scale_bwd')['count']
    scale = float(np.float32(1.0 / 0.7))
    dy, y, _ = R.relu_inputs(count, seed=4)
    dx = nan(dev, count + 4)
    dy_d, y_d = put(dev, dy), put(dev, y)
    ok(lib.capmi_relu_scale_bwd(ptr(dy_d), ptr(y_d), scale, ptr(dx), count, st), 'relu_scale_bwd')
    assert same_bits(dx[:count], R.relu_scale_bwd(dy, y, scale))
    assert bool(torch.isnan(dx[count:]).all())


def test_dropout_masks_wrap(dev):
    """the Philox quad of element quad q is drawn at counter offset + q, so the part of a wrapping launch that trip 2 writes is, bit
    for bit, a single-trip launch at offset + 2048 x 256; capmi_dropout_masks, whose longest segment decides the grid, gives the
    bits of capmi_dropout_mask for every segment, the short ones in front of and behind the long one included.
    A self-consistency check, not an independent replay of the generator: the reference is the same kernel in launches of one trip
    (whose rate and sharing with the other entry points other tests hold), so a wrong counter or index in trip 2 shows, and a
    defect common to every trip does not; the {0, 2} values and the keep rate are all that stands against the latter here."""
    lib, st = L().lib, L().stream_ptr()
    seed, p = 24681357, 0.5
    count = W.shape_of('dropout_mask')['count']
    whole = nan(dev, count + 1)
    ok(lib.capmi_dropout_mask(ptr(whole), count, p, seed, 5, st), 'dropout_mask')
    first, rest = nan(dev, 4 * W.T + 1), nan(dev, count - 4 * W.T + 1)
    ok(lib.capmi_dropout_mask(ptr(first), 4 * W.T, p, seed, 5, st), 'dropout_mask')
    ok(lib.capmi_dropout_mask(ptr(rest), count - 4 * W.T, p, seed, 5 + W.T, st), 'dropout_mask')
    assert W.arm('dropout_mask', dict(count=4 * W.T)) == 'trip 1'
    assert same_bits(whole[:4 * W.T], first[:4 * W.T]) and same_bits(whole[4 * W.T:], rest)       # the NaN guard included
    assert set(whole[:count].unique().tolist()) == {0.0, 2.0} and 0.49 < float((whole[:count] == 0).float().mean()) < 0.51
    counts = W.shape_of('dropout_masks')['counts']
    descs = (L().MaskDesc * len(counts))()
    got, want = [], []
    for k, c in enumerate(counts):
        buf = nan(dev, c + 1)
        descs[k].mask, descs[k].count, descs[k].offset = ptr(buf), c, k << 40
        descs[k].row_len, descs[k].rows, descs[k].keep_from = 0, 0, -1
        got.append(buf)
        one = nan(dev, c + 1)
        ok(lib.capmi_dropout_mask(ptr(one), c, p, seed, k << 40, st), 'dropout_mask')
        want.append(one)
    ok(lib.capmi_dropout_masks(descs, len(counts), p, seed, st), 'dropout_masks')
    for c, a, b in zip(counts, got, want):
        assert same_bits(a, b), c


# ------------------------------------------------------------------------------------------------ (b) transformer.hip / aoa_ctx.hip
def close(name, got, ref, tol):
    torch.cuda.synchronize()
    got = got.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), name
    e = float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
    print('%s rel_err %.2e (bound %.0e)' % (name, e, tol))
    assert e < tol, (name, e)


def tail_nan(buf, n):
    return bool(torch.isnan(buf.view(-1)[n:]).all())


def test_glu_family_wraps(dev):
    """glu_fwd, glu_bwd (plain and with added slabs), split_halves and relu_bwd_add at R = 64 with the row count carrying M R (2 M R
    for split_halves) 1024 past 4096 x 256: the references and the bound (POINT, CELL_FWD for glu_fwd) of their existing tests"""
    lib, st = L().lib, L().stream_ptr()
    M, Rr = W.GLU_M, W.GLU_R
    g = T.gen(11)
    pre = (torch.randn(M, 2 * Rr, generator=g) * 3).float()
    mask, res = T.keep_mask(g, M, Rr, 0.5), torch.randn(M, Rr, generator=g).float()
    pre_d, mask_d, res_d = put(dev, pre), put(dev, mask), put(dev, res)
    ref = pre[:, :Rr].double() * torch.sigmoid(pre[:, Rr:].double())
    for m, r in ((mask_d, res_d), (None, None)):
        out = nan(dev, M * Rr + 8)
        ok(lib.capmi_glu_fwd(ptr(pre_d), ptr(m), ptr(r), ptr(out), M, Rr, st), 'glu_fwd')
        close('glu_fwd wrap', out[:M * Rr].view(M, Rr), ref if m is None else res.double() + mask.double() * ref, CELL_FWD)
        assert tail_nan(out, M * Rr)
    for splits, am in ((None, False), (2, True)):
        d = T.add_inputs(M, Rr, splits, am, seed=21 + (splits or 0), glu=True)
        k = {n: put(dev, d[n]) for n in ('d_out', 'mask', 'slabs', 'add_mask', 'pre')}
        dp = nan(dev, M * 2 * Rr + 8)
        ok(lib.capmi_glu_bwd_add(ptr(k['d_out']), ptr(k['mask']), ptr(k['slabs']), splits or 0, d['stride'], ptr(k['add_mask']), ptr(k['pre']),
                                 ptr(dp), M, Rr, st), 'glu_bwd_add')
        close('glu_bwd wrap', dp[:M * 2 * Rr].view(M, 2 * Rr), T.glu_bwd_ref(d), POINT)
        assert tail_nan(dp, M * 2 * Rr)
        d = T.add_inputs(M, Rr, splits, am, seed=31 + (splits or 0), glu=False)
        k = {n: put(dev, d[n]) for n in ('d_out', 'slabs', 'add_mask', 'out')}
        dp = nan(dev, M * Rr + 8)
        ok(lib.capmi_relu_bwd_add(ptr(k['d_out']), ptr(k['slabs']), splits or 0, d['stride'], ptr(k['add_mask']), ptr(k['out']), ptr(dp), M, Rr,
                                  st), 'relu_bwd_add')
        close('relu_bwd_add wrap', dp[:M * Rr].view(M, Rr), T.relu_bwd_ref(d), POINT)
        assert tail_nan(dp, M * Rr) and bool((dp[:M * Rr].view(M, Rr).cpu()[d['out'] <= 0] == 0).all())
    Mh = W.shape_of('split_halves')['M']
    for splits, masked in ((1, False), (2, True)):
        d = T.split_inputs(Mh, Rr, splits, masked, seed=41 + splits)
        k = {n: put(dev, d[n]) for n in ('slabs', 'mask_lo', 'mask_hi')}
        lo, hi = nan(dev, Mh * Rr + 8), nan(dev, Mh * Rr + 8)
        ok(lib.capmi_split_halves(ptr(k['slabs']), splits, d['stride'], ptr(k['mask_lo']), ptr(k['mask_hi']), ptr(lo), ptr(hi), Mh, Rr, st),
           'split_halves')
        lo_ref, hi_ref = T.split_ref(d)
        close('split_halves lo wrap', lo[:Mh * Rr].view(Mh, Rr), lo_ref, POINT)
        close('split_halves hi wrap', hi[:Mh * Rr].view(Mh, Rr), hi_ref, POINT)
        assert tail_nan(lo, Mh * Rr) and tail_nan(hi, Mh * Rr)


@pytest.mark.parametrize('kind', ['glu_fwd_fused', T.CTX_GLU, T.CTX_RELU, T.CTX_LSTM], ids=['glu_fwd_fused', 'ctx-glu', 'ctx-relu', 'ctx-lstm'])
def test_fused_forwards_wrap(dev, kind):
    """glu_fwd_fused and the three kinds of ctx_fwd_fused, a thread per 4 columns: R = 64 and 65 600 rows put M (R / 4) 1024 past
    4096 x 256.  Two slabs, both masks, no planes (M > 64); fused_ref and POINT as in test_transformer_kernels_gpu.py"""
    lib, st = L().lib, L().stream_ptr()
    M, Rr, splits = W.FUSED_M, W.GLU_R, 2
    ck = T.CTX_GLU if kind == 'glu_fwd_fused' else kind
    G = T.CTX_G[ck]
    d = T.fused_inputs(ck, M, Rr, splits, True, seed=50 + ck)
    if kind == 'glu_fwd_fused':
        d['pre'] = d['pre'] - T.d64(d['bias2'])
        d['bias2'] = d['resid'] = None
    k = {n: put(dev, d.get(n)) for n in ('slabs', 'bias', 'bias2', 'c_prev', 'resid', 'mask_a', 'mask_b')}
    o = dict(pre=nan(dev, M * G * Rr + 8), out=nan(dev, M * Rr + 8), c=nan(dev, M * Rr + 8) if ck == T.CTX_LSTM else None,
             out_a=nan(dev, M * Rr + 8), out_b=nan(dev, M * Rr + 8))
    if kind == 'glu_fwd_fused':
        ok(lib.capmi_glu_fwd_fused(ptr(k['slabs']), splits, d['stride'], ptr(k['bias']), ptr(o['pre']), ptr(o['out']), ptr(k['mask_a']),
                                   ptr(o['out_a']), None, ptr(k['mask_b']), ptr(o['out_b']), None, M, Rr, st), 'glu_fwd_fused')
    else:
        s = L().CtxStep()
        for n in k:
            setattr(s, n, ptr(k[n]))
        s.pre, s.c, s.out, s.out_a, s.planes_a, s.out_b, s.planes_b = ptr(o['pre']), ptr(o['c']), ptr(o['out']), ptr(o['out_a']), None, \
            ptr(o['out_b']), None
        s.stride, s.kind, s.splits, s.M, s.R = d['stride'], ck, splits, M, Rr
        ok(lib.capmi_ctx_fwd_fused(C.byref(s), st), 'ctx_fwd_fused')
    saved, c_ref, out_ref, oa_ref, ob_ref = T.fused_ref(ck, d)
    torch.cuda.synchronize()
    if saved is None:
        assert bool(torch.isnan(o['pre']).all()), 'the ReLU kind wrote pre'
    else:
        close('pre', o['pre'][:M * G * Rr].view(M, G * Rr), saved, POINT)
        assert tail_nan(o['pre'], M * G * Rr)
    for n, ref in (('out', out_ref), ('c', c_ref), ('out_a', oa_ref), ('out_b', ob_ref)):
        if ref is not None:
            close(n, o[n][:M * Rr].view(M, Rr), ref, POINT)
            assert tail_nan(o[n], M * Rr), n


def test_embed_pe_fwd_wraps(dev):
    """embed_pe_fwd with N T D 1024 past 4096 x 256, with and without the dropout mask: every element within 3 * 2^-24 of its
    magnitude, the rule of test_reduce_kernels_gpu.test_embed_pe_fwd"""
    s = W.shape_of('embed_pe_fwd')
    N, Tt, D, tok_ld, pos0 = s['N'], s['T'], s['D'], s['T'] + 1, 2
    tok, E, pe, dr, _ = R.embed_pe_inputs(N, Tt, D, tok_ld, 5, 811, pos0 + Tt)
    keep = [put(dev, t) for t in (tok, E, pe, dr)]
    for drop in (keep[3], None):
        x = nan(dev, N * Tt * D + 8)
        ok(L().lib.capmi_embed_pe_fwd(ptr(keep[0]), tok_ld, ptr(keep[1]), ptr(keep[2]), ptr(drop), ptr(x), N, Tt, D, pos0, L().stream_ptr()),
           'embed_pe_fwd')
        torch.cuda.synchronize()
        ref, mag = R.embed_pe_fwd(tok, E, pe, dr if drop is not None else None, Tt, pos0)
        got = x[:N * Tt * D].view(N, Tt, D).double().cpu()
        assert bool(torch.isfinite(got).all()) and tail_nan(x, N * Tt * D)
        over = (got - ref).abs() - 3 * 2.0 ** -24 * mag
        print('embed_pe_fwd wrap max err / magnitude %.2e (bound %.2e)' % (float(((got - ref).abs() / (mag + 1e-30)).max()), 3 * 2.0 ** -24))
        assert float(over.max()) <= 0.0


def test_embed_pe_bwd_wraps(dev):
    """embed_pe_bwd_kernel is the atomicAdd arm of capmi_embed_pe_bwd (the deterministic arm is one workgroup per position, no capped
    grid): 16 400 positions are past EBD_MAX_ROWS, so D = 64 takes it with N T D 1024 past 4096 x 256.  With and without the dropout
    mask against R.embed_pe_bwd under the bound of test_reduce_kernels_gpu.test_embed_pe_bwd (grads_close: dE starts at FILL,
    max|got - FILL - ref| <= EMBED_TOL max(1, max|ref|)); every row of dE is compared, nothing behind it is written.  257 table
    rows: about 64 addends per element, so the order the atomics land in moves a sum by far less than the bound (with 7 rows, 2 700
    addends each, one run measured 0.78 of it)"""
    from test_reduce_kernels_gpu import grads_close
    s = W.shape_of('embed_pe_bwd')
    N, Tt, D, V = s['N'], s['T'], s['D'], 257
    assert N * Tt > R.EBD_MAX_ROWS
    tok, _, _, dr, dx = R.embed_pe_inputs(N, Tt, D, Tt + 1, V, 911, 1)
    tok_d, dx_d, dr_d = put(dev, tok), put(dev, dx), put(dev, dr)
    for drop in (dr, None):
        ref = R.embed_pe_bwd(tok, dx, drop, Tt, V)
        dE = nan(dev, V * D + 8)
        dE[:V * D] = R.FILL
        ok(L().lib.capmi_embed_pe_bwd(ptr(tok_d), Tt + 1, ptr(dx_d), ptr(dr_d) if drop is not None else None, ptr(dE), N, Tt, D,
                                      L().stream_ptr()), 'embed_pe_bwd')
        torch.cuda.synchronize()
        grads_close('embed_pe_bwd wrap[%d positions, atomic(rows>max)]' % (N * Tt), dE[:V * D].view(V, D).cpu(), ref)
        assert tail_nan(dE, V * D)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_rows_narrow_wraps(dev, dtype):
    """rows_narrow_kernel 300 16-byte stores past 2048 x 256, both dtypes: a destination on a 16-byte boundary (16-byte source
    loads, tail 3) and one element past it (head 7, dword source loads, tail 3).  Every element equals src.to(dtype) on the device as
    int16, NaN as a class, and nothing outside the destination is written -- the comparison of
    test_resident_compact_gpu.test_narrow_is_torchs_conversion_bit_for_bit, its special values and magnitudes included"""
    from imagecaptioning.pytorch_amd import ops
    from test_resident_compact_gpu import SENT16, TORCH, _same_bits_nan_as_a_class, _specials
    sp = _specials()
    for cid in ('rows_narrow', 'rows_narrow head'):
        s = W.shape_of(cid)
        count, off = s['count'], s['dst_off']
        rng = np.random.default_rng(count)
        more = count - len(sp)
        vals = np.concatenate([(rng.standard_normal(more) * 10.0 ** rng.integers(-9, 6, more)).astype(np.float32), sp])   # specials in trip 2
        src = torch.from_numpy(vals).to(dev)
        buf = torch.full((count + 24,), SENT16, dtype=torch.int16, device=dev).view(TORCH[dtype])
        dst = buf[off:off + count]
        assert dst.data_ptr() % 16 == 2 * off and src.data_ptr() % 16 == 0
        ops.rows_narrow(src, dst)
        torch.cuda.synchronize()
        assert _same_bits_nan_as_a_class(dst, src.to(TORCH[dtype])), (dtype, cid)
        raw = buf.view(torch.int16)
        assert bool((raw[:off] == SENT16).all()) and bool((raw[off + count:] == SENT16).all()), (dtype, cid)


def test_meanpool_bwd_wraps(dev):
    """meanpool_bwd with B K D 1024 past 4096 x 256, masked and accumulating: the reference and CELL_FWD of
    test_step_kernels_gpu.test_meanpool_fwd_bwd"""
    s = W.shape_of('meanpool_bwd')
    B, K, D = s['B'], s['K'], s['D']
    g = T.gen(B + D)
    x, dm = torch.randn(B, K, D, generator=g).float(), torch.randn(B, D, generator=g).float()
    mask = (torch.arange(K).unsqueeze(0) < torch.randint(1, K + 1, (B, 1), generator=g)).float()
    dm_d, m_d = put(dev, dm), put(dev, mask)
    for m in (mask, None):
        md = torch.ones(B, K, dtype=torch.float64) if m is None else m.double()
        ref_dx = (md / md.sum(1, keepdim=True)).unsqueeze(2) * dm.double().unsqueeze(1)
        for acc in (0, 1):
            dx = nan(dev, B * K * D + 8)
            if acc:
                dx[:B * K * D] = put(dev, x).view(-1)
            ok(L().lib.capmi_meanpool_bwd(ptr(dm_d), ptr(m_d) if m is not None else None, ptr(dx), acc, B, K, D, L().stream_ptr()), 'meanpool_bwd')
            close('meanpool_bwd wrap', dx[:B * K * D].view(B, K, D), ref_dx + (x.double() if acc else 0.0), CELL_FWD)
            assert tail_nan(dx, B * K * D)


# ------------------------------------------------------------------------------------------------ (c) the PPO scalar cut
PPO_N, PPO_L, PPO_n = 6, 3, 3
# (ld_new, ld_old, ld_grad as V1 + this; the side whose base sits 4 bytes into its allocation; vec of the forward, of the backward)
PPO_LAYOUTS = {
    'new pitch V1+1': ((1, 0, 0), None, 0, 1),
    'grad pitch V1+2': ((0, 0, 2), None, 1, 0),
    'all pitch V1+4': ((4, 4, 4), None, 1, 1),
    'new 4 bytes in': ((0, 0, 0), 'new', 0, 1),
    'grad 4 bytes in': ((0, 0, 0), 'grad', 1, 0),
}


def same_phase16(pa, lda, pb, ldb):
    """csrc/host_common.h same_phase16"""
    return ((pa ^ pb) & 15) == 0 and (lda - ldb) % 4 == 0


def pitched_rows(dev, src, ld, off, fill):
    """the [N, L, V1] tensor as rows of pitch ld in a `fill`-filled allocation, `off` floats past a 16-byte boundary -> (the
    allocation, the raw rows [N L, ld], the [N, L, V1] view)"""
    N, Lq, V1 = src.shape
    buf = torch.full((N * Lq * ld + 4,), fill, device=dev)
    assert buf.data_ptr() % 16 == 0
    raw = buf[off:off + N * Lq * ld].view(N * Lq, ld)
    view = raw.view(N, Lq, ld)[:, :, :V1]
    view.copy_(src)
    return buf, raw, view


@pytest.mark.parametrize('per_row', (False, True))
@pytest.mark.parametrize('V1', (11, 128))
@pytest.mark.parametrize('layout', sorted(PPO_LAYOUTS))
def test_ppo_scalar_cut_and_row_pitch(dev, layout, V1, per_row):
    """capmi_ppo_loss_fwd / _bwd through the C ABI with descriptors ops._ppo_desc never builds: row pitches above V1 and bases 4
    bytes into their allocation, so that same_phase16 fails for the forward (vec == 0), for the backward, or holds with a pitch.
    Held to ppo64 with the bounds of test_ppo_gpu._check_kernel; the pad columns of lp_new and lp_old hold NaN (a read of them
    shows), those of grad keep their bits."""
    from test_ppo_gpu import _inputs, check_against_ppo64, upstream
    (dn, do, dg), shifted, vec_fwd, vec_bwd = PPO_LAYOUTS[layout]
    N, Lq, n = PPO_N, PPO_L, PPO_n
    eps, klc = 0.2, 0.02
    ln, lo, seq, scores = _inputs(N, Lq, V1, n, seed=V1 + 7)
    _, _, ln_v = pitched_rows(dev, ln, V1 + dn, 1 if shifted == 'new' else 0, float('nan'))
    _, _, lo_v = pitched_rows(dev, lo, V1 + do, 0, float('nan'))
    buf_g, raw_g, grad = pitched_rows(dev, torch.full((N, Lq, V1), float('nan')), V1 + dg, 1 if shifted == 'grad' else 0, SENT)
    assert same_phase16(ln_v.data_ptr(), V1 + dn, lo_v.data_ptr(), V1 + do) == bool(vec_fwd)
    assert same_phase16(grad.data_ptr(), V1 + dg, lo_v.data_ptr(), V1 + do) == bool(vec_bwd)
    u = upstream(N, per_row)
    rs = nan(dev, 4, N, Lq)
    msum, out = nan(dev, N if per_row else 1), nan(dev, 4)
    loss_rows = nan(dev, N) if per_row else None
    p = L().Ppo()
    p.N, p.L, p.V1, p.n = N, Lq, V1, n
    p.ld_new, p.ld_old, p.ld_grad = V1 + dn, V1 + do, V1 + dg
    p.per_row, p.eps, p.kl_coef = int(per_row), eps, klc
    p.lp_new, p.lp_old, p.seq, p.scores = ln_v.data_ptr(), lo_v.data_ptr(), seq.data_ptr(), scores.data_ptr()
    p.row_stats, p.msum, p.out, p.loss_rows = rs.data_ptr(), msum.data_ptr(), out.data_ptr(), ptr(loss_rows)
    p.g_out, p.grad = u.data_ptr(), grad.data_ptr()
    lib, st = L().lib, L().stream_ptr()
    ok(lib.capmi_ppo_loss_fwd(C.byref(p), st), 'ppo_loss_fwd')
    ok(lib.capmi_ppo_loss_bwd(C.byref(p), st), 'ppo_loss_bwd')
    check_against_ppo64(out, loss_rows, rs, grad, ln, lo, seq, scores, n, eps, klc, per_row, u)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all())
    if dg:
        assert bool((raw_g[:, V1:] == SENT).all()), 'a pad column of grad was written'
    lead, used = raw_g.storage_offset(), raw_g.numel()
    assert bool((buf_g[:lead] == SENT).all()) and bool((buf_g[lead + used:] == SENT).all()), 'wrote in front of or behind grad'
