"""The reduction, embedding, ReLU-Jacobian, Adam and dropout-mask kernels through the C ABI against the float64 references of
reduce_ref64.py, one case per dispatch arm (16-byte vs scalar, single pass vs row split, every loop tail, deterministic vs atomicAdd,
adam2_kernel vs adam_kernel): the case tables there say which arm a row reaches, test_reduce_kernels_host.py holds them to the
dispatch predicates.  Outputs start as NaN unless the call adds into them, the pad of every pitched input is NaN, every output
element is compared and every return code is asserted.  Metric and bounds are those of test_kernels_gpu.py: column and grouped row
sums rel_err = max|got - ref| / max|ref| < 2e-6; embedding gradients max|got - fill - ref| <= 2e-6 * max(1, max|ref|); Adam see
test_adam_step.  Gathers, selects and single multiplies are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import reduce_ref64 as R
from test_step_kernels_gpu import L, dev, nan, planes_buf, ptr, put, same_planes      # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu


def ok(rc, what):
    assert rc == 0, (what, rc)


def sums_close(name, got, ref):
    torch.cuda.synchronize()
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), name
    e = R.rel_err(got, ref)
    print('%s rel_err %.2e (bound %.0e)' % (name, e, R.COLSUM_TOL))
    assert e < R.COLSUM_TOL, (name, e)


def same_bits(got, want):
    torch.cuda.synchronize()
    return torch.equal(R.bits(got), R.bits(want))


# ------------------------------------------------------------------------------------------------ capmi_colsum
@pytest.mark.parametrize('i', range(len(R.COLSUM)))
def test_colsum(dev, i):
    rows, cols, ld, off, acc, arm = R.COLSUM[i]
    x = R.pitched(rows, cols, ld, seed=i)
    out0 = torch.randn(cols, generator=R.gen(100 + i)) if acc else None
    x_d = put(dev, x, off)
    buf = nan(dev, cols + 1)                        # the output and one guard element behind it
    if acc:
        buf[:cols] = put(dev, out0)
    ok(L().lib.capmi_colsum(ptr(x_d), rows, cols, ld, ptr(buf), acc, L().stream_ptr()), 'colsum')
    sums_close('colsum[%s]' % arm, buf[:cols], R.colsum(x, cols, out0))
    assert bool(torch.isnan(buf[cols:]).all())


def test_colsum_rejects_empty(dev):
    x, out = torch.zeros(4, 4, device=dev), torch.zeros(4, device=dev)
    lib = L().lib
    assert lib.capmi_colsum(ptr(x), 0, 4, 4, ptr(out), 0, L().stream_ptr()) == L().EINVAL
    assert lib.capmi_colsum(ptr(x), 4, 0, 4, ptr(out), 0, L().stream_ptr()) == L().EINVAL


# ------------------------------------------------------------------------------------------------ batched column sums
def batch_items(dev):
    """the items of R.COLSUM_BATCH on the device: ctypes items, their outputs (out, out2 or None) and float64 references"""
    items, outs, refs, held = [], [], [], []
    for i, (rows, cols, ld, off, acc, out2, _) in enumerate(R.COLSUM_BATCH):
        x = R.pitched(rows, cols, ld, seed=200 + i)
        out0 = torch.randn(cols, generator=R.gen(300 + i)) if acc else None
        x_d = put(dev, x, off)
        o = put(dev, out0) if acc else nan(dev, cols)
        o2 = nan(dev, cols) if out2 else None
        held.append(x_d)
        it = L().ColsumItem()
        setattr(it, 'in', ptr(x_d))
        it.out, it.out2, it.rows, it.cols, it.ld, it.accumulate = ptr(o), ptr(o2), rows, cols, ld, acc
        items.append(it)
        outs.append((o, o2))
        refs.append(R.colsum(x, cols, out0))
    return items, outs, refs, held


def check_batch(name, outs, refs):
    for i, ((o, o2), ref) in enumerate(zip(outs, refs)):
        sums_close('%s item %d [%s]' % (name, i, R.COLSUM_BATCH[i][-1]), o, ref)
        if o2 is not None:
            assert same_bits(o2, o), (name, i, 'out2')


def test_colsum_batch_device_items(dev):
    items, outs, refs, held = batch_items(dev)
    arr = (L().ColsumItem * len(items))(*items)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    ok(L().lib.capmi_colsum_batch(ptr(table), len(items), L().stream_ptr()), 'colsum_batch')
    check_batch('colsum_batch', outs, refs)


def test_colsum_batch_args_eight_host_items(dev):
    items, outs, refs, held = batch_items(dev)
    assert len(items) == R.COLSUM_ARGS_MAX
    arr = (L().ColsumItem * len(items))(*items)
    ok(L().lib.capmi_colsum_batch_args(arr, len(items), L().stream_ptr()), 'colsum_batch_args')
    check_batch('colsum_batch_args', outs, refs)


def test_colsum_batch_args_rejects_nine_items_and_a_null_input(dev):
    x, o = torch.zeros(4, 4, device=dev), torch.zeros(9, 4, device=dev)
    nine = (L().ColsumItem * 9)()
    for k in range(9):
        setattr(nine[k], 'in', ptr(x))
        nine[k].out, nine[k].rows, nine[k].cols, nine[k].ld = ptr(o[k]), 4, 4, 4
    lib = L().lib
    assert lib.capmi_colsum_batch_args(nine, 9, L().stream_ptr()) == L().EINVAL
    assert lib.capmi_colsum_batch_args(nine, 8, L().stream_ptr()) == 0
    setattr(nine[3], 'in', None)
    assert lib.capmi_colsum_batch_args(nine, 8, L().stream_ptr()) == L().EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ capmi_group_rowsum
@pytest.mark.parametrize('i', range(len(R.GROUP_ROWSUM)))
def test_group_rowsum(dev, i):
    c = R.GROUP_ROWSUM[i]
    T, groups, group, cols, pad_rows, pad_floats, off_in, off_out, arm = c
    x = R.group_rowsum_input(c, seed=i)
    x_d = put(dev, x, off_in)
    out = put(dev, torch.full((groups, cols), R.NAN), off_out)
    ok(L().lib.capmi_group_rowsum(ptr(x_d), T, R.group_rowsum_slab(c), groups, group, cols, ptr(out), L().stream_ptr()), 'group_rowsum')
    sums_close('group_rowsum[%s]' % arm, out, R.group_rowsum(x, c))


# ------------------------------------------------------------------------------------------------ capmi_embed_fwd(_pl)
@pytest.mark.parametrize('i', range(len(R.EMBED_FWD)))
def test_embed_fwd(dev, i):
    N, Ed, stride, it_save, relu, mask, planes, arm = R.EMBED_FWD[i]
    it, E, m = R.embed_fwd_inputs(R.EMBED_FWD[i], seed=i)
    m = m if mask else None
    it_d, E_d, m_d = put(dev, it), put(dev, E), put(dev, m)
    x = nan(dev, N, Ed)
    saved = torch.full((N,), -1, dtype=torch.long, device=dev) if it_save else None
    pl = planes_buf(dev, Ed) if planes else None
    lib = L().lib
    if planes:
        rc = lib.capmi_embed_fwd_pl(ptr(it_d), stride, ptr(saved), ptr(E_d), ptr(m_d), ptr(x), N, Ed, int(relu), ptr(pl), L().stream_ptr())
    else:
        rc = lib.capmi_embed_fwd(ptr(it_d), stride, ptr(saved), ptr(E_d), ptr(m_d), ptr(x), N, Ed, int(relu), L().stream_ptr())
    if arm == 'EINVAL':
        assert rc == L().EINVAL
        return
    ok(rc, 'embed_fwd')
    assert same_bits(x, R.embed_fwd(it, E, m, relu))                       # one gather, one max, one float32 multiply
    assert float((x.double().cpu() - R.embed_fwd(it, E.double(), m, relu)).abs().max()) == 0.0      # ... which are exact in float64 too
    if it_save:
        assert torch.equal(saved.cpu(), it[:, 0])
    if planes:
        same_planes(pl, x)


# ------------------------------------------------------------------------------------------------ capmi_embed_bwd
@pytest.fixture(scope='module')
def embed_bwd_refs():
    """float64 scatter-adds of the EMBED_BWD rows, computed once"""
    refs = {}

    def get(i):
        if i not in refs:
            tok, dx, xs, m = R.embed_bwd_inputs(i)
            refs[i] = (tok, dx, xs, m, R.embed_bwd(tok, dx, xs, m, R.EMBED_BWD[i][2]))
        return refs[i]
    return get


def grads_close(name, got, ref):
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), name
    e, bound = float((got - R.FILL - ref).abs().max()), R.EMBED_TOL * max(1.0, float(ref.abs().max()))
    print('%s max|got - fill - ref| %.2e (bound %.2e)' % (name, e, bound))
    assert e <= bound, (name, e, bound)


@pytest.mark.parametrize('i', range(len(R.EMBED_BWD)))
def test_embed_bwd(dev, embed_bwd_refs, i):
    """rows 12 273 and 14 336 ask for more than 64 KB of dynamic LDS (72 KB at 14 336): both deterministic kernels opt in to it once,
    so a 128-image batch (13 440 positions) keeps the run-to-run identical gradient"""
    rows, Ed, V, relu, mask, off, hot, arm = R.EMBED_BWD[i]
    tok, dx, xs, m, ref = embed_bwd_refs(i)
    tok_d, dx_d, xs_d, m_d = put(dev, tok), put(dev, dx, off == 'dx'), put(dev, xs), put(dev, m)
    outs = []
    for _ in range(2 if arm.startswith('det') else 1):
        dE = put(dev, torch.full((V, Ed), R.FILL), off == 'dE')
        ok(L().lib.capmi_embed_bwd(ptr(tok_d), ptr(dx_d), ptr(xs_d), ptr(m_d), ptr(dE), rows, Ed, relu, L().stream_ptr()), 'embed_bwd')
        torch.cuda.synchronize()
        outs.append(dE.cpu())
    grads_close('embed_bwd[%d: %s]' % (rows, arm), outs[0], ref)
    if len(outs) == 2:
        assert torch.equal(R.bits(outs[0]), R.bits(outs[1])), 'two launches of the deterministic arm differ'


def test_embed_bwd_needs_x_saved_for_relu(dev):
    t = torch.zeros(4, 4, device=dev)
    tok = torch.zeros(4, dtype=torch.long, device=dev)
    assert L().lib.capmi_embed_bwd(ptr(tok), ptr(t), None, None, ptr(t.clone()), 4, 4, 1, L().stream_ptr()) == L().EINVAL


# ------------------------------------------------------------------------------------------------ capmi_embed_pe_fwd / _bwd
@pytest.mark.parametrize('i', range(len(R.EMBED_PE_FWD)))
def test_embed_pe_fwd(dev, i):
    """x = (E[tok] * sqrt(D) + pe) * drop is two or three float32 roundings (the product and the sum may contract to one fused
    multiply-add), each at most 2^-24 of |E| sqrt(D) + |pe| (times drop): every element within 3 * 2^-24 of that magnitude"""
    N, T, D, tok_ld, pos0, drop, arm = R.EMBED_PE_FWD[i]
    tok, E, pe, dr, _ = R.embed_pe_inputs(N, T, D, tok_ld, 5, 700 + i, pos0 + T)
    dr = dr if drop else None
    x = nan(dev, N, T, D)
    keep = [put(dev, t) for t in (tok, E, pe, dr)]
    ok(L().lib.capmi_embed_pe_fwd(ptr(keep[0]), tok_ld, ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(x), N, T, D, pos0, L().stream_ptr()),
       'embed_pe_fwd')
    torch.cuda.synchronize()
    ref, mag = R.embed_pe_fwd(tok, E, pe, dr, T, pos0)
    got = x.double().cpu()
    assert bool(torch.isfinite(got).all())
    over = (got - ref).abs() - 3 * 2.0 ** -24 * mag
    print('embed_pe_fwd[%s] max err / magnitude %.2e (bound %.2e)' % (arm, float(((got - ref).abs() / (mag + 1e-30)).max()), 3 * 2.0 ** -24))
    assert float(over.max()) <= 0.0


@pytest.mark.parametrize('i', range(len(R.EMBED_PE_BWD)))
def test_embed_pe_bwd(dev, i):
    N, T, D, tok_ld, drop, V, arm = R.EMBED_PE_BWD[i]
    tok, _, _, dr, dx = R.embed_pe_inputs(N, T, D, tok_ld, V, 600 + i, 1)
    dr = dr if drop else None
    ref = R.embed_pe_bwd(tok, dx, dr, T, V)
    tok_d, dx_d, dr_d = put(dev, tok), put(dev, dx), put(dev, dr)
    outs = []
    for _ in range(2 if arm.startswith('det') else 1):
        dE = put(dev, torch.full((V, D), R.FILL))
        ok(L().lib.capmi_embed_pe_bwd(ptr(tok_d), tok_ld, ptr(dx_d), ptr(dr_d), ptr(dE), N, T, D, L().stream_ptr()), 'embed_pe_bwd')
        torch.cuda.synchronize()
        outs.append(dE.cpu())
    grads_close('embed_pe_bwd[%d: %s]' % (N * T, arm), outs[0], ref)
    if len(outs) == 2:
        assert torch.equal(R.bits(outs[0]), R.bits(outs[1])), 'two launches of the deterministic arm differ'


# ------------------------------------------------------------------------------------------------ ReLU / dropout Jacobians
@pytest.mark.parametrize('i', range(len(R.RELU_MASK_BWD)))
def test_relu_mask_bwd(dev, i):
    with_y, with_mask, arm = R.RELU_MASK_BWD[i]
    dy, y, mask = R.relu_inputs(R.RELU_COUNT, seed=i)
    y, mask = (y if with_y else None), (mask if with_mask else None)
    dx = nan(dev, R.RELU_COUNT + 1)
    keep = [put(dev, t) for t in (dy, y, mask)]
    ok(L().lib.capmi_relu_mask_bwd(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(dx), R.RELU_COUNT, L().stream_ptr()), 'relu_mask_bwd')
    assert same_bits(dx[:R.RELU_COUNT], R.relu_mask_bwd(dy, y, mask))
    assert bool(torch.isnan(dx[R.RELU_COUNT:]).all())


@pytest.mark.parametrize('i', range(len(R.RELU_SCALE_BWD)))
def test_relu_scale_bwd(dev, i):
    count, off, arm = R.RELU_SCALE_BWD[i]
    scale = float(np.float32(1.0 / 0.7))
    dy, y, _ = R.relu_inputs(count, seed=10 + i)
    dx = nan(dev, count + 4)
    dy_d, y_d = put(dev, dy), put(dev, y, off)
    rc = L().lib.capmi_relu_scale_bwd(ptr(dy_d), ptr(y_d), scale, ptr(dx), count, L().stream_ptr())
    if arm == 'EINVAL':
        assert rc == L().EINVAL
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx).all())
        return
    ok(rc, 'relu_scale_bwd')
    assert same_bits(dx[:count], R.relu_scale_bwd(dy, y, scale))
    assert bool(torch.isnan(dx[count:]).all())


# ------------------------------------------------------------------------------------------------ clip + Adam
def adam_args(s):
    hp = R.ADAM_HP
    return (hp['lr'], hp['b1'], hp['b2'], hp['eps'], s['wd'], s['clip'], s['scale'])


@pytest.mark.parametrize('name', sorted(R.ADAM_SETS))
@pytest.mark.parametrize('i', range(len(R.ADAM)))
def test_adam_step(dev, i, name):
    """3 steps from zero moments against the float64 formula of capmi.h, p, m and v after every step.  Bounds (rel_err): p of the set
    without decay and scale 1e-6 (test_adam_matches_torch); everything else 4 x the error of the float32 torch restatement of the same
    formula on the same inputs, the largest over the counts of R.ADAM (reduce_ref64.adam_f32_error; a single-element case alone would
    measure the luck of one rounding).  Measured float32 errors (p, m, v) and the bounds they give:
      clip   1.344e-07 1.117e-07 1.126e-07 -> 1e-6 (fixed), 4.47e-07, 4.50e-07
      decay  9.533e-08 4.369e-07 1.060e-07 -> 3.81e-07, 1.75e-06, 4.24e-07
      all    1.241e-07 1.452e-07 1.487e-07 -> 4.96e-07, 5.81e-07, 5.95e-07
    The second trip of adam2_kernel's outer loop is not reached at these counts: grid_for caps the launch at 2048 workgroups of 256
    threads, two quads per thread and trip, so it takes more than 4 194 304 floats in each of p, g, m and v.
    test_grid_wrap_gpu.test_adam_wraps runs that trip (and adam_kernel's), with bounds measured on its own inputs."""
    count, arm = R.ADAM[i]
    s = R.ADAM_SETS[name]
    p0, grads = R.adam_inputs(count)
    refs = R.adam64(p0, grads, **s)
    bounds = R.adam_bounds(name)
    p, m, v = put(dev, p0), torch.zeros(count, device=dev), torch.zeros(count, device=dev)
    for t, gr in enumerate(grads, 1):
        g_d = put(dev, gr)
        ok(L().lib.capmi_adam_step(ptr(p), ptr(g_d), ptr(m), ptr(v), count, *adam_args(s), t, L().stream_ptr()), 'adam_step')
        torch.cuda.synchronize()
        assert torch.equal(g_d.cpu(), gr)
        for what, got, ref, bound in zip('pmv', (p, m, v), refs[t - 1], bounds):
            e = R.rel_err(got, ref)
            print('adam[%s, %d: %s] step %d %s rel_err %.2e (bound %.2e)' % (name, count, arm, t, what, e, bound))
            assert bool(torch.isfinite(got).all()) and e < bound, (what, t, e, bound)


def test_adam_step_rejects_a_misaligned_buffer_and_step_zero(dev):
    s = R.ADAM_SETS['clip']
    p0 = torch.randn(8)
    g_d, m, v = put(dev, p0), torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    lib = L().lib
    assert lib.capmi_adam_step(ptr(put(dev, p0, True)), ptr(g_d), ptr(m), ptr(v), 8, *adam_args(s), 1, L().stream_ptr()) == L().EINVAL
    assert lib.capmi_adam_step(ptr(put(dev, p0)), ptr(g_d), ptr(m), ptr(v), 8, *adam_args(s), 0, L().stream_ptr()) == L().EINVAL
    torch.cuda.synchronize()
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0


def read_record(state):
    torch.cuda.synchronize()
    return L().StepState.from_buffer_copy(state.cpu().numpy().tobytes())


@pytest.mark.parametrize('count', [1544, 1003])
def test_adam_step_dyn_equals_adam_step_and_the_step_record(dev, count):
    """capmi_adam_step_dyn reads lr and the bias corrections from a device record that went through capmi_step_set_lr and one
    capmi_step_advance per step: the same bits as capmi_adam_step with the step number, on adam2_kernel (1544) and adam_kernel (1003)"""
    s = R.ADAM_SETS['all']
    hp = R.ADAM_HP
    p0, grads = R.adam_inputs(count)
    lib, st = L().lib, L().stream_ptr()
    assert C.sizeof(L().StepState) == 32
    state = torch.zeros(32, dtype=torch.uint8, device=dev)
    ok(lib.capmi_step_set_lr(ptr(state), hp['lr'], st), 'step_set_lr')
    a = [put(dev, p0), torch.zeros(count, device=dev), torch.zeros(count, device=dev)]
    b = [put(dev, p0), torch.zeros(count, device=dev), torch.zeros(count, device=dev)]
    for t, gr in enumerate(grads, 1):
        g_d = put(dev, gr)
        ok(lib.capmi_step_advance(ptr(state), hp['b1'], hp['b2'], st), 'step_advance')
        ok(lib.capmi_adam_step_dyn(ptr(a[0]), ptr(g_d), ptr(a[1]), ptr(a[2]), count, ptr(state), hp['b1'], hp['b2'], hp['eps'], s['wd'],
                                   s['clip'], s['scale'], st), 'adam_step_dyn')
        ok(lib.capmi_adam_step(ptr(b[0]), ptr(g_d), ptr(b[1]), ptr(b[2]), count, *adam_args(s), t, st), 'adam_step')
        rec, want = read_record(state), R.step_record(t)
        assert (rec.epoch, rec.adam_step) == (want['epoch'], want['adam_step'])
        assert np.float32(rec.lr) == want['lr'] and np.float32(rec.bc1) == want['bc1'] and np.float32(rec.bc2_sqrt) == want['bc2_sqrt'], \
            (t, rec.lr, rec.bc1, rec.bc2_sqrt, want)
        for x, y in zip(a, b):
            assert same_bits(x, y), t
    assert lib.capmi_adam_step_dyn(ptr(a[0]), ptr(g_d), ptr(a[1]), ptr(a[2]), count, None, hp['b1'], hp['b2'], hp['eps'], 0.0, 0.0, 1.0,
                                   st) == L().EINVAL
    assert lib.capmi_step_advance(None, hp['b1'], hp['b2'], st) == L().EINVAL


# ------------------------------------------------------------------------------------------------ capmi_dropout_masks
def test_dropout_masks_tail_quad_and_misaligned_segments(dev):
    """beside test_dropout_masks_one_launch_equals_four_and_eval_rows (aligned segments of whole quads): a segment with count % 4 == 3
    (the last quad leaves the 16-byte store for the bounded scalar one), segments one float past a 16-byte boundary, and a segment
    shorter than a quad -- each the bits of capmi_dropout_mask on the same seed and offset, nothing written past `count`"""
    seed, p = 7654321, 0.5
    lib, st = L().lib, L().stream_ptr()
    assert len(R.DROPOUT_MASKS) <= 4
    descs = (L().MaskDesc * len(R.DROPOUT_MASKS))()
    got, want = [], []
    for k, (count, off, arm) in enumerate(R.DROPOUT_MASKS):
        buf = put(dev, torch.full((count + 1,), R.NAN), off)
        assert (buf.data_ptr() % 16 != 0) == off
        descs[k].mask, descs[k].count, descs[k].offset = ptr(buf), count, k << 40
        descs[k].row_len, descs[k].rows, descs[k].keep_from = 0, 0, -1
        got.append(buf)
        one = nan(dev, count + 1)
        ok(lib.capmi_dropout_mask(ptr(one), count, p, seed, k << 40, st), 'dropout_mask')
        want.append(one)
    ok(lib.capmi_dropout_masks(descs, len(R.DROPOUT_MASKS), p, seed, st), 'dropout_masks')
    for (count, off, arm), a, b in zip(R.DROPOUT_MASKS, got, want):
        assert same_bits(a, b), arm                                        # the NaN guard included
        assert bool(torch.isnan(a[count:]).all()) and set(a[:count].unique().tolist()) <= {0.0, 2.0}
