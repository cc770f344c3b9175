"""The kernels of region_norm.hip (BatchNorm1d over the valid region rows, use_bn) on every arm production can take, against the
float64 truth of region_norm_ref64.py (pinned on the CPU by test_region_norm_arms_host.py), through the ops.bn_* wrappers.

Inputs (region_norm_ref64.inputs): clamp_min(0) of a normal plus, where D >= 5, the hand-made columns 1 (constant 0), 2 (constant 7) and
4 (mean 100, std 0.01); dy a plain normal, not pre-masked; padded rows of x and dy hold NaN, so a padded row read into any sum shows
in every output.  Every tensor handed to a wrapper -- and every [nrb][2][D] partial the wrappers allocate, through ops._bn_partial --
lies inside a larger allocation filled with a sentinel, and everything around it must still hold the sentinel afterwards.

Bounds, none of them new:
* forward (mean, var as 1 / rstd^2 - eps, rstd, y, running buffers): truth_and_bound of test_use_bn_gpu.py -- 4 x the error of ATen's
  CPU float32 F.batch_norm against float64 on the same inputs, floor 1e-6 of the largest element;
* bn_backward (dgamma, dbeta, dx): the same rule, 4 x the error of ATen's CPU float32 autograd of F.batch_norm over the valid rows,
  the same floor (region_norm_ref64.backward_bound);
* bn_linear_bwd: derived, u = 2^-24, per element: dW 8u mag, dgamma (R + 8)u mag, dbeta (R + 2)u mag with the magnitudes of
  region_norm_ref64.linear_bwd.

The cases: the second trip of the grid-stride loops (more than 2048 x 256 quads, both paths, every row compared); mask None; in
place (dx = dy, y = x); a pivot row other than 0 (leading padded rows, leading empty 16-row blocks, an empty block in the middle);
the dword path at a width that is a multiple of 4 (bases one float off; bit-equal to the 16-byte path wherever both compile to the
same arithmetic, see that test); the edges of the 4-column quad, the 256-column tile and the 256-thread block; bn_linear_bwd at R around
its 16-row block; determinism of the backward; the argument sets every entry point refuses before it launches anything.

The mean-100 column in bn_backward: the backward kernels form xhat from the mean rounded to one float, as ATen's float32 backward
does.  Both round the same mean, so the column's error is ATen's and stays inside the bound: the remedy (carrying the (pivot,
offset) pair into the backward kernels) was not needed.  Measured on an MI355X, the worst err / bound of that column over all cases
(each case prints its own line):
  train dgamma  err 3.178e-04  ATen float32 3.164e-04  bound 1.266e-03  (width D=260)
  train dx      err 3.189e-03  ATen float32 3.159e-03  bound 1.264e-02  (in place D=37, masked)
  train dbeta   err 6.617e-06  ATen float32 1.849e-06  bound 7.185e-05  (rows=1056 D=2048)
  eval  dgamma  err 3.323e-05  ATen float32 2.119e-05  bound 8.474e-05  (one float in, D=20)
  eval  dx      err 5.058e-07  ATen float32 4.479e-07  bound 5.705e-06  (width D=258)
Over every column the worst err / bound of any backward case is 0.39 (eval dgamma, the line above); of bn_linear_bwd 0.36 (dW, R=17 D=257, eval).
"""
import pytest
import torch

import region_norm_ref64 as ref
from test_use_bn_gpu import truth_and_bound

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = -24680.5
PAD = 64                        # floats in front of every guarded tensor (256 bytes: the alignment of the allocation is kept)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Guard:
    """device tensors inside sentinel-filled allocations: `off` floats past a 16-byte boundary, PAD floats in front, a row + PAD
    floats behind"""

    def __init__(self):
        self.bufs = []

    def put(self, src, off=0):
        if src is None:
            return None
        n = src.numel()
        lead = PAD + off
        buf = torch.full((lead + n + (src.shape[-1] if src.dim() else 1) + PAD,), SENT, dtype=torch.float32, device=DEV)
        v = buf[lead:lead + n].view(src.shape)
        v.copy_(src)
        assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
        self.bufs.append((buf, lead, n))
        return v

    def new(self, *shape, off=0):
        return self.put(torch.full(shape, SENT), off)

    def check(self):
        torch.cuda.synchronize()
        for buf, lead, n in self.bufs:
            assert bool((buf[:lead] == SENT).all()) and bool((buf[lead + n:] == SENT).all()), 'wrote outside a tensor of %d floats' % n


@pytest.fixture(autouse=True)
def guarded_partials(monkeypatch):
    """the partials the wrappers allocate come out of sentinel-filled allocations too (16-byte aligned, as torch.empty's are)"""
    from imagecaptioning.pytorch_amd import ops
    real, guard = ops._bn_partial, Guard()

    def partial(rows, D, dev, counts=True):
        t, nrb = real(rows, D, dev, counts)
        return guard.put(torch.full((t.numel(),), SENT), 0), nrb

    monkeypatch.setattr(ops, '_bn_partial', partial)
    yield guard
    guard.check()


def ragged(rows, K, seed=1, lens=None):
    """prefix masks of rows / K images with K region slots each (row 0 valid, one image full), [rows] floats"""
    assert rows % K == 0
    B = rows // K
    g = torch.Generator().manual_seed(seed)
    if lens is None:
        lens = [int(v) for v in torch.randint(1, K + 1, (B,), generator=g)]
        lens[B // 2] = K
    mask = torch.zeros(B, K)
    for b, ln in enumerate(lens):
        mask[b, :ln] = 1
    return mask.view(-1)


def running(D, seed=17):
    g = torch.Generator().manual_seed(seed)
    return 0.3 * torch.rand(D, generator=g), 0.5 + torch.rand(D, generator=g)


# ---------------------------------------------------------------------------------------------- the device side
def forward_dev(x, mask, gamma, beta, steps=3, off=0, inplace=False):
    from imagecaptioning.pytorch_amd import ops
    G = Guard()
    rows, D = x.shape
    xd, md = G.put(x, off), G.put(mask, off)
    rm, rv = G.put(torch.zeros(D), off), G.put(torch.ones(D), off)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    for _ in range(steps):
        mean, rstd, count, shift = ops.bn_stats(xd, md, True, rm, rv, nbt)
    dst = xd if inplace else G.new(rows, D, off=off)
    y = ops.bn_apply(xd, md, G.put(shift, off), G.put(rstd, off), G.put(gamma, off), G.put(beta, off), out=dst)
    assert y.data_ptr() == dst.data_ptr()
    G.check()
    return dict(mean=mean, rstd=rstd, count=count, shift=shift, y=y, running_mean=rm, running_var=rv, nbt=nbt)


def backward_dev(dy, x, mask, gamma, train, rm=None, rv=None, off=0, inplace=False, stats=None):
    from imagecaptioning.pytorch_amd import ops
    G = Guard()
    rows, D = x.shape
    xd, dyd, md = G.put(x, off), G.put(dy, off), G.put(mask, off)
    mean, rstd, count, _ = ops.bn_stats(xd, md, train, None if train else G.put(rm, off), None if train else G.put(rv, off))
    if stats is not None:           # the statistics of another launch
        mean, rstd, count = stats
    dg, db = G.new(D, off=off), G.new(D, off=off)
    dst = dyd if inplace else G.new(rows, D, off=off)
    dx = ops.bn_backward(dyd, xd, md, G.put(mean, off), G.put(rstd, off), G.put(gamma, off), G.put(count, off), train, dg, db, dx=dst)
    assert dx.data_ptr() == dst.data_ptr()
    G.check()
    return dict(dgamma=dg, dbeta=db, dx=dx, count=count, stats=(mean, rstd, count))


def check_forward(got, x, mask, gamma, beta, steps, tag):
    rows, D = x.shape
    v = ref.valid_rows(mask, rows)
    t = ref.forward(x, mask, gamma, beta, steps)
    _, bound = truth_and_bound(x, v.float(), gamma, beta, steps)
    assert float(got['count']) == t['count'] == int(v.sum()) and int(got['nbt']) == steps
    y = got['y'].cpu()
    have = dict(mean=got['mean'], var=1 / got['rstd'].double() ** 2 - ref.EPS, rstd=got['rstd'], y=y[v],
                running_mean=got['running_mean'], running_var=got['running_var'])
    want = dict(t, y=t['y'][v])
    worst = {}
    for k in ('mean', 'var', 'rstd', 'y', 'running_mean', 'running_var'):
        worst[k] = float((have[k].double().cpu() - want[k]).abs().max())
        print('bn arms fwd %s %-12s err %.3e bound %.3e' % (tag, k, worst[k], bound[k]))
    for k in worst:
        assert worst[k] <= bound[k], (tag, k, worst[k], bound[k])       # (a NaN fails this comparison too)
    assert not bits(y[~v]).any(), 'padded rows of y must be +0.0'
    # the pair bn_apply subtracts is the mean
    s = got['shift'].double().cpu()
    assert float((s[0] + s[1] - t['mean']).abs().max()) <= bound['mean']


def check_backward(got, dy, x, mask, gamma, beta, train, rm, rv, tag):
    rows, D = x.shape
    v = ref.valid_rows(mask, rows)
    t = ref.backward(dy, x, mask, gamma, beta, train, rm, rv)
    bound = ref.backward_bound(t, dy, x, mask, gamma, beta, train, rm, rv)
    tag = '%s %s' % (tag, 'train' if train else 'eval')
    worst = {}
    a = ref.aten_backward(dy, x, mask, gamma, beta, train, rm, rv)
    for k in ('dgamma', 'dbeta', 'dx'):
        err = (got[k].double().cpu() - t[k]).abs()
        worst[k] = float(err.max())
        print('bn arms bwd %s %-6s err %.3e bound %.3e' % (tag, k, worst[k], bound[k]))
        if D >= 5:
            print('bn arms bwd %s %-6s mean-100 column: err %.3e, ATen float32 %.3e, bound %.3e'
                  % (tag, k, float(err[..., 4].max()), float((a[k].double() - t[k]).abs()[..., 4].max()), bound[k]))
    for k in worst:
        assert worst[k] <= bound[k], (tag, k, worst[k], bound[k])
    assert not bits(got['dx'].cpu()[~v]).any(), 'padded rows of dx must be +0.0'


def all_three(rows, D, mask, tag, seed=0, off=0, steps=3):
    """forward, train backward and eval backward of one shape against float64"""
    x, dy = ref.inputs(rows, D, mask, seed)
    gamma, beta = ref.affine(D)
    rm, rv = running(D)
    check_forward(forward_dev(x, mask, gamma, beta, steps, off), x, mask, gamma, beta, steps, tag)
    for train in (True, False):
        got = backward_dev(dy, x, mask, gamma, train, rm, rv, off)
        if train:
            assert float(got['count']) == int(ref.valid_rows(mask, rows).sum())
        check_backward(got, dy, x, mask, gamma, beta, train, rm, rv, tag)


# ---------------------------------------------------------------------------------------------- 1. the second grid-stride trip
@pytest.mark.parametrize('rows,D,K', [(1040, 2053, 40), (1056, 2048, 48)], ids=['dword-1040x2053', 'vec16-1056x2048'])
def test_second_grid_stride_trip(rows, D, K):
    """bn_apply / bn_bwd_dx launch at most 2048 blocks of 256 threads, a thread per quad: above 524288 quads the loop takes a second
    trip.  Every row is compared."""
    assert rows * ((D + 3) // 4) > 2048 * 256
    all_three(rows, D, ragged(rows, K), 'rows=%d D=%d' % (rows, D), steps=1)


# ---------------------------------------------------------------------------------------------- 2. mask None
@pytest.mark.parametrize('D', [20, 37])
@pytest.mark.parametrize('rows', [2, 17, 65])
def test_mask_none_counts_every_row(rows, D):
    all_three(rows, D, None, 'mask=None rows=%d D=%d' % (rows, D), seed=rows)


# ---------------------------------------------------------------------------------------------- 3. in place
@pytest.mark.parametrize('masked', [True, False], ids=['masked', 'unmasked'])
@pytest.mark.parametrize('D', [20, 37])
def test_in_place_equals_out_of_place_bit_for_bit(D, masked):
    rows = 70
    mask = ragged(rows, 10, seed=2) if masked else None
    v = ref.valid_rows(mask, rows)
    x, dy = ref.inputs(rows, D, mask, seed=4)
    gamma, beta = ref.affine(D)
    rm, rv = running(D)
    a, b = forward_dev(x, mask, gamma, beta), forward_dev(x, mask, gamma, beta, inplace=True)
    assert same_bits(a['y'], b['y']) and not bits(b['y'].cpu()[~v]).any()
    check_forward(b, x, mask, gamma, beta, 3, 'in place D=%d %s' % (D, masked))
    for train in (True, False):
        a, b = backward_dev(dy, x, mask, gamma, train, rm, rv), backward_dev(dy, x, mask, gamma, train, rm, rv, inplace=True)
        for k in ('dgamma', 'dbeta', 'dx'):
            assert same_bits(a[k], b[k]), (k, train)
        assert not bits(b['dx'].cpu()[~v]).any()
        check_backward(b, dy, x, mask, gamma, beta, train, rm, rv, 'in place D=%d %s' % (D, masked))


# ---------------------------------------------------------------------------------------------- 4. a pivot row other than 0
def pivot_mask(kind):
    mask = torch.ones(100)
    mask[93:] = 0
    if kind == 'empty-block-in-the-middle':
        mask[29:50] = 0                 # rows 32..47, the third block, hold no valid row; row 0 is the pivot
    else:
        mask[:int(kind)] = 0            # 5: inside the first block; 16: one empty block; 37: two, the pivot mid-block
        mask[60:66] = 0
    return mask


@pytest.mark.parametrize('D', [20, 37])
@pytest.mark.parametrize('kind', ['5', '16', '37', 'empty-block-in-the-middle'])
def test_pivot_is_the_first_valid_row(kind, D):
    mask = pivot_mask(kind)
    first = int(torch.nonzero(mask)[0])
    assert first == (0 if kind.startswith('empty') else int(kind))
    all_three(100, D, mask, 'pivot=%s D=%d' % (kind, D), seed=7)


# ---------------------------------------------------------------------------------------------- 6. width edges
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 255, 256, 257, 258, 260])
def test_width_edges(D):
    all_three(35, D, ragged(35, 7, seed=3), 'width D=%d' % D, seed=D)


# ---------------------------------------------------------------------------------------------- 7. bn_linear_bwd
def linear_case(R, D, train, seed=0):
    """the float32 inputs of bn_linear_bwd with mean / rstd from a real bn_stats call on the inputs above"""
    from imagecaptioning.pytorch_amd import ops
    rows = 40
    mask = ragged(rows, 8, seed=5)
    v = ref.valid_rows(mask, rows)
    x, _ = ref.inputs(rows, D, mask, seed)
    gamma, beta = ref.affine(D)
    rm, rv = running(D)
    mean, rstd = ops.bn_stats(x.to(DEV), mask.to(DEV), train, None if train else rm.to(DEV), None if train else rv.to(DEV))[:2]
    g = torch.Generator().manual_seed(seed + 100)
    W = torch.randn(R, D, generator=g) / D ** 0.5
    d_pre = torch.randn(int(v.sum()), R, generator=g)
    G0 = (d_pre.double().t() @ x[v].double()).float()         # the weight gradient on the RAW rows, rounded once
    db = d_pre.double().sum(0).float()
    return G0, db, W, mean.cpu(), rstd.cpu(), gamma, beta


def linear_dev(args, off):
    from imagecaptioning.pytorch_amd import ops
    G = Guard()
    R, D = args[2].shape
    dev = [G.put(a, off) for a in args]
    dg, dbt = G.new(D, off=off), G.new(D, off=off)
    partial = ops.bn_linear_bwd(*dev, dg, dbt)
    assert partial.numel() == (R + 15) // 16 * 2 * D
    G.check()
    return dict(dW=dev[0], dgamma=dg, dbeta=dbt)


@pytest.mark.parametrize('D', [3, 20, 37, 257])
@pytest.mark.parametrize('R', [1, 15, 16, 17, 33])
def test_linear_bwd_edges(R, D):
    for train in (True, False):
        args = linear_case(R, D, train, seed=R)
        if train and D >= 5:            # the mean-100 column is in the statistics
            assert abs(float(args[3][4]) - 100) < 0.02 and 50 < float(args[4][4]) < 200
        t = ref.linear_bwd(*args)
        bound = ref.linear_bwd_bound(t, R)
        for off in (0, 1):
            got = linear_dev(args, off)
            for k in ('dW', 'dgamma', 'dbeta'):
                err = (got[k].double().cpu() - t[k]).abs()
                ratio = float((err / bound[k].clamp_min(1e-300)).max())
                print('bn arms linear_bwd R=%d D=%d %s off=%d %-6s err %.3e, largest err / bound %.3f'
                      % (R, D, 'train' if train else 'eval', off, k, float(err.max()), ratio))
                assert bool((err <= bound[k]).all()), (train, off, k, float(err.max()), ratio)


# ---------------------------------------------------------------------------------------------- 5. the dword path at an aligned width
@pytest.mark.parametrize('D', [20, 256])
def test_dword_path_at_an_aligned_width_matches_the_16_byte_path(D):
    """every tensor argument starts one float into its allocation: D % 4 == 0, but the launch must take the dword path.  Both paths
    add the rows of a block, and the blocks, in the same order, and six of the seven kernels compile to the same arithmetic in both
    instantiations: their bits must match those of the 16-byte path.  bn_stats_kernel does not: the source is the same, but under
    -ffp-contract=fast the 16-byte instantiation forms a deviation v - s * inv with one fma (62 v_pk_fma_f32, 64 v_sub_f32 in its
    gfx950 code) where the dword one subtracts the rounded block mean (30 and 128).  The block M2 therefore differs in its last
    bits, and rstd, y and running_var with it (measured on an MI355X; mean, shift, running_mean and count agree bit for bit): those
    three are held to the forward bound against float64 instead, and the backward is compared on the statistics of one launch."""
    rows = 33
    mask = ragged(rows, 11, seed=6)
    x, dy = ref.inputs(rows, D, mask, seed=9)
    gamma, beta = ref.affine(D)
    rm, rv = running(D)
    a, b = forward_dev(x, mask, gamma, beta), forward_dev(x, mask, gamma, beta, off=1)
    assert a['y'].data_ptr() % 16 == 0 and b['y'].data_ptr() % 16 == 4 and b['running_mean'].data_ptr() % 16 == 4
    for k in ('mean', 'count', 'shift', 'running_mean'):
        assert same_bits(a[k], b[k]), k
    check_forward(b, x, mask, gamma, beta, 3, 'one float in D=%d' % D)          # rstd, y, running_var: see above
    for train in (True, False):
        a = backward_dev(dy, x, mask, gamma, train, rm, rv)
        b = backward_dev(dy, x, mask, gamma, train, rm, rv, off=1, stats=a['stats'])
        assert a['dx'].data_ptr() % 16 == 0 and b['dx'].data_ptr() % 16 == 4 and b['dgamma'].data_ptr() % 16 == 4
        for k in ('dgamma', 'dbeta', 'dx'):
            assert same_bits(a[k], b[k]), (k, train)
        check_backward(b, dy, x, mask, gamma, beta, train, rm, rv, 'one float in D=%d' % D)
        args = linear_case(17, D, train)
        a, b = linear_dev(args, 0), linear_dev(args, 1)
        assert a['dW'].data_ptr() % 16 == 0 and b['dW'].data_ptr() % 16 == 4
        for k in ('dW', 'dgamma', 'dbeta'):
            assert same_bits(a[k], b[k]), (k, train)


# ---------------------------------------------------------------------------------------------- 8. determinism
@pytest.mark.parametrize('D', [37, 256])
def test_backward_twice_gives_the_same_bits(D):
    rows = 70
    mask = ragged(rows, 10, seed=8)
    x, dy = ref.inputs(rows, D, mask, seed=12)
    gamma, _ = ref.affine(D)
    rm, rv = running(D)
    for train in (True, False):
        a, b = backward_dev(dy, x, mask, gamma, train, rm, rv), backward_dev(dy, x, mask, gamma, train, rm, rv)
        for k in ('dgamma', 'dbeta', 'dx'):
            assert same_bits(a[k], b[k]), (k, train)
        args = linear_case(33, D, train)
        a, b = linear_dev(args, 0), linear_dev(args, 0)
        for k in ('dW', 'dgamma', 'dbeta'):
            assert same_bits(a[k], b[k]), (k, train)


# ---------------------------------------------------------------------------------------------- 9. refusals
ROWS, WID = 5, 8        # the shape of the valid call every refused one is a variation of


def entry_points():
    """name -> (argument names in order, the pointer arguments a call may not leave NULL, further refused variations, outputs)"""
    P = lambda *n: n        # noqa: E731
    return {
        'capmi_bn_stats': (P('x', 'mask', 'rows', 'D', 'partial'), P('x', 'partial'), [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3)],
                           P('partial')),
        'capmi_bn_finalize': (P('partial', 'x', 'mask', 'rows', 'D', 'train', 'eps', 'momentum', 'running_mean', 'running_var', 'nbt', 'mean',
                                'rstd', 'count', 'shift'), P('partial', 'x', 'mean', 'rstd', 'shift'),
                              [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3), dict(train=0, running_mean=None),
                               dict(train=0, running_var=None), 'nbt+4'], P('running_mean', 'running_var', 'mean', 'rstd', 'count', 'shift')),
        'capmi_bn_apply': (P('x', 'mask', 'shift', 'rstd', 'gamma', 'beta', 'y', 'rows', 'D'), P('x', 'shift', 'rstd', 'gamma', 'beta', 'y'),
                           [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3)], P('y')),
        'capmi_bn_bwd_partial': (P('dy', 'x', 'mask', 'mean', 'rstd', 'rows', 'D', 'partial'), P('dy', 'x', 'mean', 'rstd', 'partial'),
                                 [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3)], P('partial')),
        'capmi_bn_colsum_parts': (P('partial', 'nparts', 'D', 'dgamma', 'dbeta'), P('partial'),
                                  [dict(nparts=0), dict(nparts=-1), dict(D=0), dict(D=-3)], P('dgamma', 'dbeta')),
        'capmi_bn_bwd_dx': (P('dy', 'x', 'mask', 'mean', 'rstd', 'gamma', 'dgamma', 'dbeta', 'count', 'train', 'dx', 'rows', 'D'),
                            P('dy', 'x', 'mean', 'rstd', 'gamma', 'dx', 'dgamma', 'dbeta', 'count'),
                            [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3)], P('dx')),
        'capmi_bn_linear_bwd': (P('G', 'db', 'W', 'mean', 'rstd', 'gamma', 'beta', 'rows', 'D', 'partial'),
                                P('G', 'db', 'W', 'mean', 'rstd', 'gamma', 'beta', 'partial'),
                                [dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-3)], P('G', 'partial')),
    }


@pytest.mark.parametrize('name', sorted(entry_points()))
def test_invalid_arguments_are_einval_and_write_nothing(name):
    """a NULL for each required pointer, rows / D <= 0, each float pointer 2 bytes off, num_batches_tracked 4 bytes off: EINVAL
    before anything is launched (region_norm.hip checks all of these ahead of its first launch), the outputs keep the sentinel;
    the call they are variations of is valid"""
    from imagecaptioning.pytorch_amd import _lib
    order, required, more, outputs = entry_points()[name]
    nrb = (ROWS + 15) // 16
    f = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=DEV)       # noqa: E731
    one = lambda *s: torch.ones(s, dtype=torch.float32, device=DEV)           # noqa: E731
    T = dict(x=one(ROWS, WID), dy=one(ROWS, WID), W=one(ROWS, WID), G=f(ROWS, WID), y=f(ROWS, WID), dx=f(ROWS, WID), mask=one(ROWS),
             db=one(ROWS), partial=f(nrb * (2 * WID + 1)), running_mean=f(WID), running_var=f(WID), mean=one(WID), rstd=one(WID),
             gamma=one(WID) / 2, beta=one(WID), shift=one(2, WID), dgamma=one(WID), dbeta=one(WID), count=one(1),
             nbt=torch.full((2,), 77, dtype=torch.long, device=DEV))
    if name in ('capmi_bn_finalize', 'capmi_bn_colsum_parts'):
        for k in ('mean', 'rstd', 'shift', 'count', 'dgamma', 'dbeta'):       # outputs of these two
            T[k].fill_(SENT)
    if name in ('capmi_bn_finalize', 'capmi_bn_colsum_parts'):
        T['partial'] = one(nrb * (2 * WID + 1))                               # and an input
        T['partial'][nrb * 2 * WID:] = ROWS                                   # (the valid-row count of each row block)
    good = dict({k: v.data_ptr() for k, v in T.items()}, rows=ROWS, D=WID, train=1, eps=1e-5, momentum=0.1, nparts=nrb)
    pointers = [k for k in order if k in T and k != 'nbt']
    bad = [{k: None} for k in required] + [{k: good[k] + 2} for k in pointers]
    for m in more:
        bad.append({'nbt': good['nbt'] + 4} if m == 'nbt+4' else m)
    fn = getattr(_lib.lib, name)
    call = lambda **kw: fn(*[dict(good, **kw)[k] for k in order], _lib.stream_ptr())       # noqa: E731
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, (name, kw)
    torch.cuda.synchronize()
    for k in outputs:
        assert bool((T[k] == SENT).all()), (name, k)
    assert bool((T['nbt'] == 77).all())
    assert call() == 0, name
    torch.cuda.synchronize()
    for k in outputs:
        assert not bool((T[k] == SENT).all()), (name, k)
