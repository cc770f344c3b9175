"""Tensor-level wrappers over the C ABI (include/capmi.h).  Pure plumbing: they check devices/dtypes,
pass ``data_ptr()``s and the current HIP stream, and raise on any non-zero return.  No compute happens
in Python and nothing here falls back to torch ops.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import lib, ptr, check, stream_ptr

_f32 = torch.float32


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.CapmiError('capmi ops need device tensors (got %s)' % t.device)
        if not t.is_contiguous():
            raise _lib.CapmiError('capmi ops need contiguous tensors')


class Workspace:
    """Split-K scratch shared by the GEMM launches of one stream."""

    COUNTER_FLOATS = 16384      # CAPMI_WS_COUNTER_FLOATS: tile tickets live in front of the slabs, zero-initialised

    def __init__(self, device, floats=16 * 1024 * 1024):
        self.buf = torch.zeros(floats + self.COUNTER_FLOATS, dtype=_f32, device=device)

    @property
    def slabs(self):
        return self.buf[self.COUNTER_FLOATS:]

    @property
    def capacity(self):
        return self.buf.numel()


_default_ws = {}


def default_workspace(device):
    key = str(device)
    if key not in _default_ws:
        _default_ws[key] = Workspace(device)
    return _default_ws[key]


def gemm(segs, M, N, out, ldc=None, a_layout=0, b_layout=0, bias=None, bias2=None, row_bias=None, row_bias_div=1,
         mul_mask=None, relu=False, accumulate=False, ws=None, splits=0, defer_reduce=False, a_planes=None, addend=None, stream=None,
         allow_wide=False, b_cols=None, desc_only=False):
    """segs: list of (A, lda, B, ldb, K, a_row_div) with tensors (or (tensor, element_offset) pairs).
    b_cols: optional list of up to 3 (B, ldb, ncol) column segments of a [K][N] B that stay where they are (capmi_gemm_desc.n_bcol;
    one K segment with A planes, M <= 64); the segment's own B may then be None.
    a_planes: optional list (one uint8 tensor per segment, see planes_from_f32) -- the activations also delivered pre-split,
    staged by LDS-DMA in the M <= 64 decode kernel.
    addend: out = addend + epilogue(...) (a residual stream added without copying it into `out` first; row pitch ldc).
    Returns splits_used; desc_only: nothing is called, returns the filled capmi_gemm_desc (what gemm_plan takes)."""
    d = _lib.GemmDesc()
    d.nseg = len(segs)
    if a_planes is not None:
        assert len(a_planes) == len(segs)
        for i, t in enumerate(a_planes):
            d.a_planes[i] = t.data_ptr()
    for i, (A, lda, B, ldb, K, div) in enumerate(segs):
        d.seg[i].A = None if A is None else _addr(A)
        d.seg[i].B = None if B is None else _addr(B)
        d.seg[i].lda, d.seg[i].ldb, d.seg[i].K, d.seg[i].a_row_div = lda, ldb, K, div
    d.a_layout, d.b_layout, d.M, d.N = a_layout, b_layout, M, N
    d.C = _addr(out)
    d.ldc = N if ldc is None else ldc
    d.bias, d.bias2, d.row_bias = ptr(bias), ptr(bias2), ptr(row_bias)
    d.row_bias_div = row_bias_div
    d.mul_mask = ptr(mul_mask)
    d.relu, d.accumulate = int(relu), int(accumulate or addend is not None)
    d.addend = ptr(addend)
    if ws is None:
        ws = default_workspace(_dev(out))
    d.partial, d.partial_capacity = ws.buf.data_ptr(), ws.capacity
    d.splits, d.defer_reduce = splits, int(defer_reduce)
    d.allow_wide_deferred = int(allow_wide)      # (deferred GEMMs: nothing runs beside this one on another stream)
    if b_cols:
        d.n_bcol = len(b_cols)
        for i, (B, ldb, ncol) in enumerate(b_cols):
            d.bcol_B[i], d.bcol_ldb[i], d.bcol_n[i] = _addr(B), ldb, ncol
    if desc_only:
        return d
    check(lib.capmi_gemm_f32(C.byref(d), stream_ptr() if stream is None else stream), 'capmi_gemm_f32')
    return d.splits_used


def gemm_plan(d):
    """(route, splits, epi) that capmi_gemm_f32 would take for the descriptor d (capmi.h capmi_gemm_plan): nothing is launched and no
    device is needed"""
    route, epi, splits = C.c_char_p(), C.c_char_p(), C.c_int()
    check(lib.capmi_gemm_plan(C.byref(d), C.byref(route), C.byref(splits), C.byref(epi)), 'capmi_gemm_plan')
    return route.value.decode(), splits.value, epi.value.decode()


_zero_planes = {}
_planes_cache = {}


def zero_planes(device, chunks=1):
    """>= `chunks` all-zero chunk images (the planes of an all-zero activation, e.g. the initial LSTM state), allocated once per device."""
    key = str(device)
    t = _zero_planes.get(key)
    if t is None or t.numel() < chunks * 12288:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('zero planes requested for the first time inside a graph capture (warm the function up first)')
        t = _zero_planes[key] = torch.zeros(max(chunks, 4) * 12288, dtype=torch.uint8, device=device)
    return t


_capture_scratch = [0]


class capture_scratch:
    """`with ops.capture_scratch():` around the eager WARM-UP of a function that is about to be captured into a hipGraph
    (graphs.GraphedDecode): scratch requested inside is filed under the key the capture will ask for, so it is allocated and
    zero-filled eagerly -- a torch.zeros recorded INTO a graph would only run when that graph replays, while the buffer is
    cached process-wide."""

    def __enter__(self):
        _capture_scratch[0] += 1

    def __exit__(self, *a):
        _capture_scratch[0] -= 1
        return False


def planes_scratch(device, tag, nbytes):
    """Zero-filled-once scratch for A planes, cached per (device, tag, size, stream): rows >= M / columns >= K of a planes buffer
    are never written, so a buffer keeps its zero padding across the rollouts that reuse it; concurrent streams get their own.
    Graph captures share one slot that their warm-up fills (capture_scratch); allocating while capturing is refused."""
    capturing = torch.cuda.is_current_stream_capturing()
    slot = 'capture' if (capturing or _capture_scratch[0]) else stream_ptr()
    key = (str(device), tag, int(nbytes), slot)
    t = _planes_cache.get(key)
    if t is None:
        if capturing:
            raise RuntimeError('planes scratch %r requested for the first time inside a graph capture: run the function once '
                               'under ops.capture_scratch() before capturing it' % (tag,))
        t = _planes_cache[key] = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
    return t


def planes_from_f32(x, out=None):
    """A planes (capmi.h capmi_planes_from_f32) of a [M <= 64, K] fp32 matrix (row stride = x.stride(0))."""
    M, K = x.shape
    assert x.is_cuda and x.dtype == _f32 and x.stride(1) == 1 and M <= 64
    if out is None:
        out = torch.zeros(int(lib.capmi_planes_bytes(K)), dtype=torch.uint8, device=x.device)
    check(lib.capmi_planes_from_f32(x.data_ptr(), x.stride(0), M, K, out.data_ptr(), stream_ptr()), 'capmi_planes_from_f32')
    return out


def _addr(x):
    if isinstance(x, tuple):
        t, off = x
        return t.data_ptr() + 4 * off
    return x.data_ptr()


def _dev(x):
    return (x[0] if isinstance(x, tuple) else x).device


class _WsView:
    """A region of a SlabArena with the Workspace interface of gemm()."""

    def __init__(self, buf):
        self.buf = buf

    @property
    def capacity(self):
        return self.buf.numel()


class SlabArena:
    """Bump allocator of split-K workspaces whose reduction is deferred: one region ([tickets | slabs]) per GEMM, the
    same offsets step after step.  A deferred GEMM never self-reduces (gemm_f32.hip: self_reduce requires !defer_reduce), so
    the ticket words in front of each region are layout only -- nothing reads them and nothing has to keep them zero."""

    CHUNK = 128 * 1024 * 1024          # floats (512 MB)

    def __init__(self, device):
        self.dev, self.chunks = device, []
        self.cur = self.off = 0

    def reset(self):
        self.cur = self.off = 0

    def take(self, floats):
        assert floats <= self.CHUNK
        if self.off + floats > self.CHUNK:
            self.cur, self.off = self.cur + 1, 0
        if self.cur == len(self.chunks):
            self.chunks.append(torch.zeros(self.CHUNK, dtype=_f32, device=self.dev))
        return self.chunks[self.cur][self.off:self.off + floats]

    def commit(self, floats):
        self.off += (floats + 63) // 64 * 64


_group_cache = {}


def gemm_group_tn(items, ws=None, cache_key=None):
    """capmi_gemm_group_tn: items = [(dy [K,M], x [K,N], out, accumulate[, ldc, out_off[, colsum]])] -- out_i (+)= dy_i^T x_i for all i in
    ONE persistent launch (+ one small reduction launch for the K-sliced tail).  out: [M,N] contiguous, or -- with ldc / out_off -- the
    tensor whose elements out_off + m * ldc + n receive the product (a column block of a wider gradient).  colsum: optional [M]
    tensor that receives the column sums of dy (the bias gradient), taken by the GEMM's staging waves.
    Returns the per-item splits_used.
    cache_key: any hashable; the ctypes table of an identical item list (same pointers, same shapes) is built once."""
    dev = items[0][2].device
    key = tuple((it[0].data_ptr(), it[1].data_ptr(), it[2].data_ptr(), it[0].shape[0], it[0].shape[1], it[1].shape[1], bool(it[3])) + tuple(it[4:6])
                + ((it[6].data_ptr(),) if len(it) > 6 and it[6] is not None else ()) for it in items)
    hit = _group_cache.get(cache_key) if cache_key is not None else None
    if hit is not None and hit[0] == key:
        arr = hit[1]
    else:
        arr = (_lib.GroupGemm * len(items))()
        for g, it in zip(arr, items):
            dy, x, out, acc = it[:4]
            _chk(dy, x, out)
            K, M = dy.shape
            N = x.shape[1]
            ldc = it[4] if len(it) > 4 and it[4] is not None else N
            off = it[5] if len(it) > 5 else 0
            cs = it[6] if len(it) > 6 else None
            if x.shape[0] != K or ldc < N or off + (M - 1) * ldc + N > out.numel() or (cs is not None and (cs.numel() != M or not cs.is_contiguous())):
                raise _lib.CapmiError('gemm_group_tn: shapes %s^T %s -> %s (ldc %d, offset %d)' % (tuple(dy.shape), tuple(x.shape), tuple(out.shape), ldc, off))
            g.A, g.B, g.C, g.lda, g.ldb, g.ldc, g.K, g.M, g.N, g.accumulate = dy.data_ptr(), x.data_ptr(), out.data_ptr() + 4 * off, M, N, ldc, K, M, N, int(bool(acc))
            g.colsum = None if cs is None else cs.data_ptr()
        if cache_key is not None:
            _group_cache[cache_key] = (key, arr)
    if ws is None:
        ws = default_workspace(dev)
    slabs = ws.buf[Workspace.COUNTER_FLOATS:] if isinstance(ws, Workspace) else ws.buf
    check(lib.capmi_gemm_group_tn(arr, len(items), slabs.data_ptr(), slabs.numel(), stream_ptr()), 'capmi_gemm_group_tn')
    return [g.splits_used for g in arr]


_pinned_arena = {'buf': None, 'off': 0}


def reserve_pinned_arena(nbytes=8 << 20):
    """Pinned host memory for the small tables a graph CAPTURE uploads (pinning inside a capture is refused by the runtime): call
    before capturing.  A slot is handed out once and never recycled -- the captured memcpy node re-reads it at every replay."""
    a = _pinned_arena
    if a['buf'] is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the pinned table arena must be reserved before a graph capture starts')
        a['buf'], a['off'] = torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=True), 0
    return a


def upload_bytes(raw, device):
    """host bytes -> uint8 device tensor on the current stream, valid under graph capture"""
    import numpy as np
    n = len(raw)
    if not torch.cuda.is_current_stream_capturing():
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory().to(device, non_blocking=True)
    a = _pinned_arena
    if a['buf'] is None or a['off'] + n > a['buf'].numel():
        raise RuntimeError('pinned table arena missing or full (%d bytes wanted): ops.reserve_pinned_arena() before the capture' % n)
    slot = a['buf'][a['off']:a['off'] + n]
    a['off'] += (n + 63) // 64 * 64
    slot.numpy()[:] = np.frombuffer(raw, dtype=np.uint8)
    t = torch.empty(n, dtype=torch.uint8, device=device)
    check(lib.capmi_upload_async(t.data_ptr(), slot.data_ptr(), n, stream_ptr()), 'capmi_upload_async')
    return t


class DeferredGrads:
    """Parameter gradients of a layer-by-layer backward that nothing reads before the optimizer: the weight-gradient GEMMs
    leave their K-slice slabs in a SlabArena and the bias-gradient column sums are only recorded; batched launches finish them
    (Transformer XE bs64: 98 + 162 launches and 160 zero-fills less per step).
    r4: all of it runs on a SIDE STREAM beside the dX / attention / LayerNorm chain of the backward -- nothing reads these results
    before flush(), and every kernel of the chain leaves CUs idle at its tail (212 or 636 tiles of a d_model-wide GEMM on 256 CUs)
    or altogether (MHA, LayerNorm, masks).  The GEMMs follow their operands by an event; the reductions and column sums go out in
    batches of SIDE_BATCH items behind them instead of as two launches at the very end of the backward.  Transformer XE 15.3 ->
    14.3 ms per step with the GEMMs alone (A/B inside one gpurun call).
    r6: superseded as the default by the grouped launch (see __init__); CAPMI_DW_STREAM=1 opts back in."""

    _arenas = {}
    uploads = 0
    SIDE_BATCH = 64            # (batches of 12 vs one flush at the end: 14.37 vs 14.44 ms per Transformer XE step -- and 46 more launches; 64: +6)

    def __init__(self, device):
        self.dev = device
        key = str(device)
        if key not in self._arenas:
            self._arenas[key] = {'arena': SlabArena(device), 'tables': {}}
        self.state = self._arenas[key]
        self.arena = self.state['arena']
        self.arena.reset()
        self.red, self.col, self.keep = [], [], []
        self.red_side, self.col_side, self.side_batches, self.synced = [], [], 0, None
        self.side = None
        # r5: the side stream was worth 2-5 % of the Transformer step beside one launch + deferred reduction per GEMM (profiles/
        # r05_fat_gemm_wide.md section 7).  r6: the GROUPED launch at flush() beats it in both issue modes (stepped 20.81 vs 20.98 ms,
        # captured 20.70 vs 22.78 / 23.24 with the side stream forked into the capture; gpurun_out/r6d, r6e) -- the side stream is
        # opt-in now (CAPMI_DW_STREAM=1; inside a graph capture additionally CAPMI_DW_STREAM_CAPTURE=1), and the stepped and the
        # captured step issue exactly the same launches
        if os.environ.get('CAPMI_DW_STREAM', '0') == '1' and torch.cuda.is_available() and \
                (not torch.cuda.is_current_stream_capturing() or os.environ.get('CAPMI_DW_STREAM_CAPTURE', '0') == '1'):
            if 'side' not in self.state:
                self.state['side'] = torch.cuda.Stream(device=device)
                self.state['events'] = []
            self.side, self.ev_pool, self.ev_used = self.state['side'], self.state['events'], 0
        # nothing runs beside the deferred GEMMs when there is no side stream: the planner may give them 256 x 128 tiles too -- said
        # per call (capmi_gemm_desc.allow_wide_deferred; a process-wide switch could be left stuck by two live instances: ADVICE r5)
        # r6: without a side stream the weight-gradient GEMMs are only RECORDED and go out at flush() as one grouped persistent launch
        # (capmi_gemm_group_tn); CAPMI_DW_GROUP=0 keeps one launch + deferred reduction per GEMM
        self.group = [] if (self.side is None and os.environ.get('CAPMI_DW_GROUP', '1') != '0') else None

    def _side_follows_main(self):
        """the side stream waits for everything enqueued on the current stream so far"""
        if self.ev_used == len(self.ev_pool):
            self.ev_pool.append(torch.cuda.Event())
        ev = self.ev_pool[self.ev_used]
        self.ev_used += 1
        ev.record()
        self.side.wait_event(ev)

    def dw(self, dy, x, out, final=True, ldc=None, out_off=0, accumulate=False, colsum_out=None):
        """out[M,N] (+)= dy[K,M]^T x[K,N], reduction deferred.  out: contiguous [M,N], or with ldc / out_off a column block of a wider
        gradient (elements out_off + m * ldc + n).  final: nobody writes `dy` after this call (a running gradient accumulator that the
        caller keeps adding to must be read in stream order: no side stream, no grouping).  accumulate: the caller has ALREADY
        written the addend into `out` (in stream order).  colsum_out: the bias gradient (column sums of dy) that goes with this weight
        gradient -- in a grouped launch the GEMM's staging waves take it from the operand they stage (no second pass over dy)."""
        _chk(dy, x, out)
        K, M = dy.shape
        N = x.shape[1]
        ldc = N if ldc is None else ldc
        cf = Workspace.COUNTER_FLOATS
        if self.group is not None and final:
            fold = colsum_out is not None and os.environ.get('CAPMI_GROUP_COLSUM', '1') != '0'
            self.group.append((dy, x, out, accumulate, ldc, out_off, colsum_out if fold else None))
            if colsum_out is not None and not fold:
                self.colsum(dy, colsum_out)
            return
        if colsum_out is not None:
            if final:
                self.colsum(dy, colsum_out)
            else:
                colsum(dy, out=colsum_out)
        if cf + 2 * M * N > SlabArena.CHUNK:            # a gradient this large needs no K split to fill the chip
            gemm([(dy, M, x, N, K, 1)], M, N, (out, out_off), ldc=ldc, a_layout=1, b_layout=1, accumulate=accumulate)
            return
        region = self.arena.take(min(cf + 16 * M * N, SlabArena.CHUNK))      # (the GEMM limits its K split to the region)
        on_side = self.side is not None and final
        if on_side:
            self._side_follows_main()         # dy and x are complete on the main stream here
            self.synced = dy
            self.keep.extend((dy, x))
        splits = gemm([(dy, M, x, N, K, 1)], M, N, out, a_layout=1, b_layout=1, ws=_WsView(region), defer_reduce=True,
                      stream=self.side.cuda_stream if on_side else None, allow_wide=self.side is None)
        self.arena.commit(cf + splits * M * N)
        (self.red_side if on_side else self.red).append((region.data_ptr() + 4 * cf, out.data_ptr() + 4 * out_off, 0, splits, M, N, ldc,
                                                         int(bool(accumulate)), 0))
        if on_side:
            self._flush_side()

    def colsum(self, dy, out):
        """out[cols] = column sums of dy, which nobody writes any more"""
        _chk(dy, out)
        assert dy.is_contiguous()
        row = (dy.data_ptr(), out.data_ptr(), 0, dy.shape[0], dy.shape[1], dy.shape[1], 0)
        self.keep.append(dy)               # read when its batch goes out
        if self.side is None:
            self.col.append(row)
            return
        if self.synced is not dy:
            self._side_follows_main()
            self.synced = dy
        self.col_side.append(row)
        self._flush_side()

    def _table(self, name, rows, fmt):
        """device copy of an item table; (tensor, True when it was uploaded just now -- on the CURRENT stream)"""
        import struct
        key = tuple(rows)
        cached = self.state['tables'].get(name)
        if cached is not None and cached[0] == key:
            return cached[1], False
        raw = b''.join(struct.pack(fmt, *r) for r in rows)
        DeferredGrads.uploads += 1          # (diagnostic: tables re-uploaded because the item list changed)
        t = upload_bytes(raw, self.dev)
        self.state['tables'][name] = (key, t)
        return t, True

    def _flush_side(self, force=False):
        if len(self.red_side) + len(self.col_side) < (1 if force else self.SIDE_BATCH):
            return
        st = self.side.cuda_stream
        for kind, rows, fmt, fn in (('red', self.red_side, '<QQQiiiiii', lib.capmi_splitk_reduce_batch),
                                    ('col', self.col_side, '<QQQiiii', lib.capmi_colsum_batch)):
            if rows:
                t, uploaded = self._table('%s_side%d' % (kind, self.side_batches), rows, fmt)
                if uploaded:
                    self._side_follows_main()         # the table's copy was enqueued on the main stream
                check(fn(t.data_ptr(), len(rows), st), 'capmi_%s_batch (side stream)' % kind)
        self.red_side, self.col_side = [], []
        self.side_batches += 1

    def flush(self):
        if self.side is not None and self.ev_used:
            self._flush_side(force=True)
            torch.cuda.current_stream().wait_stream(self.side)
        if self.group:
            gemm_group_tn(self.group, cache_key=('deferred', str(self.dev)))
            self.group = []
        if self.red:
            t, _ = self._table('red', self.red, '<QQQiiiiii')
            check(lib.capmi_splitk_reduce_batch(t.data_ptr(), len(self.red), stream_ptr()), 'capmi_splitk_reduce_batch')
        if self.col:
            t, _ = self._table('col', self.col, '<QQQiiii')
            check(lib.capmi_colsum_batch(t.data_ptr(), len(self.col), stream_ptr()), 'capmi_colsum_batch')
        self.red, self.col, self.keep = [], [], []

    def abandon(self):
        """the backward raised: nothing is finished, but GEMMs already enqueued on the side stream may still be reading the dy / x
        tensors in `keep`.  The main stream must wait for them before those blocks return to the caching allocator (a caller
        that catches the error -- an OOM retry -- would otherwise be handed memory a side-stream kernel still reads)."""
        if self.side is not None and self.ev_used:
            torch.cuda.current_stream().wait_stream(self.side)
        self.red, self.col, self.keep = [], [], []
        self.red_side, self.col_side = [], []
        if self.group is not None:
            self.group = []


def linear(x, weight, bias=None, relu=False, mul_mask=None, row_div=1, rows=None, ws=None, out=None):
    """y = act(x @ weight.T + bias) (* mask); x [M0,K] read as row r -> r // row_div.  out: optional [M,N] contiguous target."""
    _chk(x, weight, bias, mul_mask, out)
    M = x.shape[0] * row_div if rows is None else rows
    N, K = weight.shape
    if out is None:
        out = torch.empty(M, N, dtype=_f32, device=x.device)
    gemm([(x, x.shape[1], weight, K, K, row_div)], M, N, out, bias=bias, relu=relu, mul_mask=mul_mask, ws=ws)
    return out


def matmul_nn(a, b, out=None, ws=None):
    """a [M,K] @ b [K,N]"""
    _chk(a, b)
    M, K = a.shape
    N = b.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=_f32, device=a.device)
    gemm([(a, K, b, N, K, 1)], M, N, out, a_layout=0, b_layout=1, ws=ws)
    return out


def matmul_tn(a, b, out=None, ws=None):
    """a [K,M]^T @ b [K,N]  (weight gradients dW = dY^T X)"""
    _chk(a, b)
    K, M = a.shape
    N = b.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=_f32, device=a.device)
    gemm([(a, M, b, N, K, 1)], M, N, out, a_layout=1, b_layout=1, ws=ws)
    return out


def attention_fwd(att_h, p_att, att, mask, w, b, n, row_img=None):
    _chk(att_h, p_att, att, mask, w, b)
    B, K, A = p_att.shape
    R = att.shape[2]
    N = att_h.shape[0]
    assert row_img is not None or N == B * n
    ctx = torch.empty(N, R, dtype=_f32, device=att.device)
    alpha = torch.empty(N, K, dtype=_f32, device=att.device)
    check(lib.capmi_attention_fwd(ptr(att_h), ptr(p_att), ptr(att), ptr(mask), ptr(w), ptr(b), ptr(ctx), ptr(alpha),
                                  B, n, K, A, R, ptr(row_img), N, stream_ptr()), 'capmi_attention_fwd')
    return ctx, alpha


def attention_bwd(d_ctx, att_h, alpha, p_att, att, mask, w, n, row_img=None):
    _chk(d_ctx, att_h, alpha, p_att, att, mask, w)
    B, K, A = p_att.shape
    R = att.shape[2]
    N = att_h.shape[0]
    d_att_h = torch.empty(N, A, dtype=_f32, device=att.device)
    d_e = torch.empty(N, K, dtype=_f32, device=att.device)
    check(lib.capmi_attention_bwd(ptr(d_ctx), d_ctx.shape[1], ptr(att_h), ptr(alpha), ptr(p_att), ptr(att), ptr(mask),
                                  ptr(w), ptr(d_att_h), ptr(d_e), B, n, K, A, R, ptr(row_img), N, stream_ptr()),
          'capmi_attention_bwd')
    return d_att_h, d_e


def attention_bwd_batched(d_ctx_all, att_h_all, alpha_all, d_e_all, p_att, w, n, R):
    _chk(d_ctx_all, att_h_all, alpha_all, d_e_all, p_att, w)
    T = att_h_all.shape[0]
    B, K, A = p_att.shape
    dev = p_att.device
    d_att = torch.empty(B, K, R, dtype=_f32, device=dev)
    d_p_att = torch.empty(B, K, A, dtype=_f32, device=dev)
    d_w = torch.empty(A, dtype=_f32, device=dev)
    d_b = torch.empty(1, dtype=_f32, device=dev)
    check(lib.capmi_attention_bwd_batched(ptr(d_ctx_all), d_ctx_all.shape[-1], ptr(att_h_all), ptr(alpha_all),
                                          ptr(d_e_all), ptr(p_att), ptr(w), ptr(d_att), ptr(d_p_att), ptr(d_w), ptr(d_b),
                                          T, B, n, att_h_all.shape[1], K, A, R, stream_ptr()), 'capmi_attention_bwd_batched')
    return d_att, d_p_att, d_w, d_b


def lstm_cell_fwd(partial, splits, b_ih, b_hh, c_prev, row_bias=None, row_bias_div=1, out_mask=None, want_drop=False):
    N, R = c_prev.shape
    dev = c_prev.device
    h = torch.empty(N, R, dtype=_f32, device=dev)
    c = torch.empty(N, R, dtype=_f32, device=dev)
    gates = torch.empty(N, 4 * R, dtype=_f32, device=dev)
    h_drop = torch.empty(N, R, dtype=_f32, device=dev) if (want_drop or out_mask is not None) else None
    check(lib.capmi_lstm_cell_fwd(ptr(partial), splits, ptr(b_ih), ptr(b_hh), ptr(row_bias), row_bias_div, None, ptr(c_prev),
                                  ptr(h), ptr(c), ptr(gates), ptr(out_mask), ptr(h_drop), N, R, stream_ptr()),
          'capmi_lstm_cell_fwd')
    return h, c, gates, h_drop


def lstm_cell_bwd(dh, dc_next, gates, c_prev, c_new, dh_mask=None, dh_b=None, dh_c=None):
    N, R = c_prev.shape
    dev = c_prev.device
    dg = torch.empty(N, 4 * R, dtype=_f32, device=dev)
    dc_prev = torch.empty(N, R, dtype=_f32, device=dev)
    check(lib.capmi_lstm_cell_bwd(ptr(dh), R, ptr(dh_mask), ptr(dh_b), R, ptr(dh_c), R, ptr(dc_next), ptr(gates),
                                  ptr(c_prev), ptr(c_new), ptr(dg), ptr(dc_prev), N, R, stream_ptr()),
          'capmi_lstm_cell_bwd')
    return dg, dc_prev


def embed_fwd(it, E, mask=None, relu=True):
    N = it.shape[0]
    x = torch.empty(N, E.shape[1], dtype=_f32, device=E.device)
    check(lib.capmi_embed_fwd(ptr(it), 1, None, ptr(E), ptr(mask), ptr(x), N, E.shape[1], int(relu), stream_ptr()),
          'capmi_embed_fwd')
    return x


def _keep_scale(p):
    """1 / (1 - p) rounded as the mask kernels round it (float32 throughout)"""
    import numpy as np
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout_mask(shape, p, seed, offset, device):
    m = torch.empty(shape, dtype=_f32, device=device)
    check(lib.capmi_dropout_mask(ptr(m), m.numel(), float(p), int(seed), int(offset), stream_ptr()), 'capmi_dropout_mask')
    m._capmi_scale = (_keep_scale(p), m._version)       # (scale, tensor version: an in-place edit by a caller voids it)
    return m


def dropout_masks(specs, p, seed):
    """All dropout masks of a rollout in one launch.  specs: list of (shape, philox_offset, keep_from) with keep_from = None or
    the first row index (of the second-to-last dimension) that stays in eval mode (mask 1.0).  Returns the mask tensors."""
    dev = specs[0][3] if len(specs[0]) > 3 else None
    descs = (_lib.MaskDesc * len(specs))()
    outs = []
    for i, sp in enumerate(specs):
        shape, offset, keep_from = sp[0], sp[1], sp[2]
        m = torch.empty(shape, dtype=_f32, device=sp[3])
        if sp[2] is None:                       # (eval-mode rows hold 1.0: not a pure keep-scale mask)
            m._capmi_scale = (_keep_scale(p), m._version)
        outs.append(m)
        descs[i].mask, descs[i].count, descs[i].offset = m.data_ptr(), m.numel(), int(offset)
        descs[i].row_len = int(shape[-1])
        descs[i].rows = int(shape[-2]) if len(shape) >= 2 else 1
        descs[i].keep_from = -1 if keep_from is None else int(keep_from)
    check(lib.capmi_dropout_masks(descs, len(specs), float(p), int(seed), stream_ptr()), 'capmi_dropout_masks')
    return outs


def reward_criterion(sel, seq, reward, n_used, per_row=False):
    """capmi_reward_criterion: sel [N_all, L] f32, seq [N_all, L] int64 (rows 0..n_used-1 are scored), reward [n_used] or
    [n_used, L] f32.  Returns (loss [1] or [n_used], gcoef [N_all, L])."""
    _chk(sel, seq)
    if not (reward.is_cuda and reward.dtype == _f32):
        raise _lib.CapmiError('reward must be a float32 device tensor')
    N_all, L = sel.shape
    loss = torch.empty(n_used if per_row else 1, dtype=_f32, device=sel.device)
    gcoef = torch.empty(N_all, L, dtype=_f32, device=sel.device)
    rs, cs = (reward.stride(0), reward.stride(1)) if reward.ndim == 2 else (reward.stride(0), 0)
    check(lib.capmi_reward_criterion(ptr(sel), sel.stride(0), ptr(seq), seq.stride(0), ptr(reward), rs, cs, int(n_used), N_all, L,
                                     int(per_row), ptr(loss), ptr(gcoef), stream_ptr()), 'capmi_reward_criterion')
    return loss, gcoef


def colsum(x, out=None, accumulate=False):
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, dtype=_f32, device=x.device)
    check(lib.capmi_colsum(ptr(x), rows, cols, cols, ptr(out), int(accumulate), stream_ptr()), 'capmi_colsum')
    return out


def relu_mask_bwd(dy, y_ref, mask):
    """dx = dy * mask * (y_ref > 0).  When y_ref is the output AFTER the mask and the mask came from dropout_mask(s) (it carries its
    keep-scale 1 / (1 - p) as `_capmi_scale`), the mask is not read at all: y_ref > 0 says where it kept the element."""
    dx = torch.empty_like(dy)
    tag = getattr(mask, '_capmi_scale', None) if (mask is not None and y_ref is not None) else None
    # (trusted only while nobody has written the mask in place since the mask kernel made it: tests inject masks with copy_)
    scale = tag[0] if (tag is not None and tag[1] == mask._version) else None
    if scale is not None and dy.numel() % 4 == 0 and (dy.data_ptr() | y_ref.data_ptr() | dx.data_ptr()) % 16 == 0 \
            and os.environ.get('CAPMI_RELU_SCALE', '1') != '0':
        check(lib.capmi_relu_scale_bwd(ptr(dy), ptr(y_ref), float(scale), ptr(dx), dy.numel(), stream_ptr()), 'capmi_relu_scale_bwd')
        return dx
    check(lib.capmi_relu_mask_bwd(ptr(dy), ptr(y_ref), ptr(mask), ptr(dx), dy.numel(), stream_ptr()), 'capmi_relu_mask_bwd')
    return dx


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, clip, grad_scale, step):
    check(lib.capmi_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, clip,
                              grad_scale, step, stream_ptr()), 'capmi_adam_step')


class StepState:
    """The per-iteration record of a graph-capturable training step in device memory (capmi.h capmi_step_state): the epoch of the
    random streams, Adam's step count with its bias corrections, the learning rate.  `advance()` is the first launch of every
    iteration (stepped or captured); while `bound()` every dropout / sampling kernel offsets its seed argument by the epoch."""

    def __init__(self, device, adam_step=0, epoch=0, lr=0.0):
        import numpy as np
        self.buf = torch.zeros(32, dtype=torch.uint8, device=device)
        host = _lib.StepState(epoch=int(epoch), adam_step=int(adam_step), lr=float(lr), bc1=1.0, bc2_sqrt=1.0)
        self.buf.copy_(torch.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8).copy()))
        self.lr = float(lr)

    def advance(self, beta1, beta2):
        check(lib.capmi_step_advance(self.buf.data_ptr(), beta1, beta2, stream_ptr()), 'capmi_step_advance')

    def set_lr(self, lr):
        """outside the captured graph; a launch only when the schedule moved the rate (misc.py set_lr)"""
        if float(lr) != self.lr:
            check(lib.capmi_step_set_lr(self.buf.data_ptr(), float(lr), stream_ptr()), 'capmi_step_set_lr')
            self.lr = float(lr)

    def read(self):
        """host copy (a synchronisation: tests / checkpoints only)"""
        return _lib.StepState.from_buffer_copy(bytes(self.buf.cpu().numpy().tobytes()))

    class _Bound:
        def __init__(self, st):
            self.st = st

        def __enter__(self):
            self.prev = C.c_void_p()
            check(lib.capmi_rng_bind_epoch(self.st.buf.data_ptr(), C.byref(self.prev)), 'capmi_rng_bind_epoch')

        def __exit__(self, *a):
            check(lib.capmi_rng_bind_epoch(self.prev.value, None), 'capmi_rng_bind_epoch')
            return False

    def bound(self):
        return StepState._Bound(self)


def adam_step_dyn(p, g, m, v, state, beta1, beta2, eps, weight_decay, clip, grad_scale):
    check(lib.capmi_adam_step_dyn(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), state.buf.data_ptr(), beta1, beta2, eps, weight_decay,
                                  clip, grad_scale, stream_ptr()), 'capmi_adam_step_dyn')


OPTIM_RULES = {'rmsprop': _lib.OPTIM_RMSPROP, 'adagrad': _lib.OPTIM_ADAGRAD, 'sgdm': _lib.OPTIM_SGDM, 'sgdmom': _lib.OPTIM_SGDMOM,
               'adamw': _lib.OPTIM_ADAMW}


def _optim_hp(rule, alpha, beta, eps, weight_decay, clip, grad_scale):
    if rule not in OPTIM_RULES:
        raise _lib.CapmiError('capmi_optim_step has no rule %r (one of %s; Adam is adam_step)' % (rule, sorted(OPTIM_RULES)))
    return _lib.OptimHp(rule=OPTIM_RULES[rule], alpha=alpha, beta=beta, eps=eps, weight_decay=weight_decay, clip=clip,
                        grad_scale=grad_scale)


def optim_step(rule, p, g, s1, s2, lr, alpha, beta, eps, weight_decay, clip, grad_scale, step):
    """fused clip + `rule` ('rmsprop', 'adagrad', 'sgdm', 'sgdmom', 'adamw') on a flat fp32 range; s2: AdamW's second moment, None for
    the one-state rules (capmi.h capmi_optim_step)"""
    hp = _optim_hp(rule, alpha, beta, eps, weight_decay, clip, grad_scale)
    check(lib.capmi_optim_step(C.byref(hp), ptr(p), ptr(g), ptr(s1), ptr(s2), p.numel(), lr, step, stream_ptr()), 'capmi_optim_step')


def optim_step_dyn(rule, p, g, s1, s2, state, alpha, beta, eps, weight_decay, clip, grad_scale):
    """optim_step with the learning rate, the step number and AdamW's bias corrections read from the device record `state`"""
    hp = _optim_hp(rule, alpha, beta, eps, weight_decay, clip, grad_scale)
    check(lib.capmi_optim_step_dyn(C.byref(hp), ptr(p), ptr(g), ptr(s1), ptr(s2), p.numel(), state.buf.data_ptr(), stream_ptr()),
          'capmi_optim_step_dyn')


def ema_step(ema, p, decay, warmup, step):
    """ema = d * ema + (1 - d) * p over a flat fp32 range, d = min(decay, (1 + step) / (10 + step)) with `warmup` else decay.  `step`:
    the 1-based step number (capmi.h capmi_ema_step)"""
    check(lib.capmi_ema_step(ptr(ema), ptr(p), p.numel(), decay, int(bool(warmup)), int(step), stream_ptr()), 'capmi_ema_step')


def ema_step_dyn(ema, p, state, decay, warmup):
    """ema_step with the step number read from the device record `state` (after its advance()): the form a captured step replays"""
    check(lib.capmi_ema_step_dyn(ptr(ema), ptr(p), p.numel(), state.buf.data_ptr(), decay, int(bool(warmup)), stream_ptr()),
          'capmi_ema_step_dyn')


def logsoftmax_bwd(g_dense, sparse, seq_logp, live, dlogits, N, L, T, V1, raw=False):
    """d(logits) [T,N,V1] from the loss gradient w.r.t. the dense log-probs: dense (`g_dense` [N,L,V1]), sparse
    (`sparse`, a _lib.SparseLogpGrad from sparse_logp.split_grad) or both.
    raw: the rollout stored the LOGITS (CAPMI_SELECT_RAW; AttModel._sample(output_logsoftmax=0), AttModel.py:171-175, 265) -- the loss
    gradient IS d(logits) on the live rows, no softmax Jacobian (capmi_sparse_logp_grad.raw)."""
    if raw:
        sp = _lib.SparseLogpGrad() if sparse is None else _lib.SparseLogpGrad.from_buffer_copy(sparse)
        sp.raw = 1
        sparse = sp
    if sparse is not None:
        check(lib.capmi_logsoftmax_bwd_sparse(C.byref(sparse), ptr(g_dense), ptr(seq_logp), ptr(live), ptr(dlogits), N, L, T, V1,
                                              stream_ptr()), 'capmi_logsoftmax_bwd_sparse')
    else:
        check(lib.capmi_logsoftmax_bwd(ptr(g_dense), ptr(seq_logp), ptr(live), ptr(dlogits), N, L, T, V1, stream_ptr()),
              'capmi_logsoftmax_bwd')


def logsoftmax_select(logits, step, L, mode, temperature, gumbel, seed, forced, no_finish_mask, seq, it_next, unfinished,
                      seq_logp, sel_logp, live, top_k=0, top_p=0.0, splits=1, stride=0, bias=None, shape=None, next_embed=None,
                      ss_mode=None):
    """capmi_logsoftmax_select_partial with the optional top-k / nucleus filter; used by the host-stepped decoders
    (Transformer, AoA).  logits: finished [N,V1] (one slab, no bias), or -- with shape=(N,V1) -- the `splits` K-slice slabs a
    deferred logit GEMM left `stride` floats apart, finished here together with `bias`.
    next_embed: dict(E, mask, x, it_save, relu, x_planes) -- the workgroup that chose a row's token also writes the NEXT step's
    input embedding x[r] = relu?(E[token]) * mask[r] (+ its planes) and it_save[r] = token (capmi_next_embed).
    ss_mode: uint8 [N], the kernel's per-row mode override (scheduled sampling, AttModel.py:145-154): 1 = row r draws its token,
    2 = it takes forced[r, step]; the caller passes `forced` advanced by one column and no_finish_mask = 1."""
    N, V1 = logits.shape if shape is None else shape
    if ss_mode is not None:
        if not torch.is_tensor(ss_mode) or ss_mode.dtype != torch.uint8 or tuple(ss_mode.shape) != (N,) or not ss_mode.is_contiguous() \
                or ss_mode.device != seq.device:
            raise _lib.CapmiError('logsoftmax_select: ss_mode must be a contiguous uint8 device tensor of shape (%d,)' % N)
        if forced is None:
            raise _lib.CapmiError('logsoftmax_select: ss_mode needs the forced tokens its mode-2 rows take')
    flt = _lib.SampleFilter(int(top_k), float(top_p))
    ne = None
    if next_embed is not None:
        ne = _lib.NextEmbed(ptr(next_embed['E']), ptr(next_embed.get('mask')), ptr(next_embed['x']), ptr(next_embed.get('it_save')),
                            int(next_embed['E'].shape[1]), int(next_embed.get('relu', 1)), ptr(next_embed.get('x_planes')), None)
    check(lib.capmi_logsoftmax_select_partial(ptr(logits), int(splits), int(stride), ptr(bias), N, V1, step, L, mode, ptr(ss_mode),
                                              float(temperature),
                                              ptr(gumbel), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(forced),
                                              0 if forced is None else forced.stride(0), int(no_finish_mask), ptr(seq), L,
                                              ptr(it_next), ptr(unfinished), ptr(seq_logp), ptr(sel_logp), ptr(live),
                                              None if ne is None else C.byref(ne),
                                              C.byref(flt) if (top_k or top_p) else None, stream_ptr()),
          'capmi_logsoftmax_select_partial')


def caption_stats(seq_logp, seq):
    """(entropy [N], perplexity [N]) of a decode (eval_utils.py:173-174) from its dense log-probs [N, L, V1] and tokens [N, L]: one
    pass over seq_logp, nothing dense is built (capmi_caption_stats)."""
    _chk(seq_logp, seq)
    N, L, V1 = seq_logp.shape
    if seq.dtype != torch.int64 or tuple(seq.shape) != (N, L) or seq_logp.dtype != _f32:
        raise _lib.CapmiError('caption_stats: seq_logp [N,L,V1] float32 and seq [N,L] int64 expected')
    scratch = torch.empty(2 * N * L, dtype=_f32, device=seq_logp.device)
    ent = torch.empty(N, dtype=_f32, device=seq_logp.device)
    ppl = torch.empty(N, dtype=_f32, device=seq_logp.device)
    check(lib.capmi_caption_stats(ptr(seq_logp), ptr(seq), N, L, V1, ptr(scratch), ptr(ent), ptr(ppl), stream_ptr()), 'capmi_caption_stats')
    return ent, ppl


def ensemble_weights(weights, M):
    """AttEnsemble's weights as the kernel takes them: M floats, >= 0, normalised to sum 1 (None: all ones, AttEnsemble.py:25)."""
    if not 1 <= M <= _lib.ENSEMBLE_MAX:
        raise _lib.CapmiError('an ensemble has 1..%d members (got %d)' % (_lib.ENSEMBLE_MAX, M))
    w = [1.0] * M if weights is None else [float(x) for x in (weights.tolist() if torch.is_tensor(weights) else weights)]
    if len(w) != M:
        raise _lib.CapmiError('%d weights for %d members' % (len(w), M))
    if any(not (x >= 0.0) or x == float('inf') for x in w):
        raise _lib.CapmiError('ensemble weights must be finite and >= 0 (got %s)' % w)
    tot = sum(w)
    if not tot > 0.0:
        raise _lib.CapmiError('ensemble weights must have a positive sum (got %s)' % w)
    return [x / tot for x in w]


def ensemble_logprobs(inputs, weights=None, out=None):
    """log( sum_i w_i softmax(inputs[i]) / sum_i w_i ) row-wise (AttEnsemble.get_logprobs_state, AttEnsemble.py:45-53) in one launch
    of capmi_ensemble_logprobs.  inputs: M tensors of one shape [..., V1] (logits or log-probs: each member is normalised),
    float32 device tensors whose rows are contiguous; weights: M numbers >= 0 with a positive sum (normalised here) or None."""
    inputs = list(inputs)
    w = ensemble_weights(weights, len(inputs))
    shape = tuple(inputs[0].shape)
    if len(shape) < 1 or shape[-1] < 1:
        raise _lib.CapmiError('ensemble_logprobs: inputs [..., V1] expected (got %s)' % (shape,))
    for t in inputs:
        if tuple(t.shape) != shape:
            raise _lib.CapmiError('ensemble_logprobs: every member needs the same shape (%s vs %s)' % (tuple(t.shape), shape))
        if t.dtype != _f32:
            raise _lib.CapmiError('ensemble_logprobs: float32 inputs expected (got %s)' % t.dtype)
    V1 = shape[-1]

    def rows2d(t):
        if t.dim() == 2 and t.stride(1) == 1:
            return t
        if not t.is_contiguous():
            raise _lib.CapmiError('ensemble_logprobs: rows must be contiguous')
        return t.view(-1, V1)
    xs = [rows2d(t) for t in inputs]
    if not all(x.is_cuda for x in xs):
        raise _lib.CapmiError('capmi ops need device tensors (got %s)' % [str(x.device) for x in xs])
    if len({x.stride(0) for x in xs}) != 1:
        xs = [x.contiguous() for x in xs]
    if out is None:
        out = torch.empty(shape, dtype=_f32, device=inputs[0].device)
    if tuple(out.shape) != shape or out.dtype != _f32:
        raise _lib.CapmiError('ensemble_logprobs: out must be float32 of shape %s' % (shape,))
    o = rows2d(out)
    if not o.is_cuda:
        raise _lib.CapmiError('capmi ops need device tensors (got %s)' % o.device)
    if xs[0].shape[0] == 0:
        return out
    e = _lib.Ensemble()
    e.M, e.rows, e.V1 = len(xs), xs[0].shape[0], V1
    e.ld_in = xs[0].stride(0) if xs[0].shape[0] > 1 else V1
    e.ld_out = o.stride(0) if o.shape[0] > 1 else V1
    for i, (x, wi) in enumerate(zip(xs, w)):
        getattr(e, 'in')[i] = x.data_ptr()
        e.w[i] = wi
    e.out = o.data_ptr()
    check(lib.capmi_ensemble_logprobs(C.byref(e), stream_ptr()), 'capmi_ensemble_logprobs')
    return out


def _ppo_desc(lp_old, seq, n, eps, kl_coef, per_row, what):
    if lp_old.dim() != 3 or lp_old.dtype != _f32:
        raise _lib.CapmiError('%s: old log-probs [N, L, V1] float32 expected (got %s %s)' % (what, tuple(lp_old.shape), lp_old.dtype))
    N, L, V1 = lp_old.shape
    if seq.dtype != torch.int64 or tuple(seq.shape) != (N, L):
        raise _lib.CapmiError('%s: seq [N, L] = %s int64 expected (got %s %s)' % (what, (N, L), tuple(seq.shape), seq.dtype))
    if L < 1 or V1 < 1 or int(n) < 2 or N % int(n):
        raise _lib.CapmiError('%s: need L, V1 >= 1 and N = %d a multiple of n = %d >= 2' % (what, N, int(n)))
    _chk(lp_old, seq)
    p = _lib.Ppo()
    p.N, p.L, p.V1, p.n = N, L, V1, int(n)
    p.ld_new = p.ld_old = p.ld_grad = V1
    p.per_row = int(bool(per_row))
    p.eps, p.kl_coef = float(eps), float(kl_coef)
    p.lp_old, p.seq = lp_old.data_ptr(), seq.data_ptr()
    return p


def ppo_loss_fwd(lp_new, lp_old, seq, scores, n, eps=0.2, kl_coef=0.02, per_row=False):
    """PPOLoss.forward's arithmetic (losses.py:267-357) in two launches of capmi_ppo_loss_fwd.  lp_new (what the rollout returned)
    and lp_old (the old policy's log-probs): [N, L, V1] float32; seq [N, L] int64; scores [N] float32 (n samples per image,
    image-major).  Returns (out [4] = pg_loss, kl_loss, clipfrac, loss ('mean'); loss_rows [N] ('none') or None;
    row_stats [4, N, L] = kl, r, pg, d pg / d lp_new[seq]; msum [1] or [N]).  All stay on the device."""
    p = _ppo_desc(lp_old, seq, n, eps, kl_coef, per_row, 'ppo_loss_fwd')
    if tuple(lp_new.shape) != tuple(lp_old.shape) or lp_new.dtype != _f32:
        raise _lib.CapmiError('ppo_loss_fwd: lp_new must be float32 of shape %s (got %s %s)' % (tuple(lp_old.shape), tuple(lp_new.shape), lp_new.dtype))
    N, L, _ = lp_old.shape
    if scores.dtype != _f32 or tuple(scores.shape) != (N,):
        raise _lib.CapmiError('ppo_loss_fwd: scores [%d] float32 expected (got %s %s)' % (N, tuple(scores.shape), scores.dtype))
    _chk(lp_new, scores)
    dev = lp_old.device
    row_stats = torch.empty(4, N, L, dtype=_f32, device=dev)
    msum = torch.empty(N if per_row else 1, dtype=_f32, device=dev)
    out = torch.empty(4, dtype=_f32, device=dev)
    loss_rows = torch.empty(N, dtype=_f32, device=dev) if per_row else None
    p.lp_new, p.scores = lp_new.data_ptr(), scores.data_ptr()
    p.row_stats, p.msum, p.out, p.loss_rows = row_stats.data_ptr(), msum.data_ptr(), out.data_ptr(), ptr(loss_rows)
    check(lib.capmi_ppo_loss_fwd(C.byref(p), stream_ptr()), 'capmi_ppo_loss_fwd')
    return out, loss_rows, row_stats, msum


def ppo_loss_bwd(lp_old, seq, row_stats, msum, g_out, n, eps=0.2, kl_coef=0.02, per_row=False, out=None):
    """d loss / d lp_new of ppo_loss_fwd (capmi_ppo_loss_bwd, one launch): lp_old / seq / n / eps / kl_coef / per_row as given to the
    forward, row_stats and msum as it returned them, g_out the upstream gradient ([1] or 0-dim for 'mean', [N] for 'none', float32
    on the device).  Returns the dense [N, L, V1] gradient (masked rows are zeros)."""
    p = _ppo_desc(lp_old, seq, n, eps, kl_coef, per_row, 'ppo_loss_bwd')
    N, L, V1 = lp_old.shape
    g_out = g_out.reshape(-1)
    if g_out.dtype != _f32 or g_out.numel() != (N if per_row else 1):
        raise _lib.CapmiError('ppo_loss_bwd: upstream gradient of %d float32 values expected (got %s %s)'
                              % (N if per_row else 1, tuple(g_out.shape), g_out.dtype))
    if row_stats.dtype != _f32 or tuple(row_stats.shape) != (4, N, L) or msum.dtype != _f32 or msum.numel() != (N if per_row else 1):
        raise _lib.CapmiError('ppo_loss_bwd: row_stats [4, N, L] and msum as returned by ppo_loss_fwd expected')
    if out is None:
        out = torch.empty(N, L, V1, dtype=_f32, device=lp_old.device)
    if tuple(out.shape) != (N, L, V1) or out.dtype != _f32:
        raise _lib.CapmiError('ppo_loss_bwd: out must be float32 of shape %s' % ((N, L, V1),))
    g_out = g_out.contiguous()
    _chk(row_stats, msum, g_out, out)
    p.row_stats, p.msum, p.g_out, p.grad = row_stats.data_ptr(), msum.data_ptr(), g_out.data_ptr(), out.data_ptr()
    check(lib.capmi_ppo_loss_bwd(C.byref(p), stream_ptr()), 'capmi_ppo_loss_bwd')
    return out


def _xe_desc(N, T, V1, tok, mask, smoothing, per_row, what):
    for name, t, dt in (('tok', tok, torch.int64), ('mask', mask, _f32)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != dt or t.dim() != 2 or t.shape[0] != N:
            raise _lib.CapmiError('%s: %s [%d, >= T] %s on the device expected (got %s %s %s)'
                                  % (what, name, N, dt, tuple(t.shape), t.dtype, t.device))
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise _lib.CapmiError('%s: the rows of %s must be dense (stride %d)' % (what, name, t.stride(1)))
    p = _lib.XeLoss()
    p.N, p.T, p.V1 = int(N), int(T), int(V1)
    p.per_row = int(bool(per_row))
    p.smoothing = float(smoothing)
    # a [N, >= T] buffer is read through its row pitch: the cut views target[:, :T] / mask[:, :T] of the criteria need no copy
    # (a buffer narrower than T hands its width over as the pitch, which the entry point rejects)
    def pitch(t):
        return t.stride(0) if N > 1 and t.shape[1] >= T else t.shape[1]
    p.mask, p.mask_ld = mask.data_ptr(), pitch(mask)
    if tok is not None:
        p.tok, p.tok_ld = tok.data_ptr(), pitch(tok)
    else:
        p.tok_ld = p.T
    return p


def xe_loss_fwd(logp, tok, mask, smoothing=0.0, per_row=False):
    """LanguageModelCriterion (smoothing == 0) / LabelSmoothing (losses.py:204-265) in the two launches of capmi_xe_loss_fwd.
    logp [N, T, V1] float32 contiguous; tok [N, >= T] int64 and mask [N, >= T] float32 with dense rows (any row pitch: only the
    first T columns are read).  Returns (loss [1] ('mean') or [N] ('none'), msum [1] or [N], pos [N, T] the per-position
    values).  All stay on the device."""
    if logp.dim() != 3 or logp.dtype != _f32:
        raise _lib.CapmiError('xe_loss_fwd: log-probs [N, T, V1] float32 expected (got %s %s)' % (tuple(logp.shape), logp.dtype))
    _chk(logp)
    N, T, V1 = logp.shape
    p = _xe_desc(N, T, V1, tok, mask, smoothing, per_row, 'xe_loss_fwd')
    dev = logp.device
    pos = torch.empty(N, T, dtype=_f32, device=dev)
    msum = torch.empty(N if per_row else 1, dtype=_f32, device=dev)
    loss = torch.empty(N if per_row else 1, dtype=_f32, device=dev)
    p.logp, p.pos, p.msum, p.loss = logp.data_ptr(), pos.data_ptr(), msum.data_ptr(), loss.data_ptr()
    check(lib.capmi_xe_loss_fwd(C.byref(p), stream_ptr()), 'capmi_xe_loss_fwd')
    return loss, msum, pos


def xe_loss_bwd(mask, msum, T, V1, smoothing=0.0, per_row=False, g_out=None):
    """the sparse gradient of xe_loss_fwd (capmi_xe_loss_bwd, one launch): mask / smoothing / per_row as given to the forward,
    msum as it returned it, g_out None (the factor 1: a scalar loss passes its upstream gradient on as the sink's `scale`) or the
    upstream gradient, [1] / [N] float32 on the device.  Returns (g_sel [N, T], g_sum [N, T] or None without smoothing)."""
    N = mask.shape[0] if mask.dim() == 2 else -1
    p = _xe_desc(N, T, V1, None, mask, smoothing, per_row, 'xe_loss_bwd')
    if msum.dtype != _f32 or msum.numel() != (N if per_row else 1):
        raise _lib.CapmiError('xe_loss_bwd: msum as returned by xe_loss_fwd expected')
    if g_out is not None:
        g_out = g_out.reshape(-1)
        if g_out.dtype != _f32 or g_out.numel() != (N if per_row else 1):
            raise _lib.CapmiError('xe_loss_bwd: upstream gradient of %d float32 values expected (got %s %s)'
                                  % (N if per_row else 1, tuple(g_out.shape), g_out.dtype))
        g_out = g_out.contiguous()
    _chk(msum, g_out)
    g_sel = torch.empty(N, T, dtype=_f32, device=mask.device)
    g_sum = torch.empty(N, T, dtype=_f32, device=mask.device) if smoothing > 0 else None
    p.msum, p.g_out, p.g_sel, p.g_sum = msum.data_ptr(), ptr(g_out), g_sel.data_ptr(), ptr(g_sum)
    check(lib.capmi_xe_loss_bwd(C.byref(p), stream_ptr()), 'capmi_xe_loss_bwd')
    return g_sel, g_sum


def _distill_desc(lp_t, tok, mask, N, T, V1, lam, tau, per_row, what):
    """the capmi_distill descriptor of a teacher [N, >= T, V1] (dense rows, any row / sample stride), tok / mask [N, >= T]"""
    if lp_t.dim() != 3 or lp_t.dtype != _f32 or lp_t.shape[0] != N or lp_t.shape[1] < T or lp_t.shape[2] != V1:
        raise _lib.CapmiError('%s: teacher log-probs [%d, >= %d, %d] float32 expected (got %s %s)'
                              % (what, N, T, V1, tuple(lp_t.shape), lp_t.dtype))
    if V1 > 1 and lp_t.stride(2) != 1:
        raise _lib.CapmiError('%s: the rows of the teacher must be dense' % what)
    # row (i, t) at (i * t_rows + t) * ld_t: the sample stride must be a whole number of rows
    ld_t = lp_t.stride(1) if lp_t.shape[1] > 1 else V1
    t_rows = lp_t.shape[1]
    if N > 1:
        if ld_t <= 0 or lp_t.stride(0) % ld_t or lp_t.stride(0) // ld_t < lp_t.shape[1]:
            raise _lib.CapmiError('%s: teacher strides %s are not rows of one pitch' % (what, lp_t.stride()))
        t_rows = lp_t.stride(0) // ld_t
    for name, t, dt in (('tok', tok, torch.int64), ('mask', mask, _f32)):
        if t.dtype != dt or t.dim() != 2 or t.shape[0] != N or t.shape[1] < T or (t.shape[1] > 1 and t.stride(1) != 1) \
                or (N > 1 and t.stride(0) < T):
            raise _lib.CapmiError('%s: %s [%d, >= %d] %s with dense rows expected (got %s %s)' % (what, name, N, T, dt, tuple(t.shape), t.dtype))
    for t in (lp_t, tok, mask):
        if not t.is_cuda:
            raise _lib.CapmiError('capmi ops need device tensors (got %s)' % t.device)
    p = _lib.Distill()
    p.N, p.T, p.V1 = N, T, V1
    p.ld_s = p.ld_grad = V1
    p.ld_t, p.t_rows = ld_t, t_rows
    p.tok_ld = tok.stride(0) if N > 1 else tok.shape[1]
    p.mask_ld = mask.stride(0) if N > 1 else mask.shape[1]
    p.per_row = int(bool(per_row))
    setattr(p, 'lambda', float(lam))
    p.tau = float(tau)
    p.lp_t, p.tok, p.mask = lp_t.data_ptr(), tok.data_ptr(), mask.data_ptr()
    return p


def distill_loss_fwd(lp_s, lp_t, tok, mask, lam, tau=1.0, per_row=False):
    """DistillCriterion's arithmetic (capmi.h capmi_distill_loss_fwd, two launches): lp_s [N, T, V1] float32 contiguous, the student's
    teacher-forced log-probs; lp_t [N, >= T, V1] float32, the teacher's (dense rows; a [:, :T] cut or a wider row stride is read in
    place); tok [N, >= T] int64 and mask [N, >= T] float32 read through their row pitch.  Returns (out [3] = lm_loss, kd_loss, loss
    ('mean'); loss_rows [N] ('none') or None; row_stats [4, N, T] = lseS, lseT, kl, -ls[tok]; msum [1] or [N]), all on the device."""
    if lp_s.dim() != 3 or lp_s.dtype != _f32 or not lp_s.is_contiguous():
        raise _lib.CapmiError('distill_loss_fwd: student log-probs [N, T, V1] float32 contiguous expected (got %s %s)'
                              % (tuple(lp_s.shape), lp_s.dtype))
    _chk(lp_s)
    N, T, V1 = lp_s.shape
    p = _distill_desc(lp_t, tok, mask, N, T, V1, lam, tau, per_row, 'distill_loss_fwd')
    dev = lp_s.device
    row_stats = torch.empty(4, N, T, dtype=_f32, device=dev)
    msum = torch.empty(N if per_row else 1, dtype=_f32, device=dev)
    out = torch.empty(3, dtype=_f32, device=dev)
    loss_rows = torch.empty(N, dtype=_f32, device=dev) if per_row else None
    p.lp_s = lp_s.data_ptr()
    p.row_stats, p.msum, p.out, p.loss_rows = row_stats.data_ptr(), msum.data_ptr(), out.data_ptr(), ptr(loss_rows)
    check(lib.capmi_distill_loss_fwd(C.byref(p), stream_ptr()), 'capmi_distill_loss_fwd')
    return out, loss_rows, row_stats, msum


def distill_loss_bwd(lp_s, lp_t, tok, mask, row_stats, msum, g_out, lam, tau=1.0, per_row=False, out=None):
    """d loss / d lp_s of distill_loss_fwd (capmi_distill_loss_bwd, one launch): the inputs as given to the forward, row_stats and msum
    as it returned them, g_out the upstream gradient ([1] or 0-dim for 'mean', [N] for 'none', float32 on the device).  Returns the
    dense [N, T, V1] gradient (masked rows are zeros)."""
    if lp_s.dim() != 3 or lp_s.dtype != _f32 or not lp_s.is_contiguous():
        raise _lib.CapmiError('distill_loss_bwd: student log-probs [N, T, V1] float32 contiguous expected (got %s %s)'
                              % (tuple(lp_s.shape), lp_s.dtype))
    N, T, V1 = lp_s.shape
    p = _distill_desc(lp_t, tok, mask, N, T, V1, lam, tau, per_row, 'distill_loss_bwd')
    g_out = g_out.reshape(-1)
    if g_out.dtype != _f32 or g_out.numel() != (N if per_row else 1):
        raise _lib.CapmiError('distill_loss_bwd: upstream gradient of %d float32 values expected (got %s %s)'
                              % (N if per_row else 1, tuple(g_out.shape), g_out.dtype))
    if row_stats.dtype != _f32 or tuple(row_stats.shape) != (4, N, T) or not row_stats.is_contiguous() or msum.dtype != _f32 \
            or msum.numel() != (N if per_row else 1):
        raise _lib.CapmiError('distill_loss_bwd: row_stats [4, N, T] and msum as returned by distill_loss_fwd expected')
    if out is None:
        out = torch.empty(N, T, V1, dtype=_f32, device=lp_s.device)
    if tuple(out.shape) != (N, T, V1) or out.dtype != _f32 or not out.is_contiguous():
        raise _lib.CapmiError('distill_loss_bwd: out must be contiguous float32 of shape %s' % ((N, T, V1),))
    g_out = g_out.contiguous()
    _chk(lp_s, row_stats, msum, g_out, out)
    p.lp_s = lp_s.data_ptr()
    p.row_stats, p.msum, p.g_out, p.grad = row_stats.data_ptr(), msum.data_ptr(), g_out.data_ptr(), out.data_ptr()
    check(lib.capmi_distill_loss_bwd(C.byref(p), stream_ptr()), 'capmi_distill_loss_bwd')
    return out


def clip_len(att_masks, width=None):
    """Longest valid region count of the batch -- the K that clip_att (AttModel.py:106-112) truncates to.

    ``int(mask.sum(1).max())`` is a blocking device->host round trip; the value is cached on the mask tensor
    (``_capmi_kmax``) so one step pays it at most once, and the loaders / DevicePrefetcher stamp it from the host-side
    batch (they built the mask, they know kmax), so a training step never syncs for it."""
    if att_masks is None:
        return width
    k = getattr(att_masks, '_capmi_kmax', None)
    if k is None:
        k = int(att_masks.long().sum(1).max())
        try:
            att_masks._capmi_kmax = k
        except Exception:
            pass
    return k


REGION_KMAX = 1024                 # capmi.h CAPMI_REGION_KMAX
region_rows_build_calls = 0        # launches so far (tests: a second pass over a resident store launches none)


def region_rows_build(src, boxes, table_host, table, dst, norm_att, use_box, norm_box):
    """Store rows of a block of images from their raw region rows (capmi.h capmi_region_rows_build): norm_att_feat, the five
    box-geometry columns, norm_box_feat and the stable descending re-ordering by the last column, one launch.
    src [R, D] and boxes [R, 4] (None without use_box) float32 contiguous; table_host: numpy int32 [n, 4] (first row, K, height,
    width), table: the same words as an int32 device tensor; dst: a 2-D float32 view of unit column stride, D + 5 * use_box wide,
    whose rows first .. first + K - 1 are written (its row stride is the leading dimension)."""
    global region_rows_build_calls
    import numpy as np
    use_box = bool(use_box)
    n = int(table_host.shape[0]) if table_host.ndim == 2 else 0
    if table_host.dtype != np.int32 or table_host.ndim != 2 or table_host.shape[1] != 4 or not table_host.flags['C_CONTIGUOUS']:
        raise _lib.CapmiError('region_rows_build: table_host must be a contiguous int32 [n, 4] array')
    if table.dtype != torch.int32 or table.numel() != 4 * n or not table.is_contiguous() or table.device != src.device:
        raise _lib.CapmiError('region_rows_build: table must hold the %d int32 words of table_host on the device' % (4 * n))
    if src.dtype != _f32 or src.dim() != 2 or not src.is_contiguous():
        raise _lib.CapmiError('region_rows_build: src must be a contiguous float32 [rows, D] tensor')
    R, D = src.shape
    W = D + (5 if use_box else 0)
    if use_box and (boxes is None or boxes.dtype != _f32 or tuple(boxes.shape) != (R, 4) or not boxes.is_contiguous()
                    or boxes.device != src.device):
        raise _lib.CapmiError('region_rows_build: boxes must be a contiguous float32 [%d, 4] tensor' % R)
    if dst.dtype != _f32 or dst.dim() != 2 or dst.shape[1] != W or (dst.shape[0] > 1 and dst.stride(0) < W) or dst.stride(1) != 1 \
            or dst.device != src.device:
        raise _lib.CapmiError('region_rows_build: dst must be a float32 [rows, %d] view with unit column stride' % W)
    if n:                              # the rows the kernel reads and writes lie inside src / dst, no two images share one
        order = np.argsort(table_host[:, 0], kind='stable')
        first, K = table_host[order, 0].astype(np.int64), table_host[order, 1].astype(np.int64)
        if first[0] < 0 or (K <= 0).any() or (first[:-1] + K[:-1] > first[1:]).any() or first[-1] + K[-1] > min(R, dst.shape[0]):
            raise _lib.CapmiError('region_rows_build: the images\' rows overlap or leave src %s / dst %s' % (tuple(src.shape), tuple(dst.shape)))
    check(lib.capmi_region_rows_build(ptr(src), ptr(boxes) if use_box else None, table_host.ctypes.data, ptr(table), n, D, ptr(dst),
                                      dst.stride(0) if dst.shape[0] > 1 else W, int(bool(norm_att)), int(use_box), int(bool(norm_box)),
                                      stream_ptr()), 'capmi_region_rows_build')
    region_rows_build_calls += 1


# ---- the compact resident store (capmi.h capmi_rows_narrow / capmi_resident_gather, resident.hip) ---------------------------------
ROWS_DTYPES = {'fp32': (torch.float32, _lib.ROWS_F32), 'bf16': (torch.bfloat16, _lib.ROWS_BF16), 'fp16': (torch.float16, _lib.ROWS_FP16)}
_ROWS_CODE = {t: c for t, c in ROWS_DTYPES.values()}
resident_gather_calls = 0          # launches so far


def rows_l2norm(rows):
    """norm_att_feat on the device, in place: every row of the contiguous float32 [n, D] tensor over its L2 norm, bit for bit what the
    loader's host path (att / np.linalg.norm(att, 2, 1, keepdims=True)) computes."""
    if rows.dtype != _f32 or rows.dim() != 2 or not rows.is_contiguous() or not rows.is_cuda:
        raise _lib.CapmiError('rows_l2norm: rows must be a contiguous float32 [n, D] device tensor')
    if rows.shape[1] > _lib.ROWS_L2NORM_DMAX:
        raise _lib.CapmiError('rows_l2norm: rows of %d features; the kernel takes up to %d' % (rows.shape[1], _lib.ROWS_L2NORM_DMAX))
    if rows.numel():
        check(lib.capmi_rows_l2norm(ptr(rows), rows.shape[0], rows.shape[1], stream_ptr()), 'capmi_rows_l2norm')
    return rows


def rows_narrow(src, dst):
    """dst <- src rounded to nearest even, element by element: src float32 contiguous, dst a contiguous bfloat16 / float16 tensor (or
    view: any 2-byte-aligned place of a store) of the same number of elements on the same device.  The bits of src.to(dst.dtype)."""
    if src.dtype != _f32 or not src.is_contiguous() or not src.is_cuda:
        raise _lib.CapmiError('rows_narrow: src must be a contiguous float32 device tensor')
    if dst.dtype not in (torch.bfloat16, torch.float16) or not dst.is_contiguous() or dst.device != src.device \
            or dst.numel() != src.numel():
        raise _lib.CapmiError('rows_narrow: dst must be a contiguous bfloat16 / float16 tensor of %d elements on %s' % (src.numel(), src.device))
    if src.numel():
        check(lib.capmi_rows_narrow(ptr(src), ptr(dst), src.numel(), _ROWS_CODE[dst.dtype], stream_ptr()), 'capmi_rows_narrow')
    return dst


def resident_gather(rows, table_host, table, kmax):
    """One launch from the resident store to a batch: rows [n, F] contiguous float32 / bfloat16 / float16, table_host numpy int32
    [B, 2] of (first row, K) per image (K = 0: not resident), table the same words as an int32 device tensor
    -> (att [B, kmax, F] float32: the rows widened, +0.0 from K on; mask [B, kmax] float32: k < K)."""
    global resident_gather_calls
    import numpy as np
    if rows.dtype not in _ROWS_CODE or rows.dim() != 2 or not rows.is_contiguous() or not rows.is_cuda:
        raise _lib.CapmiError('resident_gather: rows must be a contiguous [n, F] float32 / bfloat16 / float16 device tensor')
    if table_host.dtype != np.int32 or table_host.ndim != 2 or table_host.shape[1] != 2 or not table_host.flags['C_CONTIGUOUS']:
        raise _lib.CapmiError('resident_gather: table_host must be a contiguous int32 [B, 2] array')
    B, kmax = int(table_host.shape[0]), int(kmax)
    if table.dtype != torch.int32 or table.numel() != 2 * B or not table.is_contiguous() or table.device != rows.device:
        raise _lib.CapmiError('resident_gather: table must hold the %d int32 words of table_host on the device' % (2 * B))
    first, K = table_host[:, 0].astype(np.int64), table_host[:, 1].astype(np.int64)
    if B < 1 or kmax < 1 or (K < 0).any() or (K > kmax).any() or ((K > 0) & ((first < 0) | (first + K > rows.shape[0]))).any():
        raise _lib.CapmiError('resident_gather: an image\'s rows leave the store %s or its K leaves 0..%d' % (tuple(rows.shape), kmax))
    F = rows.shape[1]
    att = torch.empty(B, kmax, F, dtype=_f32, device=rows.device)
    mask = torch.empty(B, kmax, dtype=_f32, device=rows.device)
    check(lib.capmi_resident_gather(ptr(rows), _ROWS_CODE[rows.dtype], F, table_host.ctypes.data, ptr(table), B, kmax, ptr(att), ptr(mask),
                                    stream_ptr()), 'capmi_resident_gather')
    resident_gather_calls += 1
    return att, mask


# ---- BatchNorm1d over the valid region rows (use_bn; capmi.h capmi_bn_*, region_norm.hip) ----------------------------------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1         # nn.BatchNorm1d's defaults, the reference's (AttModel.py:80-85)


def _bn_partial(rows, D, dev, counts=True):
    nrb = int(lib.capmi_bn_row_blocks(rows))
    return torch.empty(nrb * (2 * D + (1 if counts else 0)), dtype=_f32, device=dev), nrb


def bn_stats(x, mask, train, running_mean=None, running_var=None, num_batches_tracked=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """x [rows, D], mask [rows] floats (0 = padded row) or None -> (mean [D], rstd [D], count [1], shift [2, D]: the mean as the
    pair (pivot, mean - pivot) bn_apply subtracts).
    train: batch statistics over the valid rows (biased variance); the running buffers (unbiased variance, momentum) and
    num_batches_tracked (int64 [] / [1]) are updated in place on the stream when given.  Eval: the running statistics, nothing is
    updated.  No host read either way."""
    _chk(x, mask, running_mean, running_var)
    rows, D = x.shape
    mean, rstd = torch.empty(D, dtype=_f32, device=x.device), torch.empty(D, dtype=_f32, device=x.device)
    count = torch.empty(1, dtype=_f32, device=x.device)
    shift = torch.empty(2, D, dtype=_f32, device=x.device)
    partial = None
    if train:
        if mask is not None and mask.numel() != rows:
            raise _lib.CapmiError('bn_stats: mask must hold one float per row')
        if num_batches_tracked is not None and not (num_batches_tracked.is_cuda and num_batches_tracked.dtype == torch.long):
            raise _lib.CapmiError('bn_stats: num_batches_tracked must be an int64 device tensor')
        partial, _ = _bn_partial(rows, D, x.device)
        check(lib.capmi_bn_stats(ptr(x), ptr(mask), rows, D, ptr(partial), stream_ptr()), 'capmi_bn_stats')
    elif running_mean is None or running_var is None:
        raise _lib.CapmiError('bn_stats: eval mode needs the running statistics')
    check(lib.capmi_bn_finalize(ptr(partial), ptr(x), ptr(mask), rows, D, int(bool(train)), float(eps), float(momentum), ptr(running_mean),
                                ptr(running_var), ptr(num_batches_tracked), ptr(mean), ptr(rstd), ptr(count), ptr(shift),
                                stream_ptr()), 'capmi_bn_finalize')
    return mean, rstd, count, shift


def bn_apply(x, mask, shift, rstd, gamma, beta, out=None):
    """y = (x - mean) * rstd * gamma + beta on valid rows, 0 on padded rows; shift: bn_stats' fourth result"""
    _chk(x, mask, shift, rstd, gamma, beta, out)
    rows, D = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib.capmi_bn_apply(ptr(x), ptr(mask), ptr(shift), ptr(rstd), ptr(gamma), ptr(beta), ptr(out), rows, D, stream_ptr()),
          'capmi_bn_apply')
    return out


def bn_backward(dy, x, mask, mean, rstd, gamma, count, train, dgamma, dbeta, dx=None):
    """Backward of bn_apply(bn_stats(x)) over the valid rows: dgamma / dbeta [D] are overwritten, -> dx (0 on padded rows; may be dy).
    train: the full BatchNorm Jacobian (batch statistics); eval: the statistics are constants."""
    _chk(dy, x, mask, mean, rstd, gamma, dgamma, dbeta, dx)
    rows, D = x.shape
    partial, nrb = _bn_partial(rows, D, x.device, counts=False)
    check(lib.capmi_bn_bwd_partial(ptr(dy), ptr(x), ptr(mask), ptr(mean), ptr(rstd), rows, D, ptr(partial), stream_ptr()),
          'capmi_bn_bwd_partial')
    check(lib.capmi_bn_colsum_parts(ptr(partial), nrb, D, ptr(dbeta), ptr(dgamma), stream_ptr()), 'capmi_bn_colsum_parts')
    if dx is None:
        dx = torch.empty_like(dy)
    check(lib.capmi_bn_bwd_dx(ptr(dy), ptr(x), ptr(mask), ptr(mean), ptr(rstd), ptr(gamma), ptr(dgamma), ptr(dbeta), ptr(count),
                              int(bool(train)), ptr(dx), rows, D, stream_ptr()), 'capmi_bn_bwd_dx')
    return dx


def bn_linear_bwd(G, db, W, mean, rstd, gamma, beta, dgamma, dbeta):
    """BatchNorm in front of a Linear whose input needs no gradient: G [R, D] holds d_pre^T x on the RAW input and becomes the
    Linear's weight gradient; dgamma / dbeta [D] are overwritten (capmi.h capmi_bn_linear_bwd)."""
    _chk(G, db, W, mean, rstd, gamma, beta, dgamma, dbeta)
    R, D = W.shape
    partial, nrb = _bn_partial(R, D, W.device, counts=False)
    check(lib.capmi_bn_linear_bwd(ptr(G), ptr(db), ptr(W), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), R, D, ptr(partial),
                                  stream_ptr()), 'capmi_bn_linear_bwd')
    check(lib.capmi_bn_colsum_parts(ptr(partial), nrb, D, ptr(dgamma), ptr(dbeta), stream_ptr()), 'capmi_bn_colsum_parts')
    return partial


# ---- CIDEr-D document frequencies of a caption corpus (tools/prepro_ngrams.py; capmi.h capmi_df_*, df_build.hip) -----------------
def _host_offsets(off, n):
    """numpy int64 [n + 1] offsets for the host-side check of capmi_df_count (None: not checked there)"""
    import numpy as np
    if off is None:
        return None
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off.shape != (n + 1,):
        raise _lib.CapmiError('df_count: host offsets must be [%d], got %s' % (n + 1, off.shape))
    return off


def df_count(tok, cap_off, img_off, table_keys, table_counts, meta, cap_off_host=None, img_off_host=None):
    """One launch (capmi_df_count): every distinct n-gram (n = 1..4) of an image's captions adds 1 to the counting table.
    tok int32 / int64 [total_tokens]; cap_off int64 [n_caps + 1]; img_off int64 [n_img + 1]; table_keys int64 (the bits of uint64) and
    table_counts int32 [cap], cap a power of two; meta int32 [2] = error bits, distinct n-grams; tables and meta zeroed by the
    caller.  cap_off_host / img_off_host: the same offsets on the host (numpy), checked before the launch.  No host sync."""
    _chk(tok, cap_off, img_off, table_keys, table_counts, meta)
    if tok.dtype not in (torch.int32, torch.int64) or tok.dim() != 1:
        raise _lib.CapmiError('df_count: tok must be a 1-D int32 or int64 tensor')
    if cap_off.dtype != torch.int64 or img_off.dtype != torch.int64 or cap_off.dim() != 1 or img_off.dim() != 1 \
            or cap_off.numel() < 1 or img_off.numel() < 1:
        raise _lib.CapmiError('df_count: cap_off and img_off must be 1-D int64 tensors of at least one entry')
    if table_keys.dtype != torch.int64 or table_counts.dtype != torch.int32 or table_keys.numel() != table_counts.numel():
        raise _lib.CapmiError('df_count: the counting table is int64 keys and int32 counts of one size')
    if meta.dtype != torch.int32 or meta.numel() != 2:
        raise _lib.CapmiError('df_count: meta must be int32 [2]')
    n_caps, n_img = cap_off.numel() - 1, img_off.numel() - 1
    ch, ih = _host_offsets(cap_off_host, n_caps), _host_offsets(img_off_host, n_img)
    check(lib.capmi_df_count(ptr(tok) if tok.numel() else None, tok.element_size(), tok.numel(), ptr(cap_off),
                             ch.ctypes.data if ch is not None else None, n_caps, ptr(img_off),
                             ih.ctypes.data if ih is not None else None, n_img, ptr(table_keys), ptr(table_counts),
                             table_keys.numel(), meta.data_ptr() + 4, ptr(meta), stream_ptr()), 'capmi_df_count')


def df_finalize(count_keys, counts, keys, vals, meta):
    """One launch (capmi_df_finalize): the occupied slots of the counting table re-inserted into the scorer's image, keys int64
    (the bits of uint64) / vals float64 [cap], zeroed by the caller, cap a power of two.  meta: as df_count."""
    _chk(count_keys, counts, keys, vals, meta)
    if count_keys.dtype != torch.int64 or counts.dtype != torch.int32 or count_keys.numel() != counts.numel():
        raise _lib.CapmiError('df_finalize: the counting table is int64 keys and int32 counts of one size')
    if keys.dtype != torch.int64 or vals.dtype != torch.float64 or keys.numel() != vals.numel():
        raise _lib.CapmiError('df_finalize: the image is int64 keys and float64 vals of one size')
    check(lib.capmi_df_finalize(ptr(count_keys), ptr(counts), count_keys.numel(), ptr(keys), ptr(vals), keys.numel(), ptr(meta),
                                stream_ptr()), 'capmi_df_finalize')


# ---- stochastic beam search (beam.stochastic_beam_search_steps; capmi.h capmi_sbs_*, sbs.hip) ------------------------------------
SBS_BD_MAX = 16       # = BD_MAX of csrc/search_common.h, the one definition beam.hip and sbs.hip share


def _chunk_list_scratch(scratch_bytes, B, cur, b, V1, dev):
    """the chunk lists between the row kernel and the merge kernel of a select step (csrc/search_common.h) -> (buffer, its bytes)"""
    nbytes = max(int(scratch_bytes(B, cur, b, V1)), 4)
    return torch.empty(nbytes // 4, dtype=torch.int32, device=dev), nbytes


def sbs_select(logp, phi, g, alive, bd, step0=False, force_end=False, gumbel=None, seed=0, offset=0, out=None):
    """One selection step of the stochastic beam search (capmi_sbs_select): logp [B * cur, V1] normalised rows, phi / g float32 and
    alive uint8 [B, cur]; noise: `gumbel` [B * cur, V1] (injected) or Philox (seed, offset = the step).  Returns (parent int32,
    token int64, phi_out, g_out, alive_out uint8), each [B, bd], by descending g_out (out: the same five, preallocated)."""
    _chk(logp, phi, g, alive, gumbel)
    B, cur = phi.shape
    V1 = logp.shape[1]
    if logp.dtype != _f32 or phi.dtype != _f32 or g.dtype != _f32 or alive.dtype != torch.uint8 or logp.shape[0] != B * cur \
            or g.shape != phi.shape or alive.shape != phi.shape:
        raise _lib.CapmiError('sbs_select: logp float32 [B * cur, V1], phi / g float32 [B, cur], alive uint8 [B, cur]')
    if gumbel is not None and (gumbel.dtype != _f32 or gumbel.shape != logp.shape):
        raise _lib.CapmiError('sbs_select: gumbel must be float32 %s' % (tuple(logp.shape),))
    dev = logp.device
    if out is None:
        out = (torch.empty(B, bd, dtype=torch.int32, device=dev), torch.empty(B, bd, dtype=torch.long, device=dev),
               torch.empty(B, bd, dtype=_f32, device=dev), torch.empty(B, bd, dtype=_f32, device=dev),
               torch.empty(B, bd, dtype=torch.uint8, device=dev))
    _chk(*out)
    scratch, nbytes = _chunk_list_scratch(lib.capmi_sbs_scratch_bytes, B, cur, bd, V1, dev)
    check(lib.capmi_sbs_select(ptr(logp), ptr(phi), ptr(g), ptr(alive), ptr(gumbel), int(seed) & 0xFFFFFFFFFFFFFFFF,
                               int(offset) & 0xFFFFFFFF, B, cur, int(bd), V1, int(bool(step0)), int(bool(force_end)), ptr(scratch),
                               nbytes, *[ptr(t) for t in out], stream_ptr()), 'capmi_sbs_select')
    return out


def sbs_backtrack(parent, token, alive):
    """capmi_sbs_backtrack: the tables [L, B, bd] of a finished search -> (seq int64 [B * bd, L], length int32 [B * bd],
    lineage int32 [L, B * bd]), with the conventions of beam.finalize."""
    _chk(parent, token, alive)
    L, B, bd = parent.shape
    if parent.dtype != torch.int32 or token.dtype != torch.long or alive.dtype != torch.uint8 or token.shape != parent.shape \
            or alive.shape != parent.shape:
        raise _lib.CapmiError('sbs_backtrack: parent int32, token int64, alive uint8, all [L, B, bd]')
    dev = parent.device
    seq = torch.empty(B * bd, L, dtype=torch.long, device=dev)
    length = torch.empty(B * bd, dtype=torch.int32, device=dev)
    lineage = torch.empty(L, B * bd, dtype=torch.int32, device=dev)
    check(lib.capmi_sbs_backtrack(ptr(parent), ptr(token), ptr(alive), B, bd, L, ptr(seq), ptr(length), ptr(lineage), stream_ptr()),
          'capmi_sbs_backtrack')
    return seq, length, lineage


# ---- constrained beam search (beam.constrained_beam_search_steps; capmi.h capmi_cbs_*, cbs.hip) ----------------------------------
CBS_C_MAX, CBS_W_MAX, CBS_SLOTS_MAX = 4, 8, 64


class CbsTables:
    """The constraint tables of a batch on the device, checked on the host before the upload (capmi_cbs_select trusts them):
    words [B, 4, 8] int32 padded with -1, ncons [B] int32, for a vocabulary of V1 columns and S states."""

    def __init__(self, words, ncons, V1, S, dev):
        words, ncons = torch.as_tensor(words), torch.as_tensor(ncons)
        if words.is_cuda or ncons.is_cuda:
            raise _lib.CapmiError('cbs_tables: the tables are checked on the host; pass CPU tensors')
        if words.dim() != 3 or tuple(words.shape[1:]) != (CBS_C_MAX, CBS_W_MAX) or ncons.shape != (words.shape[0],):
            raise _lib.CapmiError('cbs_tables: words [B, %d, %d], ncons [B] (EINVAL)' % (CBS_C_MAX, CBS_W_MAX))
        words, ncons = words.to(torch.int32).contiguous(), ncons.to(torch.int32).contiguous()
        if bool(((words != -1) & ((words < 1) | (words >= V1))).any()):
            raise _lib.CapmiError('cbs_tables: a word id outside [1, %d) (EINVAL)' % V1)
        if bool((ncons < 0).any()) or bool(((1 << ncons.long()) > S).any()):
            raise _lib.CapmiError('cbs_tables: ncons needs 2^ncons <= S = %d (EINVAL)' % S)
        self.V1, self.S, self.B = int(V1), int(S), words.shape[0]
        self.words, self.ncons = words.to(dev), ncons.to(dev)


def cbs_tables(words, ncons, V1, S, dev):
    return CbsTables(words, ncons, V1, S, dev)


def cbs_select(logp, sums, tables, b, S, force_end=False, out=None):
    """One selection step of the constrained beam search (capmi_cbs_select): logp float32 [B * cur, V1] (cur = 1: the root, or S * b),
    sums float32 [B, S * b] (-inf: an empty slot), tables a CbsTables made for the same V1 and S.  Returns (parent int32, token
    int64, score, next_sums, ended uint8, valid uint8), each [B, S * b] (out: the same six, preallocated)."""
    if not isinstance(tables, CbsTables):
        raise _lib.CapmiError('cbs_select: tables must come from ops.cbs_tables')
    _chk(logp, sums, tables.words, tables.ncons)
    B, SB = sums.shape
    V1 = logp.shape[1]
    b, S = int(b), int(S)
    if logp.dtype != _f32 or sums.dtype != _f32 or logp.dim() != 2 or B <= 0 or logp.shape[0] % B:
        raise _lib.CapmiError('cbs_select: logp float32 [B * cur, V1], sums float32 [B, S * b]')
    cur = logp.shape[0] // B
    if tables.V1 != V1 or tables.S != S or tables.B != B:
        raise _lib.CapmiError('cbs_select: the tables were checked for B = %d, V1 = %d, S = %d (EINVAL)' % (tables.B, tables.V1, tables.S))
    if S * b != SB:
        raise _lib.CapmiError('cbs_select: sums must be [B, S * b] (EINVAL)')
    dev = logp.device
    if out is None:
        e = lambda dt: torch.empty(B, SB, dtype=dt, device=dev)      # noqa: E731
        out = (e(torch.int32), e(torch.long), e(_f32), e(_f32), e(torch.uint8), e(torch.uint8))
    _chk(*out)
    scratch, nbytes = _chunk_list_scratch(lib.capmi_cbs_scratch_bytes, B, cur, b, V1, dev)
    check(lib.capmi_cbs_select(ptr(logp), ptr(sums), ptr(tables.words), ptr(tables.ncons), B, cur, b, S, V1, int(bool(force_end)),
                               ptr(scratch), nbytes, *[ptr(t) for t in out], stream_ptr()), 'capmi_cbs_select')
    return out


def cbs_finalize(parent, token, score, ended, valid, ncons, b, S, len_div=None):
    """capmi_cbs_finalize: the tables [L, B, S * b] of a finished search and ncons int32 [B] (device) -> (seq int64 [B, L],
    lineage int32 [L, B], length int32 [B], state int32 [B], score float32 [B]); len_div float64 [L] or None."""
    _chk(parent, token, score, ended, valid, ncons, len_div)
    L, B, SB = parent.shape
    if parent.dtype != torch.int32 or token.dtype != torch.long or score.dtype != _f32 or ended.dtype != torch.uint8 \
            or valid.dtype != torch.uint8 or ncons.dtype != torch.int32 or ncons.shape != (B,) \
            or any(t.shape != parent.shape for t in (token, score, ended, valid)) or SB != int(S) * int(b):
        raise _lib.CapmiError('cbs_finalize: parent int32, token int64, score float32, ended / valid uint8, all [L, B, S * b]; '
                              'ncons int32 [B]')
    if len_div is not None and (len_div.dtype != torch.float64 or len_div.shape != (L,)):
        raise _lib.CapmiError('cbs_finalize: len_div float64 [L]')
    dev = parent.device
    seq = torch.empty(B, L, dtype=torch.long, device=dev)
    lineage = torch.empty(L, B, dtype=torch.int32, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    state = torch.empty(B, dtype=torch.int32, device=dev)
    out_score = torch.empty(B, dtype=_f32, device=dev)
    check(lib.capmi_cbs_finalize(ptr(parent), ptr(token), ptr(score), ptr(ended), ptr(valid), ptr(ncons), ptr(len_div), B, int(b),
                                 int(S), L, ptr(seq), ptr(lineage), ptr(length), ptr(state), ptr(out_score), stream_ptr()),
          'capmi_cbs_finalize')
    return seq, lineage, length, state, out_score


# ---- scoring given captions (score.score_captions; capmi.h capmi_score_step / capmi_retrieval_rank, score.hip) ----------------------
def _rows_of(x, what):
    """a float32 device matrix whose rows are contiguous (any row stride >= the width) -> its row stride"""
    if not x.is_cuda:
        raise _lib.CapmiError('capmi ops need device tensors (got %s)' % x.device)
    if x.dtype != _f32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise _lib.CapmiError('%s: a float32 matrix with contiguous rows' % what)
    return x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


def score_step(logits, tok, live, acc, cnt, tok_logp=None, inv_temperature=1.0, unk_col=-1):
    """capmi_score_step, in place: logits float32 [rows, V1] (rows may be strided), tok int64 [rows], live uint8 [rows], acc float32
    [rows], cnt int32 [rows], tok_logp float32 [rows] or None.  Live rows: acc += log p(tok), cnt += 1, tok_logp = it, live = 0
    behind token 0; dead rows are untouched.  The tokens are trusted to lie in [0, V1) (score.py checks them on the host)."""
    ld = _rows_of(logits, 'score_step: logits')
    _chk(tok, live, acc, cnt, tok_logp)
    rows, V1 = logits.shape
    if tok.dtype != torch.long or live.dtype != torch.uint8 or acc.dtype != _f32 or cnt.dtype != torch.int32 \
            or any(t.shape != (rows,) for t in (tok, live, acc, cnt)) \
            or (tok_logp is not None and (tok_logp.dtype != _f32 or tok_logp.shape != (rows,))):
        raise _lib.CapmiError('score_step: tok int64, live uint8, acc float32, cnt int32[, tok_logp float32], all [rows]')
    check(lib.capmi_score_step(ptr(logits), ld, rows, V1, ptr(tok), ptr(live), ptr(acc), ptr(cnt), ptr(tok_logp),
                               float(inv_temperature), int(unk_col), stream_ptr()), 'capmi_score_step')


def retrieval_rank(S, target, log_post=True):
    """capmi_retrieval_rank: S float32 [C, I] (rows may be strided), target [C] (host or device; checked on the host to lie in
    [0, I)) -> (rank int32 [C], log_post float32 [C] or None): 1 + the images that score higher than the caption's own, ties to the
    lower image index, and the log-posterior of the own image under a uniform prior."""
    ld = _rows_of(S, 'retrieval_rank: S')
    C, I = S.shape
    target = torch.as_tensor(target)
    if target.shape != (C,) or target.dtype.is_floating_point:
        raise _lib.CapmiError('retrieval_rank: target holds one image index per caption')
    if C and (int(target.min()) < 0 or int(target.max()) >= I):
        raise _lib.CapmiError('retrieval_rank: a target outside [0, %d) (EINVAL)' % I)
    target = target.to(device=S.device, dtype=torch.int32).contiguous()
    rank = torch.empty(C, dtype=torch.int32, device=S.device)
    post = torch.empty(C, dtype=_f32, device=S.device) if log_post else None
    check(lib.capmi_retrieval_rank(ptr(S), ld, C, I, ptr(target), ptr(rank), ptr(post), stream_ptr()), 'capmi_retrieval_rank')
    return rank, post


# ---- discriminative decoding (disc.DiscStepper; capmi.h capmi_disc_combine, disc.hip) ---------------------------------------------
DISC_MODES = {'suppress': _lib.DISC_SUPPRESS, 'listener': _lib.DISC_LISTENER}


def disc_combine(logits, present, lam, mode, B, D1, cur, out=None):
    """capmi_disc_combine: logits float32 [B * D1 * cur, V1] (slot-major: row (b * D1 + d) * cur + j; rows may be strided), present
    uint8 [B, D1] (column 0 the target) -> out float32 [B * cur, V1], the pragmatic row of every hypothesis (capmi.h has the
    formulas of mode 'suppress' / 'listener' and the edge cases).  One launch, nothing reads the device."""
    if mode not in DISC_MODES:
        raise _lib.CapmiError("disc_combine: mode is 'suppress' or 'listener' (got %r)" % (mode,))
    B, D1, cur, lam = int(B), int(D1), int(cur), float(lam)
    if not 1 <= D1 <= _lib.DISC_MAX:
        raise _lib.CapmiError('disc_combine: 1..%d slots per image (got %d)' % (_lib.DISC_MAX, D1))
    if not 0.0 <= lam <= 1.0:
        raise _lib.CapmiError('disc_combine: lambda lies in [0, 1] (got %r)' % (lam,))
    ld_in = _rows_of(logits, 'disc_combine: logits')
    rows, V1 = logits.shape
    if B < 0 or cur < 0 or rows != B * D1 * cur or V1 < 1:
        raise _lib.CapmiError('disc_combine: logits [B * D1 * cur, V1] = [%d, V1 >= 1] expected (got %s)' % (B * D1 * cur, tuple(logits.shape)))
    _chk(present)
    if present.dtype != torch.uint8 or tuple(present.shape) != (B, D1):
        raise _lib.CapmiError('disc_combine: present uint8 [B, D1] = [%d, %d] expected (got %s %s)' % (B, D1, present.dtype, tuple(present.shape)))
    if out is None:
        out = torch.empty(B * cur, V1, dtype=_f32, device=logits.device)
    ld_out = _rows_of(out, 'disc_combine: out')
    if tuple(out.shape) != (B * cur, V1):
        raise _lib.CapmiError('disc_combine: out [B * cur, V1] = [%d, %d] expected (got %s)' % (B * cur, V1, tuple(out.shape)))
    if rows == 0:
        return out
    d = _lib.Disc()
    d.B, d.D1, d.cur, d.V1, d.ld_in, d.ld_out, d.mode = B, D1, cur, V1, ld_in, ld_out, DISC_MODES[mode]
    setattr(d, 'lambda', lam)
    setattr(d, 'in', logits.data_ptr())
    d.present, d.out = present.data_ptr(), out.data_ptr()
    check(lib.capmi_disc_combine(C.byref(d), stream_ptr()), 'capmi_disc_combine')
    return out
