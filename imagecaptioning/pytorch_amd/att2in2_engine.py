"""Host-side driver of the Att2in2 decoder (configs/a2i2*.yml) on libcapmi: buffers + one native call per rollout.

  prepare()            AttModel._prepare_feature (AttModel.py:114-124) without fc_embed (Att2in2Model, :854-859)
  Rollout.run()        AttModel._sample / _forward over Att2in2Core (:750-790)
  Rollout.backward()   the BPTT torch would have recorded for them
  prepare_backward()   att_embed / ctx2att gradients
"""
import ctypes as C

import torch

from . import _lib, ops
from .ops import clip_len
from ._lib import lib, ptr, check, stream_ptr
from .updown_engine import Prepared, _relu_drop_bwd

_f32 = torch.float32
_W = (('embed', 'embed.0.weight'), ('i2h_w', 'core.i2h.weight'), ('i2h_b', 'core.i2h.bias'), ('h2h_w', 'core.h2h.weight'),
      ('h2h_b', 'core.h2h.bias'), ('a2c_w', 'core.a2c.weight'), ('a2c_b', 'core.a2c.bias'),
      ('h2att_w', 'core.attention.h2att.weight'), ('h2att_b', 'core.attention.h2att.bias'),
      ('alpha_w', 'core.attention.alpha_net.weight'), ('alpha_b', 'core.attention.alpha_net.bias'), ('logit_w', 'logit.weight'),
      ('logit_b', 'logit.bias'))


def weights_struct(P):
    w = _lib.Att2in2Weights()
    for f, k in _W:
        t = P[k]
        if not (t.is_cuda and t.is_contiguous() and t.dtype == _f32):
            raise _lib.CapmiError('parameter %s must be a contiguous fp32 device tensor' % k)
        setattr(w, f, t.data_ptr())
    return w


def prepare(P, att_feats, att_masks=None, drop_att=None, ws=None):
    """att' = drop(relu(att_embed(att))) with padded regions zeroed (pack_wrapper, AttModel.py:44-49), p_att = ctx2att(att').
    drop_att: [B,K,R] keep mask of the att_embed dropout (train mode) or None."""
    if att_masks is not None:
        max_len = clip_len(att_masks)          # clip_att, AttModel.py:106-112
        att_feats = att_feats[:, :max_len].contiguous()
        att_masks = att_masks[:, :max_len].contiguous().float()
        if drop_att is not None:
            drop_att = drop_att[:, :max_len].contiguous()
    B, K = att_feats.shape[:2]
    R = P['att_embed.0.weight'].shape[0]
    pr = Prepared()
    pr.K, pr.fc, pr.fc_in, pr.drop_fc = K, None, None, None
    pr.att_in = att_feats.contiguous()
    m = drop_att
    if att_masks is not None:
        am = att_masks.unsqueeze(-1).expand(B, K, R)
        m = (am if drop_att is None else am * drop_att).contiguous()
    pr.drop_att = m
    att2d = ops.linear(pr.att_in.view(B * K, -1), P['att_embed.0.weight'], P['att_embed.0.bias'], relu=True,
                       mul_mask=None if m is None else m.view(B * K, R), ws=ws)
    pr.att = att2d.view(B, K, R)
    pr.p_att = ops.linear(att2d, P['ctx2att.weight'], P['ctx2att.bias'], ws=ws).view(B, K, -1)
    pr.att_masks = att_masks
    return pr


def prepare_backward(P, pr, d_att, d_p_att, grads, ws=None):
    """Backward of prepare(): fills grads[...] for att_embed / ctx2att (overwrite).  d_att is accumulated into."""
    B, K, R = pr.att.shape
    A = pr.p_att.shape[2]
    dp = d_p_att.view(B * K, A)
    att2d = pr.att.view(B * K, R)
    d_att_total = d_att.view(B * K, R)
    ops.gemm([(dp, A, P['ctx2att.weight'], R, A, 1)], B * K, R, d_att_total, a_layout=0, b_layout=1, accumulate=True, ws=ws)
    d_pre = _relu_drop_bwd(d_att_total, att2d, None if pr.drop_att is None else pr.drop_att.view(B * K, R))
    items = []
    for dy, x, wname, bname in ((dp, att2d, 'ctx2att.weight', 'ctx2att.bias'),
                                (d_pre, pr.att_in.view(B * K, -1), 'att_embed.0.weight', 'att_embed.0.bias')):
        if grads[bname].data_ptr() % 16 == 0:
            items.append((dy, x, grads[wname], False, None, 0, grads[bname]))
        else:
            ops.matmul_tn(dy, x, out=grads[wname], ws=ws)
            ops.colsum(dy, out=grads[bname])
    if items:
        ops.gemm_group_tn(items, ws=ws)
    return d_pre, dp


class Rollout:
    """Device buffers + one native call for a T-step rollout of N = B*n caption rows."""

    def __init__(self, P, pr, n, T, L=None, mode='greedy', temperature=1.0, drop_xt=None, drop_out=None, gumbel=None, seed=0,
                 forced=None, teacher=False, ss_mode=None, raw=False, ws=None):
        """ss_mode (uint8 [T,N], teacher only): scheduled sampling, 1 = the input of (step, row) is drawn from the previous
        step's distribution, 2 = teacher-forced (as updown_engine.Rollout).  raw (free-running): the stored rows are the logits."""
        dev = pr.att.device
        B, K, R = pr.att.shape
        A = pr.p_att.shape[2]
        V1, E = P['embed.0.weight'].shape
        N = B * n
        L = T if L is None else L
        self.P, self.pr, self.dims = P, pr, (B, n, N, K, A, R, E, V1, T, L)
        self.ws = ws or ops.default_workspace(dev)
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        self.h, self.c = z(T + 1, N, R), z(T + 1, N, R)
        self.x, self.saved, self.h_drop = z(T, N, E), z(T, N, 5 * R), z(T, N, R)
        self.att_h, self.alpha, self.ctx = z(T, N, A), z(T, N, K), z(T, N, R)
        self.xin = z(T, N, 5 * R) if (teacher and ss_mode is None) else None
        self.it_all = torch.empty(T, N, dtype=torch.long, device=dev)
        zl = torch.empty if T == L else torch.zeros      # the select writes every (row, step < T) slot
        self.seq = zl(N, L, dtype=torch.long, device=dev)
        self.seq_logp = zl(N, L, V1, dtype=_f32, device=dev)
        self.sel_logp = zl(N, L, dtype=_f32, device=dev)
        self.live = zl(N, L, dtype=torch.uint8, device=dev)
        self.it = torch.empty(N, dtype=torch.long, device=dev)
        self.unfinished = torch.empty(N, dtype=torch.uint8, device=dev)
        self.drop_xt, self.drop_out, self.gumbel, self.forced, self.ss_mode = drop_xt, drop_out, gumbel, forced, ss_mode
        if ss_mode is not None:
            assert teacher and ss_mode.dtype == torch.uint8 and ss_mode.shape == (T, N) and ss_mode.is_contiguous()
        if forced is not None:
            assert forced.dtype == torch.long and forced.is_contiguous()
        r = _lib.Att2in2Rollout()
        r.B, r.n, r.N, r.K, r.A, r.R, r.E, r.V1, r.T, r.L = B, n, N, K, A, R, E, V1, T, L
        r.att, r.p_att, r.att_mask = ptr(pr.att), ptr(pr.p_att), ptr(pr.att_masks)
        r.drop_xt, r.drop_out = ptr(drop_xt), ptr(drop_out)
        r.mode = {'greedy': 0, 'sample': 1, 'forced': 2}[mode] | (_lib.SELECT_RAW if (raw and not teacher) else 0)
        r.temperature, r.gumbel, r.seed = float(temperature), ptr(gumbel), int(seed) & 0xFFFFFFFFFFFFFFFF
        if forced is not None:
            r.forced, r.forced_ld = ptr(forced), forced.shape[1]
        r.teacher, r.ss_mode = int(teacher), ptr(ss_mode)
        for k in ('h', 'c', 'x', 'it_all', 'xin', 'att_h', 'alpha', 'ctx', 'saved', 'h_drop', 'seq', 'seq_logp', 'sel_logp', 'live',
                  'it', 'unfinished'):
            setattr(r, k, ptr(getattr(self, k)))
        r.partial, r.partial_capacity = self.ws.buf.data_ptr(), self.ws.capacity
        self.r, self.w = r, weights_struct(P)

    def run(self):
        check(lib.capmi_att2in2_rollout_fwd(C.byref(self.w), C.byref(self.r), stream_ptr()), 'capmi_att2in2_rollout_fwd')
        return self.seq, self.seq_logp

    def backward(self, g_seq_logp, grads, sparse=None):
        """g_seq_logp [N,L,V1] (None when `sparse` carries the loss gradient); grads: name -> preallocated fp32 tensor (overwritten)
        for every parameter, the prefill's att_embed / ctx2att included."""
        B, n, N, K, A, R, E, V1, T, L = self.dims
        dev = self.seq.device
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        keep = dict(dlogits=z(T, N, V1), d_hdrop=z(T, N, R), d_sums=z(T, N, 5 * R), d_ctx=z(T, N, R), d_att_h=z(T, N, A),
                    d_e=z(T, N, K), dc=z(2, N, R), d_x=z(T, N, E))
        s = _lib.Att2in2BwdScratch()
        for k, t in keep.items():
            setattr(s, k, t.data_ptr())
        s.partial, s.partial_capacity = self.ws.buf.data_ptr(), self.ws.capacity
        if sparse is not None:
            s.sparse = C.pointer(sparse)
        g = _lib.Att2in2Grads()
        for f, k in _W:
            setattr(g, f, grads[k].data_ptr())
        d_att, d_p_att = z(B, K, R), z(B, K, A)
        g.d_att, g.d_p_att = d_att.data_ptr(), d_p_att.data_ptr()
        g_seq_logp = None if g_seq_logp is None else g_seq_logp.contiguous()
        check(lib.capmi_att2in2_rollout_bwd(C.byref(self.w), C.byref(self.r), ptr(g_seq_logp), C.byref(s), C.byref(g),
                                            stream_ptr()), 'capmi_att2in2_rollout_bwd')
        kp = prepare_backward(self.P, self.pr, d_att, d_p_att, grads, ws=self.ws)
        self._keep = (keep, d_att, d_p_att, g_seq_logp, kp)     # scratch alive until the stream has consumed it
