"""What the host-side drivers of the recurrent families (UpDown, NewFC, Att2in2, AdaAtt) share.

  fill_struct()                  parameter / gradient tensors -> pointer fields of a capmi.h struct
  Prepared, prepare(), prepare_backward()
                                 AttModel._prepare_feature (AttModel.py:114-124) and its backward; fc_embed optional
  att_linear(), RegionBN         use_bn: the name of att_embed's Linear, the BatchNorm layers' buffers and mode
  RolloutBase                    the select-side buffers, the sampling / forcing fields of capmi_*_rollout, run(), and the struct
                                 filling of backward()

A family's engine states its ctypes types, its field tables, its activation buffers and its native entry points, and keeps what
really is its own ("Adding a recurrent family").
"""
import ctypes as C

import torch

from . import _lib, ops
from .ops import clip_len
from ._lib import lib, ptr, check, stream_ptr

_f32 = torch.float32
MODES = {'greedy': 0, 'sample': 1, 'forced': 2}


def fill_struct(struct, fields, tensors, validate=True):
    """struct.<field> = tensors[name].data_ptr() for every (field, name); validate: refuse what a kernel would misread"""
    for f, k in fields:
        t = tensors[k]
        if validate and not (t.is_cuda and t.is_contiguous() and t.dtype == _f32):
            raise _lib.CapmiError('parameter %s must be a contiguous fp32 device tensor' % k)
        setattr(struct, f, t.data_ptr())
    return struct


class Prepared:
    """fc' [B,R], att' [B,K,R], p_att [B,K,A] (+ what the backward of the prefill needs)."""
    __slots__ = ('fc', 'att', 'p_att', 'att_masks', 'fc_in', 'att_in', 'drop_fc', 'drop_att', 'K', 'bn', 'bn1', 'bn2', 'att_pre', 'bn_keep')

    @classmethod
    def of_features(cls, att, p_att, att_masks):
        """features that are already embedded, one row each (get_logprobs_state, AttModel.py:166-176); a family with an fc
        feature sets pr.fc itself"""
        pr = cls()
        pr.fc = None
        pr.att, pr.p_att = att.float().contiguous(), p_att.float().contiguous()
        pr.att_masks = None if att_masks is None else att_masks.float().contiguous()
        pr.K = pr.att.shape[1]
        return pr


ATT_BN1, ATT_BN2 = 'att_embed.0', 'att_embed.4'      # the BatchNorm1d layers of use_bn (AttModel.py:80-85); gamma / beta live in P


def att_linear(P):
    """name of att_embed's Linear: index 0 of the Sequential, index 1 behind the BatchNorm1d of use_bn (AttModel.py:80-85).  The one
    place that knows; without use_bn index 1 is the ReLU and has no parameters."""
    return 'att_embed.1' if 'att_embed.1.weight' in P else 'att_embed.0'


class RegionBN:
    """The state of att_embed's BatchNorm layers for one prefill: train (batch statistics over the valid region rows, running
    buffers updated once, in place, on the stream) or eval (running statistics, nothing written), and per layer the buffers
    (running_mean, running_var, num_batches_tracked).  bn2 is None unless use_bn == 2."""
    __slots__ = ('train', 'bn1', 'bn2')

    def __init__(self, train, bn1, bn2=None):
        self.train, self.bn1, self.bn2 = bool(train), tuple(bn1), None if bn2 is None else tuple(bn2)

    @classmethod
    def of_module(cls, att_embed, use_bn, train):
        """att_embed: the nn.Sequential of AttModel.py:80-85 -> its state (None without use_bn)"""
        if not use_bn:
            return None
        bufs = lambda m: (m.running_mean, m.running_var, m.num_batches_tracked)      # noqa: E731
        return cls(train, bufs(att_embed[0]), bufs(att_embed[4]) if use_bn == 2 else None)

    def eval(self):
        return RegionBN(False, self.bn1, self.bn2)


def _check_bn(P, bn):
    has = att_linear(P) == 'att_embed.1'
    if has and bn is None:
        raise _lib.CapmiError('these parameters have BatchNorm layers around att_embed (use_bn): the prefill needs their running '
                              'buffers (engine_common.RegionBN)')
    if bn is not None and (not has or ((ATT_BN2 + '.weight') in P) != (bn.bn2 is not None)):
        raise _lib.CapmiError('the BatchNorm state does not match the parameters (use_bn)')


def prepare(P, fc_feats, att_feats, att_masks=None, drop_fc=None, drop_att=None, ws=None, out=None, bn=None):
    """AttModel._prepare_feature (AttModel.py:114-124): MFMA GEMMs with fused bias/ReLU/dropout epilogues.  Padded regions
    (att_masks == 0) are zeroed like pad_packed_sequence does (44-49).  fc_feats None: the family has no fc_embed (Att2in2).
    out: optional (fc [B,R], att [B,K,R], p_att [B,K,A]) contiguous targets (slices of a caller's larger buffers).
    bn: the RegionBN of a use_bn model -- BatchNorm1d in front of the Linear, with use_bn 2 another behind the dropout, both over
    the valid region rows only (pack_wrapper); att_masks None counts all B * K rows."""
    _check_bn(P, bn)
    if att_masks is not None:
        max_len = clip_len(att_masks)          # clip_att, AttModel.py:106-112
        att_feats = att_feats[:, :max_len].contiguous()
        att_masks = att_masks[:, :max_len].contiguous().float()
        if drop_att is not None:
            drop_att = drop_att[:, :max_len].contiguous()
    B, K = att_feats.shape[:2]
    lin = att_linear(P)
    R = P[lin + '.weight'].shape[0]
    pr = Prepared()
    pr.K = K
    pr.bn, pr.bn1, pr.bn2, pr.att_pre, pr.bn_keep = bn, None, None, None, None
    pr.att_in, pr.drop_fc = att_feats.contiguous(), drop_fc
    o_fc, o_att, o_patt = out if out is not None else (None, None, None)
    pr.fc_in = pr.fc = None
    if fc_feats is not None:
        pr.fc_in = fc_feats.contiguous()
        pr.fc = ops.linear(pr.fc_in, P['fc_embed.0.weight'], P['fc_embed.0.bias'], relu=True, mul_mask=drop_fc, ws=ws, out=o_fc)
    att_mask_full = drop_att
    if att_masks is not None:
        m = att_masks.unsqueeze(-1).expand(B, K, R)
        att_mask_full = (m if drop_att is None else m * drop_att).contiguous()
    pr.drop_att = att_mask_full
    x2d = pr.att_in.view(B * K, -1)
    o_att2d = None if o_att is None else o_att.view(B * K, R)
    rows = None if att_masks is None else att_masks.view(B * K)
    if bn is not None:
        # BatchNorm1d(att_feat_size): the normalised rows are written once and feed the GEMM ("Batch normalization")
        pr.bn1 = ops.bn_stats(x2d, rows, bn.train, *bn.bn1)
        x2d = ops.bn_apply(x2d, rows, pr.bn1[3], pr.bn1[1], P[ATT_BN1 + '.weight'], P[ATT_BN1 + '.bias'])
    two = bn is not None and bn.bn2 is not None
    att2d = ops.linear(x2d, P[lin + '.weight'], P[lin + '.bias'], relu=True,
                       mul_mask=None if att_mask_full is None else att_mask_full.view(B * K, R), ws=ws, out=None if two else o_att2d)
    if two:
        # BatchNorm1d(rnn_size) behind ReLU / dropout; the padded rows of its output are zero (pad_packed_sequence)
        pr.att_pre = att2d
        pr.bn2 = ops.bn_stats(att2d, rows, bn.train, *bn.bn2)
        att2d = ops.bn_apply(att2d, rows, pr.bn2[3], pr.bn2[1], P[ATT_BN2 + '.weight'], P[ATT_BN2 + '.bias'], out=o_att2d)
    pr.att = att2d.view(B, K, R)
    pr.p_att = ops.linear(att2d, P['ctx2att.weight'], P['ctx2att.bias'], ws=ws,
                          out=None if o_patt is None else o_patt.view(B * K, -1)).view(B, K, -1)
    pr.att_masks = att_masks
    return pr


def relu_drop_bwd(dy, y_saved, mask):
    """dx = dy * mask * [y_saved > 0]; y_saved = relu(pre)*mask.  A unit with y_saved == 0 was either
    clipped by the ReLU (gradient 0) or dropped (mask 0 => gradient 0)."""
    return ops.relu_mask_bwd(dy.contiguous(), y_saved.contiguous(), mask)


def prepare_backward(P, pr, d_fc, d_att, d_p_att, grads, ws=None, group=True, cache_key=None):
    """Backward of prepare(): fills grads[...] for ctx2att / att_embed (/ fc_embed when the family has it) (overwrite); d_att is
    accumulated into.  The weight gradients (K = B * regions rows / B rows) go with their bias gradients as ONE grouped launch at
    the end (ops.gemm_group_tn); group=False, or a bias gradient off a 16-byte boundary: one launch each.  Returns what has to
    outlive the launches.  (In that one-launch-each fallback ctx2att's pair is issued before the d_att accumulation, as UpDown
    always did; Att2in2 used to issue it after.  The launches and their operands are the same.)"""
    B, K, R = pr.att.shape
    A = pr.p_att.shape[2]
    dp = d_p_att.view(B * K, A)
    att2d = pr.att.view(B * K, R)
    items = []

    def dw(dy, x, wname, bname):
        if group and grads[bname].data_ptr() % 16 == 0:
            items.append((dy, x, grads[wname], False, None, 0, grads[bname]))
        else:
            ops.matmul_tn(dy, x, out=grads[wname], ws=ws)
            ops.colsum(dy, out=grads[bname])
    # ctx2att: p_att = att W^T + b
    dw(dp, att2d, 'ctx2att.weight', 'ctx2att.bias')
    d_att_total = d_att.view(B * K, R)
    ops.gemm([(dp, A, P['ctx2att.weight'], R, A, 1)], B * K, R, d_att_total, a_layout=0, b_layout=1, accumulate=True, ws=ws)
    # att_embed: att = drop(relu(x W^T + b)).  relu gate: pre-activation > 0  <=>  relu output > 0; with dropout the saved output
    # may be zero for kept units only if relu clipped, and for dropped units the mask already zeroes the gradient.
    bn = getattr(pr, 'bn', None)
    lin = att_linear(P)
    rows = None if pr.att_masks is None else pr.att_masks.view(B * K)
    d_h, y_saved = d_att_total, att2d
    if bn is not None and bn.bn2 is not None:
        # the second BatchNorm: its full Jacobian over the valid rows; the ReLU gate reads the saved pre-BN activation
        mean2, rstd2, count2, _ = pr.bn2
        y_saved = pr.att_pre
        d_h = ops.bn_backward(d_att_total, y_saved, rows, mean2, rstd2, P[ATT_BN2 + '.weight'], count2, bn.train,
                              grads[ATT_BN2 + '.weight'], grads[ATT_BN2 + '.bias'], dx=d_att_total)
    d_pre = relu_drop_bwd(d_h, y_saved, None if pr.drop_att is None else pr.drop_att.view(B * K, R))
    # with use_bn the weight-gradient item still reads the RAW rows: ops.bn_linear_bwd below turns G0 = d_pre^T x into the
    # gradients of the Linear and of the BatchNorm in front of it
    dw(d_pre, pr.att_in.view(B * K, -1), lin + '.weight', lin + '.bias')
    d_pre_fc = None
    if pr.fc is not None:
        d_pre_fc = relu_drop_bwd(d_fc, pr.fc, pr.drop_fc)
        dw(d_pre_fc, pr.fc_in, 'fc_embed.0.weight', 'fc_embed.0.bias')
    if items:
        ops.gemm_group_tn(items, ws=ws, cache_key=cache_key)
    if bn is not None:
        pr.bn_keep = ops.bn_linear_bwd(grads[lin + '.weight'], grads[lin + '.bias'], P[lin + '.weight'], pr.bn1[0], pr.bn1[1],
                                 P[ATT_BN1 + '.weight'], P[ATT_BN1 + '.bias'], grads[ATT_BN1 + '.weight'], grads[ATT_BN1 + '.bias'])
    return d_pre, d_pre_fc, dp


class RolloutBase:
    """Device buffers + one native call for a T-step rollout of N caption rows.  A family sets the class attributes, builds its
    capmi_*_rollout struct (dims, features, masks, its own fields) and its activation buffers in __init__, hands both to _bind(),
    and fills its weights struct; its backward() allocates scratch and feature gradients and goes through _bwd_structs()."""

    SCRATCH = GRADS = None                    # ctypes types of capmi_*_bwd_scratch / capmi_*_grads
    G_FIELDS = ()                             # (capmi_*_grads field, parameter name): gradients written in place
    FWD = BWD = None                          # native entry points, by name
    SELECT_BUFS = ('it_all', 'seq', 'seq_logp', 'sel_logp', 'live', 'it', 'unfinished')
    TRACE = 'alpha'                           # the activation that holds the per-step region weights [T, N, K] (att_trace.py)

    def _bind(self, r, acts, dev, N, T, L, V1, mode, temperature=1.0, gumbel=None, seed=0, forced=None, teacher=False,
              ss_mode=None, raw=False, ws=None, always_zero=False):
        """Allocate the select-side buffers, set the fields every capmi_*_rollout has, point r at the buffers.
        acts: name -> activation tensor (or None) by struct field name; they become attributes.
        ss_mode (uint8 [T,N], teacher only): scheduled sampling, 1 = the input of (step, row) is drawn from the previous step's
        distribution, 2 = teacher-forced.  raw (free-running): the stored rows are the logits (CAPMI_SELECT_RAW)."""
        self.ws = ws or ops.default_workspace(dev)
        self.it_all = torch.empty(T, N, dtype=torch.long, device=dev)
        # the select kernel writes every (row, step < T) slot of seq / seq_logp / sel_logp / live, zeros included (and the UpDown
        # driver clears the tail behind an early exit): fills -- a 45 MB memset of the dense log-probs at the flagship size -- are
        # only needed when fewer steps than the pitch are run (XE with an early all-pad column)
        zl = torch.zeros if (always_zero or T != L) else torch.empty
        self.seq = zl(N, L, dtype=torch.long, device=dev)
        self.seq_logp = zl(N, L, V1, dtype=_f32, device=dev)
        self.sel_logp = zl(N, L, dtype=_f32, device=dev)
        self.live = zl(N, L, dtype=torch.uint8, device=dev)
        self.it = torch.empty(N, dtype=torch.long, device=dev)
        self.unfinished = torch.empty(N, dtype=torch.uint8, device=dev)
        self.gumbel, self.forced, self.ss_mode = gumbel, forced, ss_mode
        self.__dict__.update(acts)
        if ss_mode is not None:
            assert teacher and ss_mode.dtype == torch.uint8 and ss_mode.shape == (T, N) and ss_mode.is_contiguous()
        r.mode = MODES[mode] | (_lib.SELECT_RAW if (raw and not teacher) else 0)
        r.temperature, r.gumbel, r.seed = float(temperature), ptr(gumbel), int(seed) & 0xFFFFFFFFFFFFFFFF
        if forced is not None:
            assert forced.dtype == torch.long and forced.is_contiguous()
            r.forced, r.forced_ld = ptr(forced), forced.shape[1]
        r.teacher, r.ss_mode = int(teacher), ptr(ss_mode)
        for k in acts:
            setattr(r, k, ptr(acts[k]))
        for k in self.SELECT_BUFS:
            setattr(r, k, getattr(self, k).data_ptr())
        r.partial, r.partial_capacity = self.ws.buf.data_ptr(), self.ws.capacity
        self.r = r

    def run(self):
        check(getattr(lib, self.FWD)(C.byref(self.w), C.byref(self.r), stream_ptr()), self.FWD)
        return self.seq, self.seq_logp

    def _bwd_structs(self, keep, outs, grads, g_seq_logp, sparse):
        """keep: scratch tensors by capmi_*_bwd_scratch field; outs: feature-gradient tensors by capmi_*_grads field; grads: name ->
        preallocated fp32 tensor (overwritten) for every parameter; sparse: the loss gradient as a _lib.SparseLogpGrad
        (sparse_logp.split_grad), g_seq_logp [N,L,V1] is None then.  -> (scratch struct, grads struct, contiguous g_seq_logp)"""
        s = self.SCRATCH()
        for k, t in keep.items():
            setattr(s, k, t.data_ptr())
        s.partial, s.partial_capacity = self.ws.buf.data_ptr(), self.ws.capacity
        if sparse is not None:
            s.sparse = C.pointer(sparse)
        g = fill_struct(self.GRADS(), self.G_FIELDS, grads, validate=False)
        for k, t in outs.items():
            setattr(g, k, t.data_ptr())
        return s, g, None if g_seq_logp is None else g_seq_logp.contiguous()

    def _bwd(self, keep, outs, grads, g_seq_logp, sparse):
        """the whole BPTT as one native call; -> what has to stay alive until the stream has consumed it"""
        s, g, g_seq_logp = self._bwd_structs(keep, outs, grads, g_seq_logp, sparse)
        check(getattr(lib, self.BWD)(C.byref(self.w), C.byref(self.r), ptr(g_seq_logp), C.byref(s), C.byref(g), stream_ptr()),
              self.BWD)
        return keep, outs, g_seq_logp
