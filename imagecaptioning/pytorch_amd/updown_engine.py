"""Host-side driver of the UpDown decode path on libcapmi (MI355X).

Python here only owns device memory (torch tensors), fills the C structs of include/capmi.h and makes
ONE native call per rollout (forward) / per BPTT (backward); all arithmetic is in the HIP kernels.

Mirrors, for the UpDown model (AttModel.py:875-879 + UpDownCore 615-640):
  prepare()      AttModel._prepare_feature        AttModel.py:114-124
  Rollout.run()  AttModel._sample / _forward      AttModel.py:258-352 / 126-164
  Rollout.backward()  the autograd graph torch would have recorded for them
"""
import ctypes as C
import os

import torch

from . import _lib, ops, engine_common
from ._lib import lib, ptr, check, stream_ptr
from .engine_common import Prepared, RegionBN, RolloutBase, fill_struct, prepare          # noqa: F401  (Prepared, RegionBN, prepare: this module's API)

_f32 = torch.float32

PARAM_KEYS = ('embed.0.weight', 'fc_embed.0.weight', 'fc_embed.0.bias', 'att_embed.0.weight', 'att_embed.0.bias',
              'ctx2att.weight', 'ctx2att.bias', 'core.att_lstm.weight_ih', 'core.att_lstm.weight_hh',
              'core.att_lstm.bias_ih', 'core.att_lstm.bias_hh', 'core.lang_lstm.weight_ih', 'core.lang_lstm.weight_hh',
              'core.lang_lstm.bias_ih', 'core.lang_lstm.bias_hh', 'core.attention.h2att.weight',
              'core.attention.h2att.bias', 'core.attention.alpha_net.weight', 'core.attention.alpha_net.bias',
              'logit.weight', 'logit.bias')


_W_FIELDS = (('embed', 'embed.0.weight'), ('att_w_ih', 'core.att_lstm.weight_ih'), ('att_w_hh', 'core.att_lstm.weight_hh'),
             ('att_b_ih', 'core.att_lstm.bias_ih'), ('att_b_hh', 'core.att_lstm.bias_hh'),
             ('lang_w_ih', 'core.lang_lstm.weight_ih'), ('lang_w_hh', 'core.lang_lstm.weight_hh'),
             ('lang_b_ih', 'core.lang_lstm.bias_ih'), ('lang_b_hh', 'core.lang_lstm.bias_hh'),
             ('h2att_w', 'core.attention.h2att.weight'), ('h2att_b', 'core.attention.h2att.bias'),
             ('alpha_w', 'core.attention.alpha_net.weight'), ('alpha_b', 'core.attention.alpha_net.bias'),
             ('logit_w', 'logit.weight'), ('logit_b', 'logit.bias'))


def weights_struct(P):
    return fill_struct(_lib.UpDownWeights(), _W_FIELDS, P)


def prepare_backward(P, pr, d_fc, d_att, d_p_att, grads, ws=None):
    """Backward of prepare(): fills grads[...] for fc_embed / att_embed / ctx2att (overwrite).  The three weight gradients with
    their bias gradients are ONE grouped launch (144 tiles of one round instead of three sub-wave GEMMs + reductions + three
    column sums); CAPMI_PREP_GROUP=0: one launch each"""
    engine_common.prepare_backward(P, pr, d_fc, d_att, d_p_att, grads, ws=ws, group=os.environ.get('CAPMI_PREP_GROUP', '1') != '0',
                                   cache_key=('updown_prepare', str(d_p_att.device)))


_alive = {}


def _alive_buffer(dev, L):
    """[L] int32 of pinned host memory the select kernels can write (capmi.h capmi_updown_rollout.alive_host), one per stream:
    the words are only ever SET by kernels and cleared by the host before a rollout is enqueued, so a late store of the
    previous rollout can at worst postpone an early exit."""
    key = (str(dev), stream_ptr(), L)
    t = _alive.get(key)
    if t is None:
        t = _alive[key] = torch.zeros(max(L, 32), dtype=torch.int32).pin_memory()
    return t


class Rollout(RolloutBase):
    """Device buffers + one native call for a T-step rollout of N = B*n caption rows."""

    SCRATCH, GRADS, G_FIELDS = _lib.UpDownBwdScratch, _lib.UpDownGrads, _W_FIELDS
    FWD = 'capmi_updown_rollout_fwd'

    def __init__(self, P, pr, n, T, L=None, mode='greedy', temperature=1.0, drop_xt=None, drop_out=None,
                 gumbel=None, seed=0, forced=None, teacher=False, row_mode=None, ws=None, keep_for_backward=True,
                 row_img=None, B_grad=None, top_k=0, top_p=0.0, ss_mode=None, early_exit=None, early_exit_from=4, raw=False,
                 raw_logits=False):
        """ss_mode, raw: RolloutBase._bind (raw_logits: the older spelling of raw).
        row_img (int32 [N]) + B_grad: ragged grouping for the fused SCST rollout -- the first B_grad
        feature images own rows b*n..b*n+n-1 (sampled, with gradient), the remaining rows (greedy baseline)
        point at further feature images through row_img."""
        dev = pr.fc.device
        B_feat, K, R = pr.att.shape
        A = pr.p_att.shape[2]
        V1, E = P['embed.0.weight'].shape
        B = B_feat if B_grad is None else B_grad
        N = B * n if row_img is None else row_img.shape[0]
        self.row_img = row_img
        L = T if L is None else L
        self.P, self.pr, self.dims = P, pr, (B, n, N, K, A, R, E, V1, T, L)
        self.drop_xt, self.drop_out, self.row_mode = drop_xt, drop_out, row_mode
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)       # noqa: E731
        r = _lib.UpDownRollout()
        r.B, r.n, r.N, r.K, r.A, r.R, r.E, r.V1, r.T, r.L = B, n, N, K, A, R, E, V1, T, L
        r.B_feat, r.row_img = B_feat, ptr(row_img)
        r.fc, r.att, r.p_att, r.att_mask = ptr(pr.fc), ptr(pr.att), ptr(pr.p_att), ptr(pr.att_masks)
        r.drop_xt, r.drop_out, r.row_mode = ptr(drop_xt), ptr(drop_out), ptr(row_mode)
        r.top_k, r.top_p = int(top_k), float(top_p)
        acts = dict(h_att=z(T + 1, N, R), c_att=z(T + 1, N, R), h_lang=z(T + 1, N, R), c_lang=z(T + 1, N, R), xt=z(T, N, E),
                    gates_att=z(T, N, 4 * R), gates_lang=z(T, N, 4 * R), att_h=z(T, N, A), alpha=z(T, N, K), ctx=z(T, N, R),
                    h_drop=z(T, N, R), fc_gates=z(B_feat, 4 * R), logits=z(N, V1))
        self._bind(r, acts, dev, N, T, L, V1, mode, temperature, gumbel, seed, forced, teacher, ss_mode, ws=ws)
        # AttModel._sample(output_logsoftmax=0): logits, not log-probs -- a field of its own here, not CAPMI_SELECT_RAW in `mode`
        r.raw_logits = int(bool(raw or raw_logits) and not teacher)
        if N <= 64 and os.environ.get('CAPMI_PLANES', '1') != '0':
            # decode GEMMs stage their activations as producer-written bf16x3 planes (capmi.h capmi_updown_rollout.planes);
            # the scratch is zero-filled once and shared by the rollouts of this stream with the same R / E
            nb = int(lib.capmi_updown_planes_bytes(R, E))
            self.planes = ops.planes_scratch(dev, ('updown_fwd', R, E), nb)
            r.planes, r.planes_bytes = self.planes.data_ptr(), nb
            if not teacher and os.environ.get('CAPMI_FUSED_SELECT', '1') != '0':
                # r4: slab workspace of the part of the next step's attention-LSTM gate GEMM that is computed inside the select
                # launch (capmi.h capmi_updown_rollout.pre_partial): [ticket words | up to 8 K-slice slabs of N x 4R]
                per = ops.Workspace.COUNTER_FLOATS + 8 * 64 * 4 * R
                self.pre = ops.planes_scratch(dev, ('updown_pre', R), per * 4).view(torch.float32)
                r.pre_partial, r.pre_capacity = self.pre.data_ptr(), per
        # early exit of free-running rollouts (AttModel.py:349-350): behind steps early_exit_from + k * early_exit - 1 (7, 11, 15 by
        # default) the driver looks, two steps later, at a pinned word the select kernels set and stops enqueuing once every row
        # has emitted its EOS (CAPMI_EARLY_EXIT=0: never)
        if early_exit is None:
            early_exit = int(os.environ.get('CAPMI_EARLY_EXIT', '4'))
        self.steps_run = T
        if early_exit > 0 and not teacher and mode != 'forced' and T >= 12:
            self.alive = _alive_buffer(dev, L)
            r.early_exit, r.early_exit_from, r.alive_host = int(early_exit), int(early_exit_from), self.alive.data_ptr()
        self.T_cfg = int(r.T)
        self.w = weights_struct(P)

    def run(self):
        self.r.T = self.T_cfg                # (a previous run on this object may have ended early: every run starts from the configured T)
        out = super().run()
        self.steps_run = int(self.r.steps_run)
        self.r.T = self.steps_run            # the backward runs over the steps that were enqueued
        return out

    # backward phases in launch order with the parameter gradients each one completes (capmi.h CAPMI_BWD_*)
    BWD_PHASES = ((1, ('logit.weight', 'logit.bias')),
                  (2, ()),
                  (4, ('core.lang_lstm.weight_ih', 'core.lang_lstm.weight_hh', 'core.lang_lstm.bias_ih',
                       'core.lang_lstm.bias_hh')),
                  (8, ('core.att_lstm.weight_ih', 'core.att_lstm.weight_hh', 'core.att_lstm.bias_ih',
                       'core.att_lstm.bias_hh', 'embed.0.weight')),
                  (16, ('core.attention.h2att.weight', 'core.attention.h2att.bias', 'core.attention.alpha_net.weight',
                        'core.attention.alpha_net.bias')))

    def backward(self, g_seq_logp, grads, on_ready=None, sparse=None):
        """g_seq_logp, grads, sparse: RolloutBase._bwd_structs (grads: every PARAM_KEYS entry).  Returns (d_fc, d_att, d_p_att),
        consumed by prepare_backward.
        on_ready(names): called after the launches that complete the gradients `names` have been enqueued, so a
        data-parallel trainer can start reducing that bucket while the later phases still run."""
        B, n, N, K, A, R, E, V1, T, L = self.dims
        dev = self.seq.device
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)       # noqa: E731
        keep = dict(dlogits=z(T, N, V1), d_hdrop=z(T, N, R), dg_att=z(T, N, 4 * R), dg_lang=z(T, N, 4 * R),
                    d_x2=z(T, N, 3 * R), d_e_all=z(T, N, K), d_att_h_all=z(T, N, A), dh_att_attn=z(N, R),
                    d_x1=z(4), dc_att=z(2, N, R), dc_lang=z(2, N, R), d_xt_all=z(T, N, E),
                    sum_dg_att=z(B, 4 * R), w_lang_cat=z(4 * R, 3 * R), w_att_cat=z(4 * R, 2 * R))
        outs = dict(d_fc=z(B, R), d_att=z(B, K, R), d_p_att=z(B, K, A))
        s, g, g_seq_logp = self._bwd_structs(keep, outs, grads, g_seq_logp, sparse)
        if self.row_img is not None and B * n < N and os.environ.get('CAPMI_BWD_ALL_ROWS') != '1':
            # fused SCST rollout: rows [B*n, N) are the greedy baseline (eval mode, no gradient) -- the backward runs on the
            # sampled rows only and packs the saved activations once for its time-batched GEMMs
            nb = B * n
            keep['pack'] = z(nb * (T * (4 * R + 2 * E + 2 + A + K) + R) + 64)
            s.n_grad_rows, s.pack, s.pack_capacity = nb, keep['pack'].data_ptr(), keep['pack'].numel()
        if (s.n_grad_rows or N) <= 64 and os.environ.get('CAPMI_PLANES', '1') != '0':
            nb = int(lib.capmi_updown_bwd_planes_bytes(R))
            keep['planes'] = ops.planes_scratch(dev, ('updown_bwd', R), nb)
            s.planes, s.planes_bytes = keep['planes'].data_ptr(), nb
        if on_ready is None:
            check(lib.capmi_updown_rollout_bwd(C.byref(self.w), C.byref(self.r), ptr(g_seq_logp), C.byref(s), C.byref(g),
                                               stream_ptr()), 'capmi_updown_rollout_bwd')
        else:
            for mask, names in self.BWD_PHASES:
                check(lib.capmi_updown_rollout_bwd_phases(C.byref(self.w), C.byref(self.r), ptr(g_seq_logp), C.byref(s),
                                                          C.byref(g), mask, stream_ptr()), 'capmi_updown_rollout_bwd_phases')
                if names:
                    on_ready(names)
        self._bwd_keep = keep     # keep scratch alive until the stream has consumed it
        return outs['d_fc'], outs['d_att'], outs['d_p_att']
