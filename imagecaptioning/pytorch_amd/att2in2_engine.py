"""Host-side driver of the Att2in2 decoder (configs/a2i2*.yml) on libcapmi: buffers + one native call per rollout.

  prepare()            AttModel._prepare_feature (AttModel.py:114-124) without fc_embed (Att2in2Model, :854-859)
  Rollout.run()        AttModel._sample / _forward over Att2in2Core (:750-790)
  Rollout.backward()   the BPTT torch would have recorded for them
  prepare_backward()   att_embed / ctx2att gradients
"""
import torch

from . import _lib, engine_common
from ._lib import ptr
from .engine_common import RolloutBase, fill_struct

_f32 = torch.float32
_W = (('embed', 'embed.0.weight'), ('i2h_w', 'core.i2h.weight'), ('i2h_b', 'core.i2h.bias'), ('h2h_w', 'core.h2h.weight'),
      ('h2h_b', 'core.h2h.bias'), ('a2c_w', 'core.a2c.weight'), ('a2c_b', 'core.a2c.bias'),
      ('h2att_w', 'core.attention.h2att.weight'), ('h2att_b', 'core.attention.h2att.bias'),
      ('alpha_w', 'core.attention.alpha_net.weight'), ('alpha_b', 'core.attention.alpha_net.bias'), ('logit_w', 'logit.weight'),
      ('logit_b', 'logit.bias'))


def weights_struct(P):
    return fill_struct(_lib.Att2in2Weights(), _W, P)


def prepare(P, att_feats, att_masks=None, drop_att=None, ws=None, bn=None):
    """att' = drop(relu(att_embed(att))) with padded regions zeroed (pack_wrapper, AttModel.py:44-49), p_att = ctx2att(att').
    drop_att: [B,K,R] keep mask of the att_embed dropout (train mode) or None.  bn: engine_common.RegionBN of a use_bn model."""
    return engine_common.prepare(P, None, att_feats, att_masks, None, drop_att, ws=ws, bn=bn)


def prepare_backward(P, pr, d_att, d_p_att, grads, ws=None):
    """Backward of prepare(): fills grads[...] for att_embed / ctx2att (overwrite).  d_att is accumulated into."""
    return engine_common.prepare_backward(P, pr, None, d_att, d_p_att, grads, ws=ws)


class Rollout(RolloutBase):
    """Device buffers + one native call for a T-step rollout of N = B*n caption rows."""

    SCRATCH, GRADS, G_FIELDS = _lib.Att2in2BwdScratch, _lib.Att2in2Grads, _W
    FWD, BWD = 'capmi_att2in2_rollout_fwd', 'capmi_att2in2_rollout_bwd'

    def __init__(self, P, pr, n, T, L=None, mode='greedy', temperature=1.0, drop_xt=None, drop_out=None, gumbel=None, seed=0,
                 forced=None, teacher=False, ss_mode=None, raw=False, ws=None):
        """ss_mode, raw: RolloutBase._bind"""
        dev = pr.att.device
        B, K, R = pr.att.shape
        A = pr.p_att.shape[2]
        V1, E = P['embed.0.weight'].shape
        N = B * n
        L = T if L is None else L
        self.P, self.pr, self.dims = P, pr, (B, n, N, K, A, R, E, V1, T, L)
        self.drop_xt, self.drop_out = drop_xt, drop_out
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        r = _lib.Att2in2Rollout()
        r.B, r.n, r.N, r.K, r.A, r.R, r.E, r.V1, r.T, r.L = B, n, N, K, A, R, E, V1, T, L
        r.att, r.p_att, r.att_mask = ptr(pr.att), ptr(pr.p_att), ptr(pr.att_masks)
        r.drop_xt, r.drop_out = ptr(drop_xt), ptr(drop_out)
        acts = dict(h=z(T + 1, N, R), c=z(T + 1, N, R), x=z(T, N, E), saved=z(T, N, 5 * R), h_drop=z(T, N, R), att_h=z(T, N, A),
                    alpha=z(T, N, K), ctx=z(T, N, R), xin=z(T, N, 5 * R) if (teacher and ss_mode is None) else None)
        self._bind(r, acts, dev, N, T, L, V1, mode, temperature, gumbel, seed, forced, teacher, ss_mode, raw, ws)
        self.w = weights_struct(P)

    def backward(self, g_seq_logp, grads, sparse=None):
        """g_seq_logp, grads, sparse: RolloutBase._bwd_structs; grads includes the prefill's att_embed / ctx2att."""
        B, n, N, K, A, R, E, V1, T, L = self.dims
        dev = self.seq.device
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        keep = dict(dlogits=z(T, N, V1), d_hdrop=z(T, N, R), d_sums=z(T, N, 5 * R), d_ctx=z(T, N, R), d_att_h=z(T, N, A),
                    d_e=z(T, N, K), dc=z(2, N, R), d_x=z(T, N, E))
        outs = dict(d_att=z(B, K, R), d_p_att=z(B, K, A))
        kept = self._bwd(keep, outs, grads, g_seq_logp, sparse)
        kp = prepare_backward(self.P, self.pr, outs['d_att'], outs['d_p_att'], grads, ws=self.ws)
        self._keep = (kept, kp)     # scratch alive until the stream has consumed it
