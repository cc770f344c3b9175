"""Host-side driver of the NewFC decoder (configs/fc.yml) on libcapmi: buffers + one native call per rollout."""
import torch

from . import _lib, ops
from ._lib import ptr
from .engine_common import RolloutBase, fill_struct

_f32 = torch.float32
_W = (('embed', 'embed.weight'), ('i2h_w', '_core.i2h.weight'), ('i2h_b', '_core.i2h.bias'), ('h2h_w', '_core.h2h.weight'),
      ('h2h_b', '_core.h2h.bias'), ('logit_w', 'logit.weight'), ('logit_b', 'logit.bias'))


class Rollout(RolloutBase):
    SCRATCH, GRADS, G_FIELDS = _lib.NewFCBwdScratch, _lib.NewFCGrads, _W
    FWD, BWD = 'capmi_newfc_rollout_fwd', 'capmi_newfc_rollout_bwd'

    def __init__(self, P, fc_feats, n, T, L=None, mode='greedy', temperature=1.0, drop_out=None, gumbel=None, seed=0,
                 forced=None, teacher=False, ws=None, raw=False, ss_mode=None):
        """ss_mode, raw: RolloutBase._bind (raw, r5: AttModel._sample(output_logsoftmax=0), AttModel.py:171-175, 265; the backward
        then takes the loss gradient as d(logits))"""
        dev = fc_feats.device
        B = fc_feats.shape[0]
        V1, E = P['embed.weight'].shape
        R = P['_core.h2h.weight'].shape[1]
        N = B * n
        L = T if L is None else L
        self.P, self.dims, self.fc_in, self.drop_out = P, (B, n, N, R, E, V1, T, L), fc_feats, drop_out
        ws = ws or ops.default_workspace(dev)
        self.w = fill_struct(_lib.NewFCWeights(), _W, P)
        # fc_embed is a plain Linear (AttModel.py:907)
        self.fc_emb = ops.linear(fc_feats, P['fc_embed.weight'], P['fc_embed.bias'], ws=ws)
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        r = _lib.NewFCRollout()
        r.B, r.n, r.N, r.R, r.E, r.V1, r.T, r.L = B, n, N, R, E, V1, T, L
        r.fc_emb, r.drop_out = ptr(self.fc_emb), ptr(drop_out)
        # the image step comes first: one more slot of h / c / saved than the attention families have
        acts = dict(h=z(T + 2, N, R), c=z(T + 2, N, R), x=z(T, N, E), saved=z(T + 1, N, 5 * R), h_drop=z(T, N, R), logits=z(N, V1))
        self._bind(r, acts, dev, N, T, L, V1, mode, temperature, gumbel, seed, forced, teacher, ss_mode, raw, ws, always_zero=True)

    def backward(self, g_seq_logp, grads, sparse=None):
        B, n, N, R, E, V1, T, L = self.dims
        dev = self.seq.device
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        keep = dict(dlogits=z(T, N, V1), d_hdrop=z(T, N, R), d_sums=z(T + 1, N, 5 * R), dh_prev=z(2, N, R), dc=z(2, N, R),
                    d_x_all=z(max(T * N * E, B * 5 * R)), d_ximg=z(N, E))
        d_fc_emb = z(B, E)
        self._keep = self._bwd(keep, dict(d_fc_emb=d_fc_emb), grads, g_seq_logp, sparse)
        # fc_embed (plain Linear) backward
        ops.matmul_tn(d_fc_emb, self.fc_in, out=grads['fc_embed.weight'], ws=self.ws)
        ops.colsum(d_fc_emb, out=grads['fc_embed.bias'])
