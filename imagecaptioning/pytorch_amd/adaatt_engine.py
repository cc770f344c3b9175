"""Host-side driver of the AdaAtt decoder (caption_model adaatt / adaattmo) on libcapmi: buffers + one native call per rollout.

  prepare()            AttModel._prepare_feature (AttModel.py:114-124: fc_embed, att_embed, ctx2att) + the step-independent
                       (v2h | r_v2h)(fc) product of AdaAtt_lstm (:492, :521) with all six gate biases folded in
  Rollout.run()        AttModel._sample / _forward over AdaAttCore (:604-613)
  Rollout.backward()   the BPTT torch would have recorded for them
  prepare_backward()   v2h / r_v2h / gate-bias / fc_embed / att_embed / ctx2att gradients
"""
import torch

from . import _lib, ops, updown_engine
from ._lib import ptr
from .engine_common import RolloutBase, fill_struct

_f32 = torch.float32
_L, _A = 'core.lstm.', 'core.attention.'
# capmi_adaatt_weights fields that are parameters as they stand (xw / hw are packed, see packed())
_W = (('embed', 'embed.0.weight'), ('fr_w', _A + 'fr_linear.0.weight'), ('fr_b', _A + 'fr_linear.0.bias'),
      ('ho_w', _A + 'ho_linear.0.weight'), ('ho_b', _A + 'ho_linear.0.bias'), ('fre_w', _A + 'fr_embed.weight'),
      ('fre_b', _A + 'fr_embed.bias'), ('hoe_w', _A + 'ho_embed.weight'), ('hoe_b', _A + 'ho_embed.bias'),
      ('alpha_w', _A + 'alpha_net.weight'), ('alpha_b', _A + 'alpha_net.bias'), ('att2h_w', _A + 'att2h.weight'),
      ('att2h_b', _A + 'att2h.bias'), ('logit_w', 'logit.weight'), ('logit_b', 'logit.bias'))
# capmi_adaatt_grads fields written straight into a parameter's gradient
_G = _W + (('w2h_w', _L + 'w2h.weight'), ('r_w2h_w', _L + 'r_w2h.weight'), ('h2h_w', _L + 'h2h.0.weight'),
           ('r_h2h_w', _L + 'r_h2h.weight'))
_GATE = ('w2h', 'v2h', 'h2h.0')          # the three Linear layers behind the gate columns; 'r_' + name.split('.')[0]: the sentinel's


def packed(P):
    """(xw [G+R,E], hw [G+R,R], vw [G+R,R], gate_b [G+R]): the gate and sentinel-gate layers stacked by rows, so each operand is
    one GEMM; the biases of all six layers summed.  Rebuilt per rollout / stepper (3 small copies and a sum): the fused optimizer
    updates parameters through raw pointers, so a tensor version cannot vouch for a cached copy."""
    for n in _GATE:
        for k in (_L + n + '.weight', _L + 'r_' + n.split('.')[0] + '.weight'):
            if not (P[k].is_cuda and P[k].dtype == _f32):
                raise _lib.CapmiError('parameter %s must be a fp32 device tensor' % k)
    cat = lambda a, b: torch.cat([P[_L + a], P[_L + b]], 0).contiguous()          # noqa: E731
    gate_b = torch.cat([P[_L + 'w2h.bias'] + P[_L + 'v2h.bias'] + P[_L + 'h2h.0.bias'],
                        P[_L + 'r_w2h.bias'] + P[_L + 'r_v2h.bias'] + P[_L + 'r_h2h.bias']]).contiguous()
    return cat('w2h.weight', 'r_w2h.weight'), cat('h2h.0.weight', 'r_h2h.weight'), cat('v2h.weight', 'r_v2h.weight'), gate_b


def weights_struct(P, packs=None):
    w = fill_struct(_lib.AdaAttWeights(), _W, P)
    xw, hw, _, _ = packs or packed(P)
    w.xw, w.hw = xw.data_ptr(), hw.data_ptr()
    w._keep = (xw, hw)
    return w


class Prepared:
    """updown_engine.Prepared (fc', att', p_att, masks) + fc_gates [B,G+R]."""

    def __init__(self, pr, fc_gates, packs):
        self.pr, self.fc_gates, self.packs = pr, fc_gates, packs
        self.fc, self.att, self.p_att, self.att_masks, self.K = pr.fc, pr.att, pr.p_att, pr.att_masks, pr.K


def from_features(P, pr, ws=None):
    """Prepared for features that are already embedded (pr.fc, pr.att, pr.p_att, pr.att_masks)"""
    packs = packed(P)
    return Prepared(pr, ops.linear(pr.fc, packs[2], packs[3], ws=ws), packs)


def prepare(P, fc_feats, att_feats, att_masks=None, drop_fc=None, drop_att=None, ws=None):
    pr = updown_engine.prepare(P, fc_feats, att_feats, att_masks, drop_fc, drop_att, ws=ws)
    return from_features(P, pr, ws)


def prepare_backward(P, ap, d_fc_gates, gate_b, d_att, d_p_att, grads, ws=None):
    """Backward of prepare(): v2h / r_v2h weights, the six gate biases, then fc_embed / att_embed / ctx2att (overwrite)."""
    pr = ap.pr
    vw = ap.packs[2]
    W, R = vw.shape
    G = W - R
    dvw = ops.matmul_tn(d_fc_gates, pr.fc, ws=ws)                  # [G+R, R]
    grads[_L + 'v2h.weight'].copy_(dvw[:G])
    grads[_L + 'r_v2h.weight'].copy_(dvw[G:])
    for n in _GATE:
        grads[_L + n + '.bias'].copy_(gate_b[:G])
        grads[_L + 'r_' + n.split('.')[0] + '.bias'].copy_(gate_b[G:])
    d_fc = torch.empty_like(pr.fc)
    ops.gemm([(d_fc_gates, W, vw, R, W, 1)], d_fc.shape[0], R, d_fc, a_layout=0, b_layout=1, ws=ws)
    updown_engine.prepare_backward(P, pr, d_fc, d_att, d_p_att, grads, ws=ws)
    return dvw, d_fc


class Rollout(RolloutBase):
    """Device buffers + one native call for a T-step rollout of N = B*n caption rows."""

    SCRATCH, GRADS, G_FIELDS = _lib.AdaAttBwdScratch, _lib.AdaAttGrads, _G
    FWD, BWD = 'capmi_adaatt_rollout_fwd', 'capmi_adaatt_rollout_bwd'
    TRACE = 'pi'                               # [T, N, K + 1]: sentinel, then the regions
    DROPS = ('drop_xt', 'drop_h', 'drop_fake', 'drop_fr', 'drop_ho', 'drop_out', 'drop_tile')

    def __init__(self, P, ap, n, T, L=None, mode='greedy', temperature=1.0, gumbel=None, seed=0, forced=None, teacher=False,
                 ss_mode=None, raw=False, tile_p=0.0, tile_seed=0, ws=None, **drops):
        """drops: keep masks by capmi_adaatt_rollout field name (drop_xt [T,N,E] ... drop_tile [T,N,K+1,A]); without drop_tile,
        tile_p > 0 draws the tanh-tile mask inside the kernels from (tile_seed, step, row, score row, column).
        ss_mode, raw: RolloutBase._bind."""
        dev = ap.att.device
        B, K, R = ap.att.shape
        A = ap.p_att.shape[2]
        V1, E = P['embed.0.weight'].shape
        W = P[_L + 'w2h.weight'].shape[0] + R
        N = B * n
        L = T if L is None else L
        assert set(drops) <= set(self.DROPS), sorted(drops)
        self.P, self.ap, self.dims, self.drops = P, ap, (B, n, N, K, A, R, E, V1, T, L, W), drops
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        r = _lib.AdaAttRollout()
        r.B, r.n, r.N, r.K, r.A, r.R, r.E, r.V1, r.T, r.L, r.maxout = B, n, N, K, A, R, E, V1, T, L, int(W == 6 * R)
        r.fc_gates, r.att, r.p_att, r.att_mask = ptr(ap.fc_gates), ptr(ap.att), ptr(ap.p_att), ptr(ap.att_masks)
        shapes = dict(drop_xt=(T, N, E), drop_h=(T, N, R), drop_fake=(T, N, R), drop_fr=(T, N, E), drop_ho=(T, N, E),
                      drop_out=(T, N, R), drop_tile=(T, N, K + 1, A))
        for k, m in drops.items():
            if m is not None:
                assert m.shape == shapes[k] and m.is_contiguous() and m.dtype == _f32, (k, tuple(m.shape), shapes[k])
            setattr(r, k, ptr(m))
        r.tile_p, r.tile_seed = (0.0 if drops.get('drop_tile') is not None else float(tile_p)), int(tile_seed) & 0xFFFFFFFFFFFFFFFF
        acts = dict(h=z(T + 1, N, R), c=z(T + 1, N, R), x=z(T, N, E), saved=z(T, N, W), h_drop=z(T, N, R), fake_drop=z(T, N, R),
                    ctx=z(T, N, R), out_t=z(T, N, R), out_drop=z(T, N, R), fr=z(T, N, E), ho_t=z(T, N, E), ho=z(T, N, E),
                    fr_e=z(T, N, A), ho_e=z(T, N, A), pi=z(T, N, K + 1), xin=z(T, N, W) if (teacher and ss_mode is None) else None)
        self._bind(r, acts, dev, N, T, L, V1, mode, temperature, gumbel, seed, forced, teacher, ss_mode, raw, ws)
        self.w = weights_struct(P, ap.packs)

    def backward(self, g_seq_logp, grads, sparse=None):
        """g_seq_logp, grads, sparse: RolloutBase._bwd_structs; grads includes the prefill's parameters."""
        B, n, N, K, A, R, E, V1, T, L, W = self.dims
        dev = self.seq.device
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)          # noqa: E731
        keep = dict(dlogits=z(T, N, V1), d_out=z(T, N, R), d_ctx=z(T, N, R), d_e=z(T, N, K + 1), d_hoe=z(T, N, A), d_fre=z(T, N, A),
                    d_fr=z(T, N, E), d_ho=z(T, N, E), d_hdrop=z(T, N, R), d_fakedrop=z(T, N, R), d_sums=z(T, N, W), dc=z(2, N, R),
                    d_x=z(T, N, E))
        o = dict(gate_b=z(W), d_fc_gates=z(B, W), d_att=z(B, K, R), d_p_att=z(B, K, A))
        kept = self._bwd(keep, o, grads, g_seq_logp, sparse)
        kp = prepare_backward(self.P, self.ap, o['d_fc_gates'], o['gate_b'], o['d_att'], o['d_p_att'], grads, ws=self.ws)
        self._keep = (kept, kp)     # scratch alive until the stream has consumed it
