"""Single-step decoders ("steppers") for the LSTM families, and the reference's step API on top of them.

A stepper holds the recurrent state of ``B * rows_per_image_max`` hypotheses (image-major rows) and exposes

    step(t, it, rows_per_image) -> logits [B*rows_per_image, V1]      # AttModel.get_logprobs_state up to the logits
    reorder(parent [B,bd] int32, cur)                                 # beam search: row b*cur+parent[b,j] -> b*bd+j
    hidden(rows) -> [rows, R] view, no copy                           # the rows the logit of the last step read (contrastive search)
    snapshot() / restore(s)                                           # (scheduled host loops that fork the state)

which is the protocol the Transformer ``Decoder`` and the AoA ``BeamDecoder`` already implement; the host-stepped
samplers of ``decode.py`` / ``beam.py`` (constrained decoding, diverse sampling, diverse beam search) drive any of them.
A model hands them out through one factory, ``model._decode_stepper(fc_feats, att_feats, att_masks, L)`` -> ``make(rows_per_image)``:
the features are prepared once when the factory is made and shared by every stepper it makes.  ``CaptionModel._sample`` builds no
other; AttEnsemble, score.py and disc.py call the same one.
The fast paths (one native call per rollout / per beam search) do not go through here.

  UpDownStepper   capmi_updown_decode_step  (UpDownCore.forward, AttModel.py:615-640, eval numerics)
  NewFCStepper    maxout LSTMCore.forward   (FCModel.py:13-42 via AttModel.py:904-945)
  Att2in2Stepper  capmi_att2in2_decode_step (Att2in2Core.forward, AttModel.py:750-790, eval numerics)
  AdaAttStepper   capmi_adaatt_decode_step  (AdaAttCore.forward, AttModel.py:604-613, eval numerics)
  EnsembleStepper M member steppers + capmi_ensemble_logprobs (AttEnsemble.get_logprobs_state, AttEnsemble.py:45-53)

disc.DiscStepper (discriminative decoding, opt['distractors']) wraps any of them the way EnsembleStepper wraps its members.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import lib, ptr, check, stream_ptr

_f32 = torch.float32


class _Stepper:
    """The recurrent state of B * cap hypotheses as a ping-pong pair [2, S, N, R] (a step and a beam reorder read one half and
    write the other), the workspace, and the beam reorder."""

    def _init_state(self, B, R, V1, rows_per_image_max, S, dev):
        self.B, self.R, self.V1, self.cap = B, R, V1, int(rows_per_image_max)
        self.N = B * self.cap
        self.ws = ops.default_workspace(dev)
        self.state = torch.zeros(2, S, self.N, R, dtype=_f32, device=dev)
        self.cur = 0

    def reorder(self, parent, cur):
        from . import beam
        src, dst = self.state[self.cur], self.state[1 - self.cur]
        beam.reorder_rows(src, dst, parent, self.B, cur, parent.shape[1])
        self.cur = 1 - self.cur

    HIDDEN = 0                        # the slot of the state that the vocabulary projection reads

    def hidden(self, rows):
        """the pre-logit rows of the last step, [rows, R] (read-only view of the state; a reorder or the next step moves it)"""
        return self.state[self.cur][self.HIDDEN, :rows]


class _StructStepper(_Stepper):
    """A stepper whose step is ONE native call on a capmi.h struct.  The family fills the struct's dims and features and states
    its buffers (by field name; `it` and `logits` are added here) and its entry point."""

    STEP = None                       # native entry point, by name
    TRACE = 'alpha'                   # the buffer that holds the step's region weights [rows, K] (att_trace.Recorder)

    def _bind(self, s, bufs, dev):
        logits = torch.empty(self.N, self.V1, dtype=_f32, device=dev)
        self.bufs = dict(bufs, logits=logits, it=torch.zeros(self.N, dtype=torch.long, device=dev))
        for k, t in self.bufs.items():
            setattr(s, k, t.data_ptr())
        s.partial, s.partial_capacity = self.ws.buf.data_ptr(), self.ws.capacity
        self.s = s

    def _native(self, rows, rows_per_image, src, dst):
        return getattr(lib, self.STEP)(C.byref(self.w), C.byref(self.s), rows, rows_per_image, ptr(src[0]), ptr(src[1]),
                                       ptr(dst[0]), ptr(dst[1]), stream_ptr())

    def step(self, t, it, rows_per_image):
        rows = self.B * rows_per_image
        assert it.shape[0] == rows and rows_per_image <= self.cap
        self.bufs['it'][:rows].copy_(it)
        check(self._native(rows, rows_per_image, self.state[self.cur], self.state[1 - self.cur]), self.STEP)
        self.cur = 1 - self.cur
        return self.bufs['logits'][:rows]


class _OneLayerState:
    """snapshot / restore, and the reference layout of the recurrent state (h [layers,N,R], c [layers,N,R]) for a core that
    reads the last layer and returns one; the stepper's state is (h, c)"""

    def snapshot(self):
        return self.state[self.cur].clone()

    def restore(self, snap):
        self.state[self.cur].copy_(snap)

    def load_state(self, state, rows):
        h, c = state
        s = self.state[self.cur]
        s[0, :rows], s[1, :rows] = h[-1], c[-1]

    def export_state(self, rows):
        s = self.state[self.cur]
        return (s[0, :rows].clone().unsqueeze(0), s[1, :rows].clone().unsqueeze(0))


class UpDownStepper(_StructStepper):
    STEP = 'capmi_updown_decode_step'
    HIDDEN = 2                        # h_lang

    def __init__(self, P, pr, rows_per_image_max):
        from . import updown_engine
        self.P, self.pr = P, pr
        dev = pr.att.device
        B, K, R = pr.att.shape
        A = pr.p_att.shape[2]
        V1, E = P['embed.0.weight'].shape
        self._init_state(B, R, V1, rows_per_image_max, 4, dev)      # (h_att, c_att, h_lang, c_lang)
        N = self.N
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)       # noqa: E731
        b = _lib.UpDownBeam()
        b.B, b.bd, b.K, b.A, b.R, b.E, b.V1, b.L = B, self.cap, K, A, R, E, V1, 0
        b.fc, b.att, b.p_att, b.att_mask = ptr(pr.fc), ptr(pr.att), ptr(pr.p_att), ptr(pr.att_masks)
        b.temperature, b.unk_col = 1.0, -1
        self._bind(b, dict(xt=z(N, E), gates=z(N, 4 * R), att_h=z(N, A), alpha=z(N, K), ctx=z(N, R), fc_gates=z(B, 4 * R)), dev)
        self.w = updown_engine.weights_struct(P)
        self._first = True

    def _native(self, rows, rows_per_image, src, dst):
        first, self._first = self._first, False
        return lib.capmi_updown_decode_step(C.byref(self.w), C.byref(self.s), rows, rows_per_image, ptr(src), ptr(dst),
                                            1 if first else 0, stream_ptr())

    # reference layout of the recurrent state: (h [2,N,R], c [2,N,R]) with index 0 = att_lstm, 1 = lang_lstm
    def load_state(self, state, rows):
        h, c = state
        s = self.state[self.cur]
        s[0, :rows], s[1, :rows], s[2, :rows], s[3, :rows] = h[0], c[0], h[1], c[1]

    def export_state(self, rows):
        s = self.state[self.cur]
        return (torch.stack([s[0, :rows], s[2, :rows]]), torch.stack([s[1, :rows], s[3, :rows]]))


class NewFCStepper(_Stepper):
    """AttModel.py:925-936: the first call feeds the image (state all zero), then words.  The image step is taken in the
    constructor so that step(0, BOS) is the first WORD step like for every other family."""

    def __init__(self, P, fc_feats, rows_per_image_max, drop_out=None):
        # drop_out [steps, B*rows_per_image_max, R] (train-mode beam search): step t multiplies the LSTMCore output of row r
        # by drop_out[t, r] before the logit (FCModel.py:40); the image step's output is discarded, so it has no mask
        dev = fc_feats.device
        self.P = P
        self.drop_out = drop_out
        B = fc_feats.shape[0]
        V1, self.E = P['embed.weight'].shape
        R = P['_core.h2h.weight'].shape[1]
        self._init_state(B, R, V1, rows_per_image_max, 2, dev)      # (h, c)
        N = self.N
        self.saved = torch.empty(N, 5 * R, dtype=_f32, device=dev)
        self.logits = torch.empty(N, self.V1, dtype=_f32, device=dev)
        self.h_drop = None if drop_out is None else torch.empty(N, R, dtype=_f32, device=dev)
        fc_emb = ops.linear(fc_feats.float().contiguous(), P['fc_embed.weight'], P['fc_embed.bias'], ws=self.ws)
        self._cell(fc_emb, B)                                           # one row per image, cur = 1 afterwards

    def hidden(self, rows):
        """the cell output the logit reads (under a train-mode mask: the dropped copy)"""
        return self.state[self.cur][0, :rows] if self.drop_out is None else self.h_drop[:rows]

    def _cell(self, x, rows, out_mask=None):
        P, R, E = self.P, self.R, self.E
        src, dst = self.state[self.cur], self.state[1 - self.cur]
        splits = ops.gemm([(x, E, P['_core.i2h.weight'], E, E, 1), (src[0, :rows], R, P['_core.h2h.weight'], R, R, 1)], rows,
                          5 * R, self.ws.buf, ws=self.ws, defer_reduce=True)
        check(lib.capmi_maxout_cell_fwd(self.ws.slabs.data_ptr(), splits, ptr(P['_core.i2h.bias']), ptr(P['_core.h2h.bias']),
                                        ptr(src[1]), ptr(dst[0]), ptr(dst[1]), ptr(self.saved), ptr(out_mask),
                                        None if out_mask is None else ptr(self.h_drop), rows, R, stream_ptr()), 'capmi_maxout_cell_fwd')
        self.cur = 1 - self.cur
        self._keep = x

    def step(self, t, it, rows_per_image):
        rows = self.B * rows_per_image
        if t == 0 and rows_per_image > 1:
            # the image step left one row per image: fan it out (AttModel._sample repeats the features BEFORE the image
            # step, same values)
            idx = torch.arange(rows, device=it.device) // rows_per_image
            s = self.state[self.cur]
            s[:, :rows] = s[:, :self.B][:, idx]
        x = ops.embed_fwd(it, self.P['embed.weight'], relu=False)      # plain Embedding (AttModel.py:908)
        mask = None if self.drop_out is None else self.drop_out[t, :rows]
        self._cell(x, rows, mask)
        h = self.hidden(rows)
        logits = self.logits[:rows]
        ops.gemm([(h, self.R, self.P['logit.weight'], self.R, self.R, 1)], rows, self.V1, logits, bias=self.P['logit.bias'],
                 ws=self.ws)
        return logits


class Att2in2Stepper(_OneLayerState, _StructStepper):
    """Att2in2Model (AttModel.py:854-859): BOS first, no image step; the state is (h, c) of the one cell."""

    STEP = 'capmi_att2in2_decode_step'

    def __init__(self, P, pr, rows_per_image_max):
        from . import att2in2_engine
        dev = pr.att.device
        B, K, R = pr.att.shape
        A = pr.p_att.shape[2]
        V1, E = P['embed.0.weight'].shape
        self.P, self.pr = P, pr
        self._init_state(B, R, V1, rows_per_image_max, 2, dev)
        N = self.N
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)       # noqa: E731
        s = _lib.Att2in2Step()
        s.B, s.K, s.A, s.R, s.E, s.V1 = B, K, A, R, E, V1
        s.att, s.p_att, s.att_mask = ptr(pr.att), ptr(pr.p_att), ptr(pr.att_masks)
        self._bind(s, dict(xt=z(N, E), att_h=z(N, A), alpha=z(N, K), ctx=z(N, R), saved=z(N, 5 * R)), dev)
        self.w = att2in2_engine.weights_struct(P)


class AdaAttStepper(_OneLayerState, _StructStepper):
    """AdaAttModel / AdaAttMOModel (AttModel.py:843-852): BOS first, no image step; the state is (h, c) of the one layer (the
    undropped h: AdaAtt_lstm returns it beside the copy that goes on to the attention)."""

    STEP = 'capmi_adaatt_decode_step'
    TRACE = 'pi'                      # [rows, K + 1]: sentinel, then the regions

    def __init__(self, P, ap, rows_per_image_max):
        from . import adaatt_engine
        dev = ap.att.device
        B, K, R = ap.att.shape
        A = ap.p_att.shape[2]
        V1, E = P['embed.0.weight'].shape
        W = ap.fc_gates.shape[1]
        self.P, self.pr = P, ap
        self._init_state(B, R, V1, rows_per_image_max, 2, dev)
        N = self.N
        z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)       # noqa: E731
        s = _lib.AdaAttStep()
        s.B, s.K, s.A, s.R, s.E, s.V1, s.maxout = B, K, A, R, E, V1, int(W == 6 * R)
        s.fc_gates, s.att, s.p_att, s.att_mask = ptr(ap.fc_gates), ptr(ap.att), ptr(ap.p_att), ptr(ap.att_masks)
        self._bind(s, dict(xt=z(N, E), saved=z(N, W), h_drop=z(N, R), fake_drop=z(N, R), fr=z(N, E), ho_t=z(N, E), ho=z(N, E),
                           fr_e=z(N, A), ho_e=z(N, A), pi=z(N, K + 1), ctx=z(N, R), out_t=z(N, R), out_drop=z(N, R)), dev)
        self.w = adaatt_engine.weights_struct(P, ap.packs)

    def hidden(self, rows):
        """the attention output tanh(att2h(.)) the logit reads (eval numerics: out_drop is the undropped row)"""
        return self.bufs['out_drop'][:rows]


class EnsembleStepper:
    """AttEnsemble's decoder step over M member steppers of any family: every member takes the same tokens, then ONE launch of
    capmi_ensemble_logprobs turns their M rows of logits into the mixture log-probability (a normalised row: the drivers'
    log_softmax leaves it unchanged, and their temperature applies to the mixture, as CaptionModel.py:204 does).  Members with
    weight 0 are stepped too.  snapshot / restore exist when every member has them."""

    def __init__(self, members, weights=None):
        self.members = list(members)
        self.w = ops.ensemble_weights(weights, len(self.members))
        V1 = {m.V1 for m in self.members}
        B = {m.B for m in self.members}
        if len(V1) != 1 or len(B) != 1:
            raise _lib.CapmiError('ensemble members disagree on the vocabulary or the batch (V1 %s, B %s)' % (sorted(V1), sorted(B)))
        self.V1, self.B = V1.pop(), B.pop()
        self.out = None
        if all(hasattr(m, 'snapshot') and hasattr(m, 'restore') for m in self.members):
            self.snapshot, self.restore = self._snapshot, self._restore

    def step(self, t, it, rows_per_image):
        logits = [m.step(t, it, rows_per_image) for m in self.members]
        rows = logits[0].shape[0]
        if self.out is None or self.out.shape[0] < rows:
            self.out = torch.empty(rows, self.V1, dtype=_f32, device=logits[0].device)
        return ops.ensemble_logprobs(logits, self.w, out=self.out[:rows])

    def reorder(self, parent, cur):
        for m in self.members:
            m.reorder(parent, cur)

    def _snapshot(self):
        return [m.snapshot() for m in self.members]

    def _restore(self, snap):
        for m, s in zip(self.members, snap):
            m.restore(s)
