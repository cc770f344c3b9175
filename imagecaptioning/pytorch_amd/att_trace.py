"""Per-word region attention of a decoded caption: ``opt['return_attention'] = 1`` on ``model(..., mode='sample')``.

The attention-LSTM families (updown / topdown, att2in2, adaatt, adaattmo) already keep every step's weights on the device -- the
rollouts as ``alpha [T, N, K]`` (AdaAtt: ``pi [T, N, K + 1]``, the visual sentinel in column 0 as AdaAtt_attention concatenates it,
AttModel.py:581-593), the steppers as the step's ``alpha [rows, K]``.  This module brings them into one caption-major array and
publishes it as ``model.last_attention``:

    att      [N, L, Kout]  float32   Kout = the caller's region count (+ 1 for AdaAtt); rows aligned with the returned seq;
                                     0 on the steps after a caption's end (losses._shifted_mask) and in the columns >= the clipped K
    top      [N, L]        int32     the arg-max column per word (lowest index on ties), -1 on zeroed steps
    top_w    [N, L]        float32   its weight
    entropy  [N, L]        float32   -sum a ln a
    box      [N, L, 4]     float32   sum_k a_k box_k, when opt['boxes'] [B, Kfull, 4] was passed

  rollout() / beam() / ground()   the three native entries (csrc/att_trace.hip), one launch each
  Request                         what a sample call asked for; CaptionModel.forward hangs it on the model for the call
  Recorder                        a stepper that keeps its inner stepper's weights of every step ([L, rows, K], copies on the stream)
  from_rollout / from_steps / from_beam   the three decode routes -> model.last_attention

Nothing here reads the device; with the option off none of it runs.
"""
import torch

from ._lib import lib, ptr, check, stream_ptr

_f32 = torch.float32


def wanted(opt):
    return bool(opt.get('return_attention', 0)) if opt else False


def rollout(alpha, seq, Kout, steps=None, beta=None):
    """capmi_att_trace_rollout: alpha [T, N, K] (the first `steps` steps are read), seq [N, L] int64 -> att [N, L, Kout]"""
    T, N, K = alpha.shape
    L = seq.shape[1]
    assert alpha.is_contiguous() and alpha.dtype == _f32 and seq.is_contiguous() and seq.dtype == torch.long and seq.shape[0] == N
    assert beta is None or (beta.shape == (T, N) and beta.is_contiguous() and beta.dtype == _f32)
    att = torch.empty(N, L, Kout, dtype=_f32, device=alpha.device)
    check(lib.capmi_att_trace_rollout(ptr(alpha), ptr(beta), ptr(seq), min(T if steps is None else int(steps), L), N, L, K, Kout,
                                      ptr(att), stream_ptr()), 'capmi_att_trace_rollout')
    return att


def beam(alpha_rows, lineage, length, Kout, out=None):
    """capmi_att_trace_beam: alpha_rows [L, rows_src, K] by search row, lineage [L, rows] / length [rows] (beam.finalize) ->
    att [rows, L, Kout] (out: a caller's contiguous target)"""
    L, rows_src, K = alpha_rows.shape
    rows = lineage.shape[1]
    assert alpha_rows.is_contiguous() and alpha_rows.dtype == _f32 and lineage.shape[0] == L and length.shape == (rows,)
    assert lineage.dtype == torch.int32 and length.dtype == torch.int32 and lineage.is_contiguous()
    att = torch.empty(rows, L, Kout, dtype=_f32, device=alpha_rows.device) if out is None else out
    assert att.shape == (rows, L, Kout) and att.is_contiguous()
    check(lib.capmi_att_trace_beam(ptr(alpha_rows), ptr(lineage), ptr(length), L, rows_src, rows, K, Kout, ptr(att), stream_ptr()),
          'capmi_att_trace_beam')
    return att


def ground(att, n=1, boxes=None, col0=0):
    """capmi_att_ground: att [N, L, Kw] -> dict(top, top_w, entropy[, box]); boxes [B, Kb, 4] are those of columns col0 .. of the
    image r // n of row r"""
    N, L, Kw = att.shape
    dev = att.device
    assert att.is_contiguous() and att.dtype == _f32
    out = dict(top=torch.empty(N, L, dtype=torch.int32, device=dev), top_w=torch.empty(N, L, dtype=_f32, device=dev),
               entropy=torch.empty(N, L, dtype=_f32, device=dev))
    B = Kb = 0
    if boxes is not None:
        boxes = boxes.to(device=dev, dtype=_f32).contiguous()
        B, Kb = boxes.shape[:2]
        assert boxes.shape == (B, Kb, 4)
        out['box'] = torch.empty(N, L, 4, dtype=_f32, device=dev)
    check(lib.capmi_att_ground(ptr(att), N, L, Kw, ptr(boxes), B, int(n), int(col0), Kb, ptr(out['top']), ptr(out['top_w']),
                               ptr(out['entropy']), ptr(out.get('box')), stream_ptr()), 'capmi_att_ground')
    return out


class Request:
    """One sample call's return_attention: B images of Kfull regions each, col0 leading columns that are no region (AdaAtt's
    sentinel), the optional boxes [B, Kfull, 4]"""
    __slots__ = ('B', 'Kfull', 'col0', 'boxes')

    def __init__(self, model, att_feats, opt):
        self.B, self.Kfull, self.col0, self.boxes = att_feats.shape[0], att_feats.shape[1], int(model._trace_col0), opt.get('boxes')
        if self.boxes is not None and tuple(self.boxes.shape) != (self.B, self.Kfull, 4):
            raise ValueError("opt['boxes'] must be [B, regions, 4] = %s, got %s" % ((self.B, self.Kfull, 4), tuple(self.boxes.shape)))

    @property
    def Kout(self):
        return self.Kfull + self.col0


def refuse(model):
    """Families without region attention and ensembles"""
    raise NotImplementedError('return_attention is implemented for the attention-LSTM families (updown / topdown, att2in2, adaatt, '
                              'adaattmo), not for %s: %s' % (type(model).__name__, model._trace_refusal))


def publish(model, att, n, filled=None):
    """att [N, L, Kout] with n caption rows per image -> model.last_attention.  filled < N: only the first `filled` rows hold
    captions (n of them per image); the rows behind them are zero and get top -1, every other number 0"""
    req = model._trace_req
    N = att.shape[0]
    filled = N if filled is None else filled
    out = dict(att=att)
    g = ground(att[:filled], n, req.boxes, req.col0)
    for k, t in g.items():
        if filled < N:
            pad = t.new_full((N - filled,) + tuple(t.shape[1:]), -1 if k == 'top' else 0)
            t = torch.cat([t, pad])
        out[k] = t
    model.last_attention = out


def from_rollout(model, ro):
    """the trace of a one-call rollout, from its own weight buffer (engine Rollout.TRACE names it)"""
    att = rollout(getattr(ro, ro.TRACE), ro.seq, model._trace_req.Kout, steps=getattr(ro, 'steps_run', None))
    publish(model, att, max(att.shape[0] // model._trace_req.B, 1))


class Recorder:
    """step.py protocol around a stepper: after every step the inner stepper's weights (its buffer named by TRACE) are copied, on the
    stream, into row t of buf [L, rows, K]"""

    def __init__(self, stepper, L):
        self.st = stepper
        self.src = stepper.bufs[stepper.TRACE]
        self.buf = torch.empty(L, self.src.shape[0], self.src.shape[1], dtype=_f32, device=self.src.device)

    def step(self, t, it, rows_per_image):
        out = self.st.step(t, it, rows_per_image)
        rows = self.st.B * rows_per_image
        self.buf[t, :rows].copy_(self.src[:rows])
        return out

    def __getattr__(self, name):            # reorder, snapshot / restore, V1, B, ...
        return getattr(self.st, name)


def recording(make_stepper, L):
    """make_stepper -> (make_stepper whose steppers record, the list they are appended to)"""
    made = []

    def make(rows):
        made.append(Recorder(make_stepper(rows), L))
        return made[-1]
    return make, made


def from_steps(model, rec, seq):
    """host-stepped sampling (decode.sample_steps / diverse_sample_steps): the recorded steps are laid out like a rollout's alpha"""
    att = rollout(rec.buf, seq.contiguous(), model._trace_req.Kout)
    publish(model, att, max(att.shape[0] // model._trace_req.B, 1))


def from_beam(model, rec, parent, token, score, ended, sample_n, n_rows, opt):
    """host-stepped beam search: capmi_beam_finalize on the tables of the recorded decoder, then the gather along the lineage.
    sample_n: beams kept per image (rows b * sample_n + j of the returned seq); n_rows: the rows of the returned seq -- the
    reference fills only the first B of them when sample_n is neither 1 nor beam_size, the others stay 0 here too."""
    from . import beam as beam_mod
    req = model._trace_req
    _, lineage, length, _ = beam_mod.finalize(parent, token, score, ended, sample_n, opt.get('length_penalty', ''))
    rows = lineage.shape[1]
    att = (torch.empty if rows == n_rows else torch.zeros)(n_rows, lineage.shape[0], req.Kout, dtype=_f32, device=rec.buf.device)
    beam(rec.buf, lineage, length, req.Kout, out=att[:rows])
    publish(model, att, sample_n, filled=rows)          # row i of the filled rows belongs to image i // sample_n
