"""Discriminative decoding: ``opt['distractors']`` makes a sample call produce captions that tell each image from given distractor
images of the same batch -- the decode-time counterpart of the self-retrieval numbers of score.py.  It is the introspective
(emitter-suppressor) speaker of Vedantam et al. 2017, "Context-aware captions from context-agnostic supervision", and in its
listener form the RSA speaker of Cohn-Gordon et al. 2018, "Pragmatically informative image captioning with character-level
inference".  No training, no new weights: the same token history is stepped under the target image and under its D distractors,
and capmi_disc_combine (csrc/disc.hip) turns the 1 + D vocabulary rows of a hypothesis into the row the search sees.

    opt['distractors']  integer tensor [B, D], host or device, 1 <= D <= D_MAX = 7: entry [b, d] is the index, within this call's
                        batch, of a distractor image for image b; -1: no distractor in this slot (images may have different
                        numbers of distractors, none included).  An image may not be its own distractor.
    opt['disc_lambda']  lambda in [0, 1], default 0.5; 1 is the plain decoder
    opt['disc_mode']    'suppress' (default) | 'listener'

With lt the log-softmax of the decoder's logits under image b, ld_i the same under its i-th present distractor, D' their number:

    suppress   u[v] = lt[v] - (1 - lambda) (logsumexp_i ld_i[v] - log D')            log p(w|I_t) - (1 - lambda) log mean_i p(w|I_d_i)
    listener   u[v] = lt[v] + (1 - lambda) (lt[v] - logsumexp_{j in {t} + distractors} l_j[v])
                                                      the second term: the posterior of a literal listener, uniform prior over the images
    D' = 0 or lambda = 1: u = lt

u is handed to the searches as the stepper's "logits": they normalise it as they normalise any stepper's logits, and temperature,
suppress_UNK, decoding_constraint, remove_bad_endings and length_penalty apply to the normalised pragmatic distribution; the
seqLogprobs of such a call are that distribution's.  The literal log p(caption | image) of the result is what mode='score' gives.

Such a call runs the stepper-driven searches (beam.beam_search_steps, the samplers of decode.py, stochastic and constrained beam
search) on a DiscStepper, for every family with a single-step decoder; the families' one-call rollouts are not used.  The features
of the B * (1 + D) slots are gathered and prefilled slot by slot (a distractor that serves several images is prefilled once per use).
After the call ``model.last_disc = {'distractors', 'lambda', 'mode'}`` (the distractors as given, int64 [B, D] on the device).
"""
import math

import torch

from . import ops

D_MAX = 7             # CAPMI_DISC_MAX - 1
MODES = ('suppress', 'listener')


def wanted(opt):
    return bool(opt) and opt.get('distractors') is not None


class Request:
    """The checked options of one call (host tensors): distractors int64 [B, D], slots int64 [B, 1 + D] -- the feature index of
    every slot, column 0 the image itself, an absent slot the image itself too, so that the stepper has something to step --
    present uint8 [B, 1 + D], lam, mode.  on(dev) puts the tables on the device, once."""

    def __init__(self, distractors, lam, mode):
        B, D = distractors.shape
        own = torch.arange(B, dtype=torch.long).unsqueeze(1)
        there = distractors >= 0
        self.distractors, self.lam, self.mode = distractors, float(lam), mode
        self.B, self.D, self.D1 = B, D, 1 + D
        self.slots = torch.cat([own, torch.where(there, distractors, own.expand(B, D))], 1)
        self.present = torch.cat([torch.ones(B, 1, dtype=torch.uint8), there.to(torch.uint8)], 1)
        self.device, self.cbs = None, None

    def on(self, dev):
        if self.device != dev:
            self.slots_dev, self.present_dev = self.slots.to(dev), self.present.to(dev).contiguous()
            self.distractors_dev = self.distractors.to(dev)
            self.device = dev
        return self


def rows_per_image(opt, cbs_req=None):
    """the rows per image of the search such a call runs (the stepper's rows_per_image_max)"""
    if cbs_req is not None:
        return cbs_req.S * cbs_req.b
    method = opt.get('sample_method', 'greedy')
    if method == 'sbs':
        return int(opt.get('sample_n', 1))
    if int(opt.get('beam_size', 1)) > 1 and method in ('greedy', 'beam_search'):
        G = max(1, int(opt.get('group_size', 1)))
        return int(opt['beam_size']) // G
    if int(opt.get('group_size', 1)) > 1:
        return int(opt['group_size'])
    return int(opt.get('sample_n', 1))


def check_options(model, opt, B):
    """every refusal of a sample call with opt['distractors'], before any device work -> Request; with opt['constraints'] those of
    cbs.prepare too, whose Request is kept as .cbs (else None).  (Distractors given as a device tensor are read once, here.)"""
    name = type(model).__name__
    refusal = getattr(model, '_sbs_refusal', 'the model has no single-step decoder for the beam driver')
    if refusal is not None or not hasattr(model, '_decode_stepper'):
        raise NotImplementedError("opt['distractors'] (discriminative decoding) is not implemented for %s: %s"
                                  % (name, refusal or 'the model has no single-step decoder for the beam driver'))
    if model.training:
        if int(opt.get('beam_size', 1)) > 1 and torch.is_grad_enabled():
            raise NotImplementedError("opt['distractors'] does not support train_beam_size > 1 (beam search in train mode with "
                                      'gradients): it is a test-time option')
        raise NotImplementedError("opt['distractors'] is a test-time option: call model.eval() first")
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError("output_logsoftmax=0 is implemented for the sampled / greedy rollout; opt['distractors'] "
                                  'returns log-probabilities')
    if opt.get('return_attention', 0):
        raise NotImplementedError("return_attention together with opt['distractors'] is not implemented: the recorder's row layout "
                                  'is per stepper row, and a discriminative call steps 1 + D rows per hypothesis')
    d = opt['distractors']
    if not torch.is_tensor(d) or d.dtype.is_floating_point or d.dtype == torch.bool or d.dim() != 2:
        raise ValueError("opt['distractors'] is an integer tensor [B, D] of image indices within the batch (-1: no distractor)")
    if d.shape[0] != B:
        raise ValueError("opt['distractors'] lists %d images, the batch holds %d" % (d.shape[0], B))
    if not 1 <= d.shape[1] <= D_MAX:
        raise ValueError("opt['distractors']: 1 <= D <= %d distractor slots per image, got %d" % (D_MAX, d.shape[1]))
    d = d.detach().to('cpu', torch.long)
    if B and (int(d.min()) < -1 or int(d.max()) >= B):
        raise ValueError("opt['distractors']: indices lie in [-1, %d), the table holds %d .. %d" % (B, int(d.min()), int(d.max())))
    own = (d == torch.arange(B).unsqueeze(1)).any(1)
    if bool(own.any()):
        raise ValueError("opt['distractors']: image %d is listed as its own distractor" % int(own.nonzero()[0]))
    lam = opt.get('disc_lambda', 0.5)
    lam = 0.5 if lam is None else float(lam)
    if not 0.0 <= lam <= 1.0 or math.isnan(lam):
        raise ValueError("opt['disc_lambda'] lies in [0, 1], got %r" % (opt.get('disc_lambda'),))
    mode = opt.get('disc_mode', 'suppress') or 'suppress'
    if mode not in MODES:
        raise ValueError("opt['disc_mode'] is 'suppress' or 'listener', got %r" % (mode,))
    from . import cbs, score
    cbs_req = cbs.prepare(model, opt) if cbs.wanted(opt) else None
    rows = B * (1 + d.shape[1]) * max(1, rows_per_image(opt, cbs_req))
    limit = score.default_rows(model.vocab_size + 1, getattr(model, 'rnn_size', None))
    if rows > limit:
        raise ValueError("opt['distractors']: B * (1 + D) * rows_per_image = %d rows in one decoder step, the steppers' shared "
                         'workspace bounds them at %d: decode fewer images per call' % (rows, limit))
    req = Request(d, lam, mode)
    req.cbs = cbs_req
    return req


class DiscStepper:
    """A stepper (step.py protocol) over B images whose step is the pragmatic row of every hypothesis.  `inner` is the family's
    stepper over the G = B * (1 + D) feature slots of req.slots, slot-major: its row (b * (1 + D) + d) * cur + j is hypothesis j of
    image b under slot d's features.  step() repeats each image's tokens to its slots, steps `inner` once and launches
    capmi_disc_combine once; reorder() repeats the parents likewise.  The repeated tokens and parents and the returned rows live in
    buffers made here, once; nothing reads the device.  snapshot / restore exist when `inner` has them."""

    def __init__(self, inner, req, rows_per_image_max):
        if req.device is None:
            raise ValueError('DiscStepper: put the request on the device first (Request.on)')
        self.inner, self.req = inner, req
        self.B, self.D1, self.V1, self.cap = req.B, req.D1, inner.V1, int(rows_per_image_max)
        if inner.B != self.B * self.D1:
            raise ValueError('DiscStepper: the inner stepper holds %d feature slots, B * (1 + D) = %d' % (inner.B, self.B * self.D1))
        dev, G = req.device, self.B * self.D1
        self.it = torch.zeros(G * self.cap, dtype=torch.long, device=dev)
        self.parent = torch.zeros(G * self.cap, dtype=torch.int32, device=dev)
        self.out = torch.empty(self.B * self.cap, self.V1, dtype=torch.float32, device=dev)
        if hasattr(inner, 'snapshot') and hasattr(inner, 'restore'):
            self.snapshot, self.restore = inner.snapshot, inner.restore

    def step(self, t, it, cur):
        B, D1 = self.B, self.D1
        assert it.shape[0] == B * cur and cur <= self.cap
        rep = self.it[:B * D1 * cur]
        rep.view(B, D1, cur).copy_(it.view(B, 1, cur).expand(B, D1, cur))
        logits = self.inner.step(t, rep, cur)
        return ops.disc_combine(logits, self.req.present_dev, self.req.lam, self.req.mode, B, D1, cur, self.out[:B * cur])

    def reorder(self, parent, cur):
        B, D1, bd = self.B, self.D1, parent.shape[1]
        rep = self.parent[:B * D1 * bd].view(B, D1, bd)
        rep.copy_(parent.view(B, 1, bd).expand(B, D1, bd))
        self.inner.reorder(rep.view(B * D1, bd), cur)


def make_stepper(model, req, fc_feats, att_feats, att_masks, L):
    """make(rows_per_image) -> DiscStepper for the model's family: its single-step decoder over the gathered features of the slots"""
    idx = req.on(att_feats.device).slots_dev.view(-1)
    gather = lambda t: t[idx] if (torch.is_tensor(t) and t.dim() > 0 and t.shape[0] == req.B) else t       # noqa: E731
    inner = model._decode_stepper(gather(fc_feats), gather(att_feats), gather(att_masks), L)
    return lambda rows: DiscStepper(inner(rows), req, rows)


# ---- choosing distractors within a batch (tools/eval.py --disc_pick) ------------------------------------------------------------
def pooled_regions(att_feats, att_masks=None):
    """the mean of every image's valid region features [B, F] (fc_feats is not used: Att2in2 gets zeros there)"""
    x = att_feats.float()
    if att_masks is None:
        return x.mean(1)
    m = att_masks.to(x.dtype).unsqueeze(2)
    return (x * m).sum(1) / m.sum(1).clamp(min=1.0)


def pick_nearest(att_feats, att_masks, D):
    """int64 [B, D]: per image the D other images of the batch with the highest cosine similarity of the pooled region features,
    most similar first; a batch with fewer than D + 1 images pads with -1.  One GEMM and a top-k, on the features' device."""
    B = att_feats.shape[0]
    out = torch.full((B, D), -1, dtype=torch.long, device=att_feats.device)
    k = min(D, B - 1)
    if k > 0:
        p = torch.nn.functional.normalize(pooled_regions(att_feats, att_masks), dim=1)
        sim = p @ p.t()
        sim.fill_diagonal_(float('-inf'))
        out[:, :k] = sim.topk(k, dim=1).indices
    return out


def pick_random(B, D, generator=None):
    """int64 [B, D] (host): per image D other images of the batch, drawn without replacement with `generator` (a seeded
    torch.Generator makes the pick reproducible); a batch with fewer than D + 1 images pads with -1"""
    out = torch.full((B, D), -1, dtype=torch.long)
    k = min(D, B - 1)
    for b in range(B if k > 0 else 0):
        others = torch.cat([torch.arange(b), torch.arange(b + 1, B)])
        out[b, :k] = others[torch.randperm(B - 1, generator=generator)[:k]]
    return out
