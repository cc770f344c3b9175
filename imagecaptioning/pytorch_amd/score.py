"""Scoring GIVEN captions: log p(caption | image) under the model, for captions that came from elsewhere -- another system's output,
human captions, candidate lists -- and self-retrieval, the discriminability measure of a captioner (Dai and Lin 2017, "Contrastive
Learning for Image Captioning"; Luo et al. 2018, "Discriminability Objective for Training Descriptive Captions"): does a caption
pick its own image out of a pool.  Test-time only: no autograd graph, no [N, T, V1] log-probabilities, no BPTT buffers.

``score_captions(model, fc_feats, att_feats, att_masks, seqs, opt)`` takes one of two pairings:

  aligned  seqs [B, n, L] (or [B * n, L], image-major): the n captions of each image -> [B, n]
  cross    seqs [C, L] with opt['pairing'] = 'cross': every caption against every image -> S [C, B]

Captions follow the label convention: token 0 ends a caption (padding is 0), the end token itself is scored -- the shifted mask of
LanguageModelCriterion -- and a caption that fills all L columns has no end token to score.  ``len`` counts the scored tokens.

The decoder is the family's single-step decoder (step.py protocol), driven as beam.beam_search_steps drives it: step(0, BOS, 1)
with one row per image, reorder(parent = 0, cur = 1) fans the state out to one row per (image, caption), then step(t + 1, tokens
of column t, rows_per_image).  After each step's logits capmi_score_step (csrc/score.hip) reads every live row once and adds the
given token's log-probability; nothing of the logits' size is written.  (The one exception is the root step: its logits, one row
per image, are copied out to the fanned rows -- a copy of one step's logits per tile.)  The number of steps is 1 + the longest
caption of the tile, at most L; the host reads the captions' lengths and token range ONCE per call, before any step.

Tiling: no step holds more than opt['score_rows'] rows (default: default_rows(V1, rnn_size): the rows whose float32 logits fill
512 MB, and no more than the steppers' shared split-K workspace takes).
Image tiles are the outer loop and the features are prepared ONCE per image tile; caption tiles are the inner loop, each on a fresh
stepper made from the same prepared features.  A tile takes as many captions as fit (up to all of them), then as many images.

opt: 'temperature' (every step scores softmax(logits / temperature), the root step too), 'suppress_UNK' (the UNK token scores 1000
lower, as in beam search), 'score_norm' ('none' | 'length': the returned scores are divided by len), 'score_tok_logp' (keep the
per-token log-probabilities; default: aligned yes, cross no -- [C, B, L] floats).
"""
import math

import torch

from . import ops

_f32 = torch.float32
LOGITS_BYTES = 512 << 20
WORKSPACE_FLOATS = 16 * 1024 * 1024      # ops.Workspace's slabs
NORMS = ('none', 'length')
PAIRINGS = ('aligned', 'cross')


def default_rows(V1, R=None):
    """The default opt['score_rows']: the largest row count whose float32 logits [rows, V1] stay within 512 MB (9488 columns: 14146
    rows) and -- R: the model's rnn_size -- whose widest gate pre-activations [rows, 6 R] (the maxout LSTM of AdaAttMO; 4 R / 5 R
    in the other families) fit the split-K workspace the steppers share (ops.Workspace: 16 Mi floats), because a stepper's gate GEMM
    leaves its K slices there for the cell kernel.  At the configured sizes (R = 1000, V1 = 9488) the second bound decides: 2796."""
    rows = LOGITS_BYTES // (4 * int(V1))
    if R:
        rows = min(rows, WORKSPACE_FLOATS // (6 * int(R)))
    return max(1, rows)


def check_options(model, opt):
    """every refusal of a scoring call that does not depend on the tensors, before any device work -> (pairing, norm, score_rows)"""
    opt = opt or {}
    refusal = getattr(model, '_sbs_refusal', 'the model has no single-step decoder for the beam driver')
    if refusal is not None or not hasattr(model, '_decode_stepper'):
        raise NotImplementedError("mode='score' is not implemented for %s: %s"
                                  % (type(model).__name__, refusal or 'the model has no single-step decoder for the beam driver'))
    if model.training:
        raise NotImplementedError("mode='score' is a test-time mode without gradients: call model.eval() first")
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError("output_logsoftmax=0: mode='score' returns log-probabilities, a raw logit is no score of a caption")
    pairing = opt.get('pairing', 'aligned')
    if pairing not in PAIRINGS:
        raise ValueError("opt['pairing'] is 'aligned' or 'cross', got %r" % (pairing,))
    norm = opt.get('score_norm', 'none') or 'none'
    if norm not in NORMS:
        raise ValueError("opt['score_norm'] is 'none' or 'length', got %r" % (norm,))
    if not float(opt.get('temperature', 1.0)) > 0 or math.isinf(float(opt.get('temperature', 1.0))):
        raise ValueError("mode='score' needs a finite temperature > 0, got %r" % (opt.get('temperature'),))
    rows = opt.get('score_rows')
    if rows is not None and int(rows) < 1:
        raise ValueError("opt['score_rows'] is a row count >= 1, got %r" % (rows,))
    return pairing, norm, None if rows is None else int(rows)


def shape_of(seqs, B, L, pairing):
    """the shape rules of the two pairings -> (captions per image or C, seqs as [B, n, L] / [C, L])"""
    if not torch.is_tensor(seqs) or seqs.dtype.is_floating_point or seqs.dtype == torch.bool:
        raise ValueError("mode='score' takes the captions as an integer tensor of token ids")
    if seqs.dim() not in (2, 3) or seqs.shape[-1] < 1 or seqs.shape[-1] > L:
        raise ValueError("mode='score': captions are [.., L'] token ids with 1 <= L' <= seq_length = %d, got %s" % (L, tuple(seqs.shape)))
    if pairing == 'cross':
        if seqs.dim() != 2 or seqs.shape[0] < 1:
            raise ValueError("pairing 'cross' takes seqs [C, L], every caption against every image; got %s" % (tuple(seqs.shape),))
        return seqs.shape[0], seqs
    if seqs.dim() == 3:
        if seqs.shape[0] != B or seqs.shape[1] < 1:
            raise ValueError("pairing 'aligned' takes seqs [B, n, L] with B = %d images, got %s" % (B, tuple(seqs.shape)))
        return seqs.shape[1], seqs
    if seqs.shape[0] < B or seqs.shape[0] % B:
        raise ValueError("pairing 'aligned' takes seqs [B * n, L], image-major, with B = %d images; got %d rows"
                         % (B, seqs.shape[0]))
    return seqs.shape[0] // B, seqs.reshape(B, seqs.shape[0] // B, seqs.shape[1])


def plan(B, n, score_rows):
    """The tiles of B images x n captions (per image, or of the cross product) with at most score_rows rows each:
    [((i0, i1), [(c0, c1), ...]), ...] -- image tiles outside, caption tiles inside.  A tile takes as many captions as fit, then as
    many images; every (image, caption) pair lies in exactly one tile."""
    score_rows = max(1, int(score_rows))
    ct = min(n, score_rows)
    bt = min(B, max(1, score_rows // ct))
    caps = [(c, min(c + ct, n)) for c in range(0, n, ct)]
    return [((i, min(i + bt, B)), caps) for i in range(0, B, bt)]


def lengths(seqs):
    """words before the first 0 of every caption (device, int64 [..]); L for a caption without one"""
    L = seqs.shape[-1]
    return (seqs != 0).long().cumprod(-1).sum(-1) if L else seqs.new_zeros(seqs.shape[:-1])


def run(prepare, B, V1, seqs, pairing, dev, score_rows=None, inv_temperature=1.0, unk_col=-1, keep_tok=True, hook=None):
    """The tiled driver.  prepare(i0, i1) -> make_decoder for the images [i0, i1) (the prefill; called once per image tile),
    make_decoder(rows_per_image) -> a fresh stepper.  seqs int64 [B, n, L] (aligned) or [C, L] (cross) on `dev`.
    Returns {'logp', 'len' (int32), 'tok_logp' (or None)}: [B, n] (+ [L]) aligned, [C, B] (+ [L]) cross.
    hook: a dict that receives 'logits' -- per tile and step a clone of what was scored (tests)."""
    cross = pairing == 'cross'
    n, L = (seqs.shape[0] if cross else seqs.shape[1]), seqs.shape[-1]
    seqs = seqs.long().contiguous()
    lens = lengths(seqs)
    host = torch.cat([lens.reshape(-1), seqs.min().reshape(1), seqs.max().reshape(1)]).cpu()       # the call's one read of the device
    lo, hi = int(host[-2]), int(host[-1])
    if lo < 0 or hi >= V1:
        raise ValueError("mode='score': token ids must lie in [0, %d), the captions hold %d .. %d" % (V1, lo, hi))
    lens_h = host[:-2].reshape(lens.shape)
    shape = (n, B) if cross else (B, n)
    logp = torch.zeros(shape, dtype=_f32, device=dev)
    count = torch.zeros(shape, dtype=torch.int32, device=dev)
    tokp = torch.zeros(shape + (L,), dtype=_f32, device=dev) if keep_tok else None
    for (i0, i1), cap_tiles in plan(B, n, score_rows or default_rows(V1)):
        make = prepare(i0, i1)
        bt = i1 - i0
        for c0, c1 in cap_tiles:
            ct = c1 - c0
            rows = bt * ct
            if cross:
                toks = seqs[c0:c1].unsqueeze(0).expand(bt, ct, L)
                longest = int(lens_h[c0:c1].max())
            else:
                toks = seqs[i0:i1, c0:c1]
                longest = int(lens_h[i0:i1, c0:c1].max())
            T = min(L, longest + 1)
            toks = toks.reshape(rows, L)[:, :T].t().contiguous()                # [T, rows]: a step's tokens are contiguous
            live = torch.ones(rows, dtype=torch.uint8, device=dev)
            acc = torch.zeros(rows, dtype=_f32, device=dev)
            cnt = torch.zeros(rows, dtype=torch.int32, device=dev)
            tl = torch.zeros(T, rows, dtype=_f32, device=dev) if keep_tok else None
            dec = make(ct)
            root = dec.step(0, torch.zeros(bt, dtype=torch.long, device=dev), 1)              # BOS, one row per image
            logits = root if ct == 1 else root.unsqueeze(1).expand(bt, ct, V1).contiguous().view(rows, V1)
            if T > 1:
                dec.reorder(torch.zeros(bt, ct, dtype=torch.int32, device=dev), 1)
            for t in range(T):
                if hook is not None:
                    hook.setdefault('logits', []).append(((i0, i1), (c0, c1), t, logits.clone()))
                ops.score_step(logits, toks[t], live, acc, cnt, None if tl is None else tl[t], inv_temperature, unk_col)
                if t + 1 < T:
                    logits = dec.step(t + 1, toks[t], ct)
            if cross:
                logp[c0:c1, i0:i1] = acc.view(bt, ct).t()
                count[c0:c1, i0:i1] = cnt.view(bt, ct).t()
                if tl is not None:
                    tokp[c0:c1, i0:i1, :T] = tl.view(T, bt, ct).permute(2, 1, 0)
            else:
                logp[i0:i1, c0:c1] = acc.view(bt, ct)
                count[i0:i1, c0:c1] = cnt.view(bt, ct)
                if tl is not None:
                    tokp[i0:i1, c0:c1, :T] = tl.view(T, bt, ct).permute(1, 2, 0)
    return {'logp': logp, 'len': count, 'tok_logp': tokp}


def score_captions(model, fc_feats, att_feats, att_masks, seqs, opt=None):
    """log p(caption | image) of given captions (see the module docstring) -> [B, n] (aligned) or S [C, B] (cross), divided by the
    scored length under opt['score_norm'] = 'length'.  Sets model.last_score = {'logp', 'len', 'tok_logp', 'perplexity'} (device
    tensors; logp the joint log-probability whatever the norm, perplexity = exp(-logp / len)).  Every refusal comes before any
    device work."""
    from . import beam, _lib
    opt = opt or {}
    model.last_score = None
    pairing, norm, score_rows = check_options(model, opt)
    B, L, V1 = att_feats.shape[0], model.seq_length, model.vocab_size + 1
    n, seqs = shape_of(seqs, B, L, pairing)
    for t in (fc_feats, att_feats, att_masks, seqs):
        if t is not None and not t.is_cuda:
            raise _lib.CapmiError('the capmi backend runs on a HIP device only (got a %s tensor); there is no CPU path' % t.device.type)
    dev = att_feats.device

    def prepare(i0, i1):
        return model._decode_stepper(fc_feats[i0:i1], att_feats[i0:i1], None if att_masks is None else att_masks[i0:i1], L)

    with torch.no_grad():
        out = run(prepare, B, V1, seqs, pairing, dev, score_rows or default_rows(V1, getattr(model, 'rnn_size', None)), 1.0 / float(opt.get('temperature', 1.0)),
                  beam.unk_column(model, opt, V1), bool(opt.get('score_tok_logp', pairing == 'aligned')), opt.get('_score_hook'))
        per_len = out['logp'] / out['len'].to(_f32)
        out['perplexity'] = torch.exp(-per_len)
    model.last_score = out
    return per_len if norm == 'length' else out['logp']


def retrieval_summary(ranks, pool_size=None, pools=None):
    """host arithmetic on the ranks (1 = the caption picked its own image): R@1, R@5, R@10, median / mean rank, MRR"""
    ranks = sorted(int(r) for r in ranks)
    m = len(ranks)
    if m == 0:
        raise ValueError('retrieval_summary: no ranks')
    if ranks[0] < 1:
        raise ValueError('retrieval_summary: ranks start at 1')
    out = {'R@%d' % k: sum(1 for r in ranks if r <= k) / m for k in (1, 5, 10)}
    out['median_rank'] = (ranks[(m - 1) // 2] + ranks[m // 2]) / 2
    out['mean_rank'] = sum(ranks) / m
    out['MRR'] = sum(1.0 / r for r in ranks) / m
    out['captions'] = m
    if pool_size is not None:
        out['pool_size'] = int(pool_size)
    if pools is not None:
        out['pools'] = int(pools)
    return out


def encode_captions(captions, vocab, L, oov='unk'):
    """words -> token rows: captions a list of strings (or word lists) -> (int64 [n, L] padded with 0, words outside the vocabulary
    per caption).  oov 'unk': such a word becomes the vocabulary's UNK token (ValueError if it has none); 'drop': it is left out.
    Captions are cut at L words."""
    if oov not in ('unk', 'drop'):
        raise ValueError("oov is 'unk' or 'drop', got %r" % (oov,))
    inv = {w: int(i) for i, w in vocab.items()}
    unk = inv.get('UNK')
    rows = torch.zeros(len(captions), L, dtype=torch.long)
    missing = []
    for k, cap in enumerate(captions):
        words = cap.split() if isinstance(cap, str) else list(cap)
        ids, miss = [], 0
        for w in words:
            ix = inv.get(w)
            if ix is None:
                miss += 1
                if oov == 'drop':
                    continue
                if unk is None:
                    raise ValueError('%r is not in the vocabulary, which has no UNK token to stand in for it (drop such words instead)' % (w,))
                ix = unk
            ids.append(ix)
        ids = ids[:L]
        rows[k, :len(ids)] = torch.tensor(ids, dtype=torch.long)
        missing.append(miss)
    return rows, missing
