"""Beam search for the UpDown model on libcapmi: ONE native call runs all L steps on the device
(capmi_updown_beam_search); the host then reads the small [L,B,b] parent/token/score tables once and
assembles ``done_beams`` exactly as CaptionModel.beam_search does (CaptionModel.py:183-209), group_size 1.
"""
import ctypes as C

import torch

from . import _lib, logits_proc, ops, updown_engine as engine
from ._lib import lib, ptr, check, stream_ptr

_f32 = torch.float32


def _penalty(cfg):
    """captioning/utils/misc.py:133-157 penalty_builder."""
    if cfg == '':
        return lambda length, logp: logp
    kind, alpha = cfg.split('_')
    alpha = float(alpha)
    if kind == 'wu':
        return lambda length, logp: logp / (((5 + length) ** alpha) / ((5 + 1) ** alpha))
    if kind == 'avg':
        return lambda length, logp: logp / length
    raise ValueError(cfg)


def sample_beam(model, fc_feats, att_feats, att_masks, opt):
    """AttModel._sample_beam (AttModel.py:218-256): returns (seq [B*sample_n, L], seqLogprobs [.., L, V1]) and
    sets model.done_beams[k] = [{'seq','logps','unaug_p','p'}, ...] sorted by descending p."""
    beam_size = opt.get('beam_size', 10)
    group_size = opt.get('group_size', 1)
    sample_n = opt.get('sample_n', 10)
    assert sample_n == 1 or sample_n == beam_size // group_size, 'when beam search, sample_n == 1 or beam search'
    model._device_check(fc_feats)
    P = {k: v.detach() for k, v in model.named_parameters()}
    pr = engine.prepare(P, fc_feats.float().contiguous(), att_feats.float().contiguous(),
                        None if att_masks is None else att_masks.float(), bn=model._region_bn(False))      # an eval-mode prefill
    dev = fc_feats.device
    if group_size != 1 or opt.get('decoding_constraint', 0) or opt.get('remove_bad_endings', 0) or model._trace_req is not None \
            or logits_proc.wanted(opt):
        # diverse groups / decoding constraints / logits processors / return_attention: same kernels, host-stepped (the one-call search below has no
        # hooks and keeps no per-step weights)
        from .step import UpDownStepper
        return beam_search_steps(model, lambda rows: UpDownStepper(P, pr, rows), pr.att.shape[0], P['embed.0.weight'].shape[0],
                                 model.seq_length, opt, dev)
    B, V1 = pr.att.shape[0], P['embed.0.weight'].shape[0]
    L, bd = model.seq_length, beam_size
    bufs = _native_search(model, P, pr, bd, L, opt)
    return assemble_done_beams(model, bufs['parent'], bufs['token'], bufs['score'], bufs['ended'], bufs['logp_rows'], B, bd, L, V1,
                               sample_n, beam_size, opt)


def _native_search(model, P, pr, bd, L, opt, drop_xt=None, drop_out=None, train=False):
    """All L steps of the UpDown search in one native call; returns the buffers (tables parent / token / score / ended [L,B,bd],
    logp_rows [L,B*bd,V1]).  train: capmi_updown_beam_search_train, `pr` holds the dropped features and drop_xt [L,B*bd,E] /
    drop_out [L,B*bd,R] are the keep masks by search row (None: no dropout there)."""
    dev = pr.att.device
    B, K, R = pr.att.shape
    A = pr.p_att.shape[2]
    V1, E = P['embed.0.weight'].shape
    assert bd <= V1
    N = B * bd
    ws = ops.default_workspace(dev)
    z = lambda *s: torch.empty(*s, dtype=_f32, device=dev)       # noqa: E731
    bufs = dict(state=z(2, 4, N, R), xt=z(N, E), gates=z(N, 4 * R), att_h=z(N, A), alpha=z(N, K), ctx=z(N, R),
                fc_gates=z(B, 4 * R), logits=z(N, V1), it=torch.empty(N, dtype=torch.long, device=dev), sums=z(2, B, bd),
                logp_rows=z(L, N, V1), parent=torch.empty(L, B, bd, dtype=torch.int32, device=dev),
                token=torch.empty(L, B, bd, dtype=torch.long, device=dev), score=z(L, B, bd),
                ended=torch.empty(L, B, bd, dtype=torch.uint8, device=dev))
    bt = _lib.UpDownBeamTrain() if train else None
    b = bt.b if train else _lib.UpDownBeam()
    b.B, b.bd, b.K, b.A, b.R, b.E, b.V1, b.L = B, bd, K, A, R, E, V1, L
    b.fc, b.att, b.p_att, b.att_mask = ptr(pr.fc), ptr(pr.att), ptr(pr.p_att), ptr(pr.att_masks)
    b.temperature = float(opt.get('temperature', 1))
    b.unk_col = unk_column(model, opt, V1)
    for k, t in bufs.items():
        setattr(b, k, t.data_ptr())
    b.partial, b.partial_capacity = ws.buf.data_ptr(), ws.capacity
    w = engine.weights_struct(P)
    if train:
        for m, c in ((drop_xt, E), (drop_out, R)):
            assert m is None or (m.shape == (L, N, c) and m.is_contiguous() and m.dtype == _f32)
        bufs['h_drop'] = z(N, R)
        bt.drop_xt, bt.drop_out, bt.h_drop = ptr(drop_xt), ptr(drop_out), ptr(bufs['h_drop'])
        check(lib.capmi_updown_beam_search_train(C.byref(w), C.byref(bt), stream_ptr()), 'capmi_updown_beam_search_train')
    else:
        check(lib.capmi_updown_beam_search(C.byref(w), C.byref(b), stream_ptr()), 'capmi_updown_beam_search')
    return bufs


# ---------------------------------------------------------------------------------------------------------------------------
# Beam search as a training rollout (reference ADVANCED.md "SCST in Topdown Bottomup paper": train_sample_method greedy,
# train_beam_size > 1): search with training numerics -> capmi_beam_finalize -> forced replay of the surviving beams with the
# dropout masks their ancestors saw.  Nothing here reads the device.
# ---------------------------------------------------------------------------------------------------------------------------
_len_div_cache = {}
marks = None        # a list: the phases of a training beam search append (name, recorded event) -- scripts/tools_beam_scst_bench.py


def _mark(name):
    if marks is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))


def length_divisors(cfg, L, dev):
    """[L] float64 on the device: what the length penalty `cfg` divides the joint log-prob of a (t+1)-word beam by, computed
    with the host arithmetic of _penalty (so that device keys order exactly like the host's); None for ''.  Cached."""
    if cfg == '':
        return None
    key = (cfg, L, str(dev))
    t = _len_div_cache.get(key)
    if t is None:
        kind, alpha = cfg.split('_')
        alpha = float(alpha)
        if kind == 'wu':
            div = [((5 + n) ** alpha) / ((5 + 1) ** alpha) for n in range(1, L + 1)]
        elif kind == 'avg':
            div = [float(n) for n in range(1, L + 1)]
        else:
            raise ValueError(cfg)
        t = _len_div_cache[key] = torch.tensor(div, dtype=torch.float64).to(dev)
    return t


def finalize(parent, token, score, ended, sample_n, length_penalty=''):
    """capmi_beam_finalize: tables [L,B,bd] -> (seq [B*sample_n,L] int64, lineage [L,B*sample_n] int32, length [B*sample_n] int32,
    p [B*sample_n] fp32), all on the device (CaptionModel.py:183-208)."""
    L, B, bd = parent.shape
    dev = parent.device
    rows = B * sample_n
    seq = torch.empty(rows, L, dtype=torch.long, device=dev)
    lineage = torch.empty(L, rows, dtype=torch.int32, device=dev)
    length = torch.empty(rows, dtype=torch.int32, device=dev)
    p = torch.empty(rows, dtype=_f32, device=dev)
    div = length_divisors(length_penalty, L, dev)
    check(lib.capmi_beam_finalize(ptr(parent), ptr(token), ptr(score), ptr(ended), ptr(div), B, bd, L, sample_n, ptr(seq),
                                  ptr(lineage), ptr(length), ptr(p), stream_ptr()), 'capmi_beam_finalize')
    return seq, lineage, length, p


def lineage_gather(lineage, rows_src, src_a, src_b=None):
    """mask_replay[t, i, :] = mask_search[t, lineage[t, i], :] for one or two [L, rows_src, C] arrays in one launch."""
    L, rows = lineage.shape
    out = [None if s is None else torch.empty(L, rows, s.shape[2], dtype=_f32, device=s.device) for s in (src_a, src_b)]
    if src_a is None and src_b is None:
        return out
    check(lib.capmi_lineage_gather(ptr(lineage), L, rows_src, rows, ptr(src_a), ptr(out[0]), 0 if src_a is None else src_a.shape[2],
                                   ptr(src_b), ptr(out[1]), 0 if src_b is None else src_b.shape[2], stream_ptr()),
          'capmi_lineage_gather')
    return out


def wants_train_beam(model, opt):
    """The dispatch rule of the training beam search: beam_size > 1, greedy / beam_search, train mode, gradients enabled."""
    return (opt.get('beam_size', 1) > 1 and opt.get('sample_method', 'greedy') in ('greedy', 'beam_search') and model.training
            and torch.is_grad_enabled())


def refuse_train_beam(model, opt):
    """Families without a training beam search: refuse instead of returning log-probs that carry no gradient."""
    if wants_train_beam(model, opt):
        raise NotImplementedError('train_beam_size > 1 (beam search in train mode with gradients) is implemented for updown / '
                                  'topdown and newfc, not for %s; its eval / no_grad beam search is unchanged' % type(model).__name__)


def check_train_beam_options(opt):
    """Options the replay cannot reproduce (none is reachable from LossWrapper's training calls except the last two)."""
    for name, bad in (('group_size', int(opt.get('group_size', 1)) != 1), ('decoding_constraint', opt.get('decoding_constraint', 0)),
                      ('remove_bad_endings', opt.get('remove_bad_endings', 0)), ('temperature', float(opt.get('temperature', 1)) != 1.0),
                      ('output_logsoftmax', not opt.get('output_logsoftmax', 1)), ('use_ppo', opt.get('use_ppo', 0))):
        if bad:
            raise NotImplementedError('the training beam search (train_beam_size > 1) does not support %s=%r'
                                      % (name, opt.get(name)))
    beam_size, sample_n = opt.get('beam_size', 10), opt.get('sample_n', 10)
    assert sample_n == 1 or sample_n == beam_size, 'when beam search, sample_n == 1 or beam search'


def updown_beam_train(model, fc_feats, att_feats, att_masks, opt):
    """AttModel._sample_beam called in train() mode with gradients (loss_wrapper.py with train_beam_size > 1): returns
    (seq [B*sample_n, L], seqLogprobs [B*sample_n, L, V1] attached to the forced rollout's autograd function)."""
    if getattr(model, 'use_bn', 0):
        # the search and its forced replay would each run a train-mode prefill: two updates of the running statistics per step
        raise NotImplementedError('train_beam_size > 1 does not support use_bn=%d: the search-then-replay would update the BatchNorm '
                                  'running statistics more than once per step' % model.use_bn)
    check_train_beam_options(opt)
    bd, sample_n = opt.get('beam_size', 10), opt.get('sample_n', 10)
    fc_feats, att_feats = fc_feats.float().contiguous(), att_feats.float().contiguous()
    att_masks = None if att_masks is None else att_masks.float().contiguous()
    B, L, dev = fc_feats.shape[0], model.seq_length, fc_feats.device
    K = ops.clip_len(att_masks, att_feats.shape[1])
    masks = opt.get('_beam_masks')              # test hook: injected keep masks (drop_fc, drop_att, drop_xt, drop_out by search row)
    if masks is None:
        masks = model._dropout_masks(B, K, B * bd, L, dev)
    _mark('start')
    with torch.no_grad():
        P = {k: v.detach() for k, v in model._named_param_list()}
        pr = engine.prepare(P, fc_feats, att_feats, att_masks, masks.get('drop_fc'), masks.get('drop_att'))
        bufs = _native_search(model, P, pr, bd, L, opt, masks.get('drop_xt'), masks.get('drop_out'), train=True)
        _mark('search')
        seq, lineage, length, p = finalize(bufs['parent'], bufs['token'], bufs['score'], bufs['ended'], sample_n,
                                           opt.get('length_penalty', ''))
        r_xt, r_out = lineage_gather(lineage, B * bd, masks.get('drop_xt'), masks.get('drop_out'))
        _mark('finalize')
    cfg = dict(n=sample_n, T=L, L=L, mode='forced', forced=seq, temperature=1.0)
    for k, v in (('drop_fc', masks.get('drop_fc')), ('drop_att', masks.get('drop_att')), ('drop_xt', r_xt), ('drop_out', r_out)):
        if v is not None:
            cfg[k] = v
    model.done_beams = None                      # not assembled on the host in this path
    model._last_beam = dict(score=bufs['score'], parent=bufs['parent'], token=bufs['token'], ended=bufs['ended'], lineage=lineage,
                            length=length, p=p)
    out = model._run(cfg, fc_feats, att_feats, att_masks)
    _mark('replay')
    return out


def newfc_beam_train(model, fc_feats, opt):
    """The same for NewFCModel: the search is host-stepped over NewFCStepper (L iterations, no synchronisation), the only
    dropout is the LSTMCore output's ([L, B*bd, R] by search row; the image step's output is discarded)."""
    from .step import NewFCStepper
    check_train_beam_options(opt)
    bd, sample_n = opt.get('beam_size', 10), opt.get('sample_n', 10)
    fc_feats = fc_feats.float().contiguous()
    B, L, dev = fc_feats.shape[0], model.seq_length, fc_feats.device
    masks = opt.get('_beam_masks')
    if masks is None:
        masks = {}
        if model.drop_prob_lm > 0:
            masks['drop_out'] = ops.dropout_mask((L, B * bd, model.rnn_size), model.drop_prob_lm, model._next_seed(), 0, dev)
    drop = masks.get('drop_out')
    _mark('start')
    with torch.no_grad():
        P = dict(zip(model._param_names, [q.detach() for q in model._param_list()]))
        parent, token, score, ended, _ = beam_search_steps(model, lambda rows: NewFCStepper(P, fc_feats, rows, drop_out=drop), B,
                                                           P['embed.weight'].shape[0], L, opt, dev, tables_only=True)
        _mark('search')
        seq, lineage, length, p = finalize(parent, token, score, ended, sample_n, opt.get('length_penalty', ''))
        r_out, _ = lineage_gather(lineage, B * bd, drop)
        _mark('finalize')
    cfg = dict(n=sample_n, T=L, L=L, mode='forced', forced=seq, temperature=1.0)
    if r_out is not None:
        cfg['drop_out'] = r_out
    model.done_beams = None
    model._last_beam = dict(score=score, parent=parent, token=token, ended=ended, lineage=lineage, length=length, p=p)
    out = model._run(cfg, fc_feats)
    _mark('replay')
    return out


def assemble_done_beams(model, parent, token, score, ended, logp_rows, B, bd, L, V1, sample_n, beam_size, opt, groups=1):
    """One device->host transfer of the small [L,B,groups*bd] tables, then the bookkeeping of CaptionModel.py:183-209:
    per image and group the finished beams sorted by p, best bd kept, groups concatenated (:207-208)."""
    dev = logp_rows.device
    W = groups * bd
    N = B * W
    parent, token, score, ended = (t.cpu().numpy() for t in (parent, token, score, ended))
    penalty = _penalty(opt.get('length_penalty', ''))
    seq = torch.zeros(B * sample_n, L, dtype=torch.long, device=dev)
    seq_logp = torch.zeros(B * sample_n, L, V1, dtype=_f32, device=dev)
    done_beams = []
    gather_idx, gather_meta = [], []
    for k in range(B):
        beams = []
        for g in range(groups):
            fin = []
            for t in range(L):
                for j in range(g * bd, (g + 1) * bd):
                    if ended[t, k, j]:
                        fin.append((penalty(t + 1, float(score[t, k, j])), t, j))
            fin = sorted(fin, key=lambda x: -x[0])[:bd]            # stable, like the reference's sorted()
            for p, t, j in fin:
                toks, rows = [], []
                jj = j
                for s in range(t, -1, -1):
                    toks.append(int(token[s, k, jj]))
                    par = int(parent[s, k, jj])                   # index among the image's W rows of step s-1
                    rows.append(s * N + (k if s == 0 else k * W + par))   # step-0 rows are one per image
                    jj = par
                toks.reverse()
                rows.reverse()
                beams.append({'seq': torch.tensor(toks, dtype=torch.long, device=dev), 'p': p, '_rows': rows})
                gather_idx.extend(rows)
                gather_meta.append((k, len(beams) - 1, len(rows)))
        done_beams.append(beams)
    if gather_idx:
        flat = logp_rows.view(L * N, V1)[torch.tensor(gather_idx, device=dev)]
        off = 0
        sums = []
        for k, bi, ln in gather_meta:
            lp = flat[off:off + ln]
            off += ln
            done_beams[k][bi]['logps'] = lp
            sums.append(lp.sum())
        sums = torch.stack(sums).cpu().tolist()
        for (k, bi, _), s in zip(gather_meta, sums):
            done_beams[k][bi]['unaug_p'] = s
            del done_beams[k][bi]['_rows']
    model.done_beams = done_beams
    for k in range(B):
        if sample_n == beam_size:
            for _n in range(sample_n):
                ln = done_beams[k][_n]['seq'].shape[0]
                seq[k * sample_n + _n, :ln] = done_beams[k][_n]['seq']
                seq_logp[k * sample_n + _n, :ln] = done_beams[k][_n]['logps']
        else:
            ln = done_beams[k][0]['seq'].shape[0]
            seq[k, :ln] = done_beams[k][0]['seq']
            seq_logp[k, :ln] = done_beams[k][0]['logps']
    return seq, seq_logp


def unk_column(model, opt, V1):
    """CaptionModel.py:159-162: the column pushed down by 1000 when suppress_UNK is on."""
    if opt.get('suppress_UNK', 0) and hasattr(model, 'vocab') and model.vocab.get(str(V1 - 1)) == 'UNK':
        return V1 - 1
    if getattr(model, 'unk_idx', None) is not None:
        return int(model.unk_idx)
    return -1


def _decode_flags(model, opt, dev):
    flags = (_lib.DECODE_NO_REPEAT if opt.get('decoding_constraint', 0) else 0) | \
            (_lib.DECODE_NO_BAD_ENDING if opt.get('remove_bad_endings', 0) else 0)
    bad = torch.tensor(sorted(getattr(model, 'bad_endings_ix', [])), dtype=torch.long, device=dev)
    return flags, bad


def _normaliser(model, opt, V1, dev, root_temperature=1.0, renormalise=False, edit=None):
    """-> normalise(t, logits, out, rows, prev_token): out[:rows] = log_softmax(logits / T) with the UNK column pushed down
    (CaptionModel.py:159-162), T = root_temperature at t = 0 and opt['temperature'] afterwards (:203-204); from t = 1 on
    capmi_decode_constrain against the previous tokens when decoding_constraint / remove_bad_endings are set (:152-155).
    renormalise (sbs): edited rows go through a second log_softmax, so that they are distributions again.
    edit(t, rows_tensor, rows) or None: one more in-place edit of the step's rows, after the others (the logits processors)."""
    temperature = float(opt.get('temperature', 1))
    unk = unk_column(model, opt, V1)
    flags, bad = _decode_flags(model, opt, dev)
    st = stream_ptr()
    edited = [None]

    def normalise(t, logits, out, rows, prev_token):
        dst = out
        if renormalise and (flags or unk >= 0 or edit is not None):
            if edited[0] is None:
                edited[0] = torch.empty(out.shape[0], V1, dtype=_f32, device=dev)
            dst = edited[0]
        check(lib.capmi_beam_logsoftmax(ptr(logits), ptr(dst), rows, V1, temperature if t else root_temperature, unk, st),
              'beam_logsoftmax')
        if flags and t > 0:
            check(lib.capmi_decode_constrain(ptr(dst), rows, V1, ptr(prev_token), 1, flags, ptr(bad), bad.numel(), None, 0, t, 0, st),
                  'decode_constrain')
        if edit is not None:
            edit(t, dst, rows)
        if dst is not out:
            check(lib.capmi_beam_logsoftmax(ptr(dst), ptr(out), rows, V1, 1.0, -1, st), 'beam_logsoftmax')
    return normalise


def _search_loop(model, make_decoder, B, W, V1, L, opt, dev, select, trace=True, root_temperature=1.0, renormalise=False,
                 exempt=None):
    """The loop that the beam search, the stochastic and the constrained beam search share, W rows per image: step the decoder
    (from BOS on one row per image, then on B * W rows), normalise the rows (root_temperature, renormalise: _normaliser's),
    select(t, logp_t [B * cur, V1], cur, parent_t, token_t) -- it fills the step's [B, W] slices -- and reorder the decoder's
    state; the last step only selects.  The caller makes the tables its select writes before it calls, so their zero fills precede
    the decoder's construction on the stream.  With a logits processor on (logits_proc.py) every step's rows are edited once more
    after the normaliser's own edits, from the histories that the parent / token tables below hold: capmi_logits_process walks the
    parents itself (exempt int32 [B, n]: per image, words its n-gram rule spares).  Nothing reads the device.  Returns (logp_rows [L, B * W, V1], parent int32 / token int64 [L, B, W], and the
    recorders of att_trace.recording when the model wants the attention and `trace` allows it, else None)."""
    recs = None
    if trace and getattr(model, '_trace_req', None) is not None:
        from . import att_trace
        make_decoder, recs = att_trace.recording(make_decoder, L)
    dec = make_decoder(W)
    N = B * W
    logp_rows = torch.zeros(L, N, V1, dtype=_f32, device=dev)
    parent = torch.zeros(L, B, W, dtype=torch.int32, device=dev)
    token = torch.zeros(L, B, W, dtype=torch.long, device=dev)
    proc = logits_proc.make(opt, L)                                          # None: the four options are at their defaults
    edit = None if proc is None else (lambda t, x, rows: proc.search(x, rows, V1, t, token, parent, 1 if t == 0 else W, exempt))
    normalise = _normaliser(model, opt, V1, dev, root_temperature, renormalise, edit)
    it, rows, cur = torch.zeros(B, dtype=torch.long, device=dev), B, 1       # BOS
    for t in range(L):
        logits = dec.step(t, it, cur)
        normalise(t, logits, logp_rows[t], rows, token[t - 1] if t else None)
        select(t, logp_rows[t, :rows], cur, parent[t], token[t])
        if t == L - 1:
            break
        dec.reorder(parent[t], cur)
        it, rows, cur = token[t].reshape(N), N, W
    return logp_rows, parent, token, recs


def _publish_trace(model, recs, lineage, length, n):
    """return_attention of a search that backtracks on the device: the recorded weights along the lineage, n captions per image"""
    if recs is not None:
        from . import att_trace
        att_trace.publish(model, att_trace.beam(recs[0].buf, lineage, length, model._trace_req.Kout), n)


def seq_logp_from_lineage(logp_rows, lineage):
    """seqLogprobs [rows, L, V1] of the paths of lineage [L, rows] (beam.finalize's convention): step t's row lineage[t, i] of
    logp_rows [L, N, V1], zeros where lineage < 0 (behind a path's end)."""
    L, _, V1 = logp_rows.shape
    live = (lineage >= 0).unsqueeze(2)
    gathered = logp_rows.gather(1, lineage.clamp(min=0).long().unsqueeze(2).expand(L, lineage.shape[1], V1))
    return torch.where(live, gathered, gathered.new_zeros(())).permute(1, 0, 2).contiguous()


def beam_search_steps(model, make_decoder, B, V1, L, opt, dev, tables_only=False):
    """CaptionModel.beam_search (CaptionModel.py:35-209) for any decoder given as a single-step object (step.py
    protocol): the selection / reordering / normalisation / constraint / diversity kernels are native, only the decoder
    step is a callback.  Covers decoding_constraint, remove_bad_endings, suppress_UNK, temperature, length_penalty and
    -- group_size > 1 -- diverse beam search, which is delegated to diverse_beam_search_steps.

    make_decoder(rows_per_image) -> decoder with
      step(t, it, rows_per_image) -> logits [B*rows_per_image, V1]: consumes tokens `it` (BOS zeros at t = 0, one row per
          image; afterwards rows_per_image rows per image, image-major) and advances the state;
      reorder(parent [B,bd] int32, cur): state row b*cur + parent[b,j] becomes row b*bd + j.
    """
    beam_size = opt.get('beam_size', 10)
    sample_n = opt.get('sample_n', 10)
    if int(opt.get('group_size', 1)) != 1:
        return diverse_beam_search_steps(model, make_decoder, B, V1, L, opt, dev)
    assert sample_n == 1 or sample_n == beam_size, 'when beam search, sample_n == 1 or beam search'
    bd = beam_size
    score = torch.zeros(L, B, bd, dtype=_f32, device=dev)
    ended = torch.zeros(L, B, bd, dtype=torch.uint8, device=dev)
    sums = torch.zeros(2, B, bd, dtype=_f32, device=dev)
    st = stream_ptr()

    def select(t, logp_t, cur, parent_t, token_t):
        check(lib.capmi_beam_select(ptr(logp_t), ptr(sums[t & 1]), B, cur, bd, V1, 1 if t == L - 1 else 0, ptr(parent_t),
                                    ptr(token_t), ptr(score[t]), ptr(sums[(t + 1) & 1]), ptr(ended[t]), st), 'beam_select')
    # the first distribution is the model's own log_softmax; the temperature enters at CaptionModel.py:203-204 only
    logp_rows, parent, token, recs = _search_loop(model, make_decoder, B, bd, V1, L, opt, dev, select, trace=not tables_only)
    if tables_only:                                                         # the training search finalises on the device
        return parent, token, score, ended, logp_rows
    if recs is not None:
        from . import att_trace
        att_trace.from_beam(model, recs[0], parent, token, score, ended, sample_n if sample_n == beam_size else 1, B * sample_n, opt)
    return assemble_done_beams(model, parent, token, score, ended, logp_rows, B, bd, L, V1, sample_n, beam_size, opt)


def stochastic_beam_search_steps(model, make_decoder, B, V1, L, opt, dev):
    """Stochastic beam search (sbs.py; Kool et al. 2019) for any decoder of the protocol above: opt['sample_n'] = k distinct captions
    per image, drawn without replacement from the model.  A sibling of beam_search_steps: the decoder step is the callback, the
    normalisation / constraints / selection (capmi_sbs_select) / reordering / backtrack (capmi_sbs_backtrack) are native, nothing
    reads the device.

    Sampling semantics: EVERY step's rows are log_softmax(logits / temperature), step 0 included.  suppress_UNK, decoding_constraint
    and remove_bad_endings edit the rows as in the beam path; the rows are then renormalised, so that the draw is without replacement
    from the constrained distribution.  Returns (seq [B*k, L], seqLogprobs [B*k, L, V1]) like a sampled rollout with sample_n = k
    (rows of an image by descending perturbed value) and sets model.last_sbs = {'phi', 'g', 'log_w'} [B, k] (sbs.py).
    opt['_gumbel'] [L, B*k, V1]: injected noise by search row (test hook; step 0 reads the first B rows)."""
    from . import sbs
    k = sbs.check_options(model, opt)
    if k > V1:
        raise ValueError("sample_method 'sbs': sample_n = %d captions need a vocabulary of at least as many words (%d)" % (k, V1))
    gumbel = opt.get('_gumbel')
    seed = model._next_seed()
    alive = torch.zeros(L, B, k, dtype=torch.uint8, device=dev)
    phi = torch.zeros(2, B, k, dtype=_f32, device=dev)
    g = torch.zeros(2, B, k, dtype=_f32, device=dev)
    root, zero = torch.ones(B, 1, dtype=torch.uint8, device=dev), torch.zeros(B, 1, dtype=_f32, device=dev)     # the root: phi 0

    def select(t, logp_t, cur, parent_t, token_t):
        i, o = t & 1, (t + 1) & 1
        state = (zero, zero, root) if t == 0 else (phi[i], g[i], alive[t - 1])
        ops.sbs_select(logp_t, *state, k, step0=t == 0, force_end=t == L - 1,
                       gumbel=None if gumbel is None else gumbel[t, :logp_t.shape[0]], seed=seed, offset=t,
                       out=(parent_t, token_t, phi[o], g[o], alive[t]))
    logp_rows, parent, token, recs = _search_loop(model, make_decoder, B, k, V1, L, opt, dev, select,
                                                  root_temperature=float(opt.get('temperature', 1)), renormalise=True)
    seq, length, lineage = ops.sbs_backtrack(parent, token, alive)
    seq_logp = seq_logp_from_lineage(logp_rows, lineage)
    phi_k, g_k = phi[L & 1].clone(), g[L & 1].clone()
    model.last_sbs = dict(phi=phi_k, g=g_k, log_w=sbs.log_weights(phi_k, g_k))
    _publish_trace(model, recs, lineage, length, k)
    return seq, seq_logp


def constrained_beam_search_steps(model, make_decoder, B, V1, L, opt, dev):
    """Constrained beam search (cbs.py; Anderson et al. 2017) for any decoder of the protocol above: opt['constraints'] lists, per
    image, sets of tokens of which the caption must contain one each.  A sibling of beam_search_steps and everything that is not
    about states is that function's: the root row at temperature 1, `temperature` afterwards, suppress_UNK, decoding_constraint and
    remove_bad_endings through the same kernels, ended hypotheses carried on 1000 lower.  The decoder steps S * beam_size rows per
    image (slot = state * beam_size + j, S = 2^C states of the batch's largest C); capmi_cbs_select keeps the beam_size best per
    state, capmi_cbs_finalize picks the caption; nothing reads the device.  Returns (seq [B, L], seqLogprobs [B, L, V1]) and sets
    model.last_cbs = {'state', 'satisfied', 'total', 'score'} [B] (cbs.py)."""
    from . import cbs
    req = getattr(model, '_cbs_req', None) or cbs.prepare(model, opt)
    if req.B != B:
        raise ValueError("opt['constraints'] lists %d images, the batch holds %d" % (req.B, B))
    b, S = req.b, req.S
    SB = S * b
    if V1 < 2:
        raise ValueError("opt['constraints'] needs a vocabulary")
    tables = ops.cbs_tables(req.words, req.ncons, V1, S, dev)
    score = torch.zeros(L, B, SB, dtype=_f32, device=dev)
    ended = torch.zeros(L, B, SB, dtype=torch.uint8, device=dev)
    valid = torch.zeros(L, B, SB, dtype=torch.uint8, device=dev)
    sums = torch.zeros(2, B, SB, dtype=_f32, device=dev)

    def select(t, logp_t, cur, parent_t, token_t):
        ops.cbs_select(logp_t, sums[t & 1], tables, b, S, force_end=t == L - 1,
                       out=(parent_t, token_t, score[t], sums[(t + 1) & 1], ended[t], valid[t]))
    # no_repeat_ngram_size never blocks a word of the image's own constraint lists: a required word stays reachable
    exempt = req.words.reshape(B, -1).to(dev).contiguous() if (logits_proc.wanted(opt) and B) else None
    logp_rows, parent, token, recs = _search_loop(model, make_decoder, B, SB, V1, L, opt, dev, select, exempt=exempt)
    seq, lineage, length, state, p = ops.cbs_finalize(parent, token, score, ended, valid, tables.ncons, b, S,
                                                      length_divisors(opt.get('length_penalty', ''), L, dev))
    seq_logp = seq_logp_from_lineage(logp_rows, lineage)
    cbs.publish(model, state, tables.ncons, p)
    if isinstance(opt.get('_cbs_tables'), dict):                            # test hook: the per-step tables and rows
        opt['_cbs_tables'].update(parent=parent, token=token, score=score, ended=ended, valid=valid, logp_rows=logp_rows,
                                  lineage=lineage, length=length, words=req.words, ncons=req.ncons, b=b, S=S)
    _publish_trace(model, recs, lineage, length, 1)
    return seq, seq_logp


def diverse_beam_search_steps(model, make_decoder, B, V1, L, opt, dev):
    """Diverse beam search: group_size groups of bdash = beam_size // group_size beams; group g is penalised by
    diversity_lambda for every token the beams of groups < g hold at the same position (CaptionModel.add_diversity, :38-57).

    The groups run staggered in time exactly as in the reference (:145-204: at time t group g takes its local step t - g),
    and that matters: `beam_seq_table[pg][:, :, local_time]` is read AFTER group pg has already advanced g - pg further
    steps, so it holds position local_time of pg's *surviving* beams, not what pg chose at that step.  Here that column is
    recovered from pg's parent pointers by a (g - pg)-deep gather on the device.  Every group owns a decoder of bdash rows
    per image."""
    beam_size = opt.get('beam_size', 10)
    sample_n = opt.get('sample_n', 10)
    G = int(opt.get('group_size', 1))
    lam = float(opt.get('diversity_lambda', 0.5))
    assert beam_size % G == 0, 'beam_size must be a multiple of group_size (split_tensors, models/utils.py:19)'
    bd = beam_size // G
    assert sample_n == 1 or sample_n == bd, 'when beam search, sample_n == 1 or beam search'
    W, n = G * bd, B * bd
    normalise = _normaliser(model, opt, V1, dev)
    trace = getattr(model, '_trace_req', None)
    if trace is not None:
        # the returned caption of an image is the best beam of group 0 (CaptionModel.py:207-208 concatenates the groups in order):
        # only that group's decoder records
        from . import att_trace
        rec_make, recs = att_trace.recording(make_decoder, L)
    decs = [(rec_make if (trace is not None and g == 0) else make_decoder)(bd) for g in range(G)]
    logp_rows = torch.zeros(L, B * W, V1, dtype=_f32, device=dev)          # rows image-major, then group, then beam
    lparent = torch.zeros(G, L, B, bd, dtype=torch.int32, device=dev)      # per-group tables
    ltoken = torch.zeros(G, L, B, bd, dtype=torch.long, device=dev)
    lscore = torch.zeros(G, L, B, bd, dtype=_f32, device=dev)
    lended = torch.zeros(G, L, B, bd, dtype=torch.uint8, device=dev)
    sums = torch.zeros(G, 2, B, bd, dtype=_f32, device=dev)
    cur_logp = torch.empty(G, n, V1, dtype=_f32, device=dev)               # the rows group g selects from next
    aug = torch.empty(n, V1, dtype=_f32, device=dev)
    ident = torch.arange(bd, device=dev).expand(B, bd)
    st = stream_ptr()
    it0 = torch.zeros(B, dtype=torch.long, device=dev)                      # BOS
    for g in range(G):                                                      # logprobs_table = [init_logprobs.clone() ...] (:136)
        normalise(0, decs[g].step(0, it0, 1), cur_logp[g], B, None)
    logp_rows[0, :B] = cur_logp[0, :B]
    for t in range(L + G - 1):
        for g in range(G):
            lt = t - g
            if lt < 0 or lt > L - 1:
                continue
            cur = 1 if lt == 0 else bd
            src = cur_logp[g]
            sel = src
            if g > 0:
                prev = []
                for pg in range(g):
                    idx = ident
                    for s in range(min(t - pg, L - 1), lt, -1):            # follow pg's survivors back to position lt
                        idx = lparent[pg, s].long().gather(1, idx)
                    prev.append(ltoken[pg, lt].gather(1, idx))
                prev = torch.cat(prev, 1).contiguous()                     # [B, g*bd]
                check(lib.capmi_beam_diversity(ptr(src), ptr(aug), B, cur, V1, ptr(prev), g * bd, g * bd, lam, st), 'beam_diversity')
                sel = aug
            last = 1 if lt == L - 1 else 0
            check(lib.capmi_beam_select(ptr(sel), ptr(sums[g, lt & 1]), B, cur, bd, V1, last, ptr(lparent[g, lt]), ptr(ltoken[g, lt]),
                                        ptr(lscore[g, lt]), ptr(sums[g, (lt + 1) & 1]), ptr(lended[g, lt]), st), 'beam_select')
            if last:
                continue
            decs[g].reorder(lparent[g, lt], cur)
            normalise(lt + 1, decs[g].step(lt + 1, ltoken[g, lt].reshape(n), bd), cur_logp[g], n, ltoken[g, lt])
            logp_rows[lt + 1].view(B, G, bd, V1)[:, g] = cur_logp[g].view(B, bd, V1)
    # image-major global tables for the shared assembly: beam j of group g is column g*bd + j
    offs = (torch.arange(G, device=dev, dtype=torch.int32) * bd).view(G, 1, 1, 1)
    parent = (lparent + offs).permute(1, 2, 0, 3).reshape(L, B, W).contiguous()
    token = ltoken.permute(1, 2, 0, 3).reshape(L, B, W).contiguous()
    score = lscore.permute(1, 2, 0, 3).reshape(L, B, W).contiguous()
    ended = lended.permute(1, 2, 0, 3).reshape(L, B, W).contiguous()
    if trace is not None:
        att_trace.from_beam(model, recs[0], lparent[0], ltoken[0], lscore[0], lended[0], 1, B * sample_n, opt)
    return assemble_done_beams(model, parent, token, score, ended, logp_rows, B, bd, L, V1, sample_n, beam_size, opt, groups=G)


def reorder_rows(src, dst, parent, B, cur, bd):
    """dst[a, b*bd + j, :] = src[a, b*cur + parent[b,j], :] for stacked state arrays [arrays, rows, R] (capmi_beam_reorder)."""
    arrays, _, R = src.shape
    check(lib.capmi_beam_reorder(ptr(src), ptr(dst), ptr(parent), arrays, B, cur, bd, R, stream_ptr()), 'beam_reorder')
