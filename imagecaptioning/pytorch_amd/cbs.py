"""Constrained beam search: ``opt['constraints']`` makes the caption of every image contain given words (Anderson, Fernando, Johnson
and Gould 2017, "Guided Open Vocabulary Image Captioning with Constrained Beam Search").  The search is
beam.constrained_beam_search_steps on the kernels of csrc/cbs.hip; this module holds the option checks and the conversion of the
constraints to the device tables.

``opt['constraints']`` is a list of B entries, one per image; an entry is a list of C <= 4 constraints, a constraint a non-empty list
of <= 8 token ids or words (a disjunction such as ['zebra', 'zebras']: satisfied once one of them has been emitted).  Words are
looked up in ``model.vocab``.  A hypothesis's state is the bitmask of its satisfied constraints; the search keeps one beam of
``opt['beam_size']`` slots per state, S = 2^C states of the batch's largest C, S * beam_size <= 64 -- the decoder steps S * beam_size
rows per image.  The returned caption is the best finished hypothesis of the fully satisfied state; only if that state stayed empty,
of the state with the most constraints satisfied.  With no constraint on any image the call is the ordinary beam search bit for bit.

After such a call ``model.last_cbs = {'state', 'satisfied', 'total', 'score'}``, each [B] on the device: the mask of the returned
caption, its popcount, the image's C, and the caption's score after the length penalty.
"""
import torch

C_MAX, W_MAX, SLOTS_MAX = 4, 8, 64            # = cbs.hip / ops.CBS_*


def wanted(opt):
    return bool(opt) and opt.get('constraints') is not None


class Request:
    """The checked constraints of one call: words int32 [B, C_MAX, W_MAX] padded with -1 and ncons int32 [B] (host tensors),
    b = beam_size, S = states of the batch."""

    def __init__(self, words, ncons, b, S):
        self.words, self.ncons, self.b, self.S = words, ncons, b, S
        self.B = words.shape[0]


def check_options(model, opt):
    """the refusals of a sample call with opt['constraints'] that do not depend on the constraints -> beam_size"""
    if getattr(model, '_cbs_refusal', None) is not None:
        raise NotImplementedError("opt['constraints'] (constrained beam search) is not implemented for %s: %s"
                                  % (type(model).__name__, model._cbs_refusal))
    if model.training:
        raise NotImplementedError("opt['constraints'] is a test-time option: call model.eval() first")
    if int(opt.get('group_size', 1)) > 1:
        raise NotImplementedError("opt['constraints'] does not support group_size > 1: the beams are already grouped, by the "
                                  'constraints they have satisfied')
    if opt.get('block_trigrams', 0):
        raise NotImplementedError("opt['constraints'] does not support block_trigrams: the blocking reads a hypothesis's whole "
                                  'history, which a beam keeps as parent pointers until the search has ended')
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError("output_logsoftmax=0 is implemented for the sampled / greedy rollout; opt['constraints'] "
                                  'returns log-probabilities')
    if int(opt.get('sample_n', 1)) > 1:
        raise NotImplementedError("opt['constraints'] returns one caption per image: sample_n = 1, got %d" % int(opt.get('sample_n', 1)))
    method = opt.get('sample_method', 'greedy')
    if method not in ('greedy', 'beam_search'):
        raise NotImplementedError("opt['constraints'] is a beam search: sample_method 'greedy' or 'beam_search', got %r" % (method,))
    b = int(opt.get('beam_size', 1))
    if b < 1:
        raise ValueError("opt['constraints'] needs beam_size >= 1, got %d" % b)
    if not float(opt.get('temperature', 1.0)) > 0:
        raise ValueError("opt['constraints'] needs temperature > 0, got %r" % (opt.get('temperature'),))
    return b


def unk_column(model, opt, V1):
    """the column suppress_UNK pushes down by 1000 (beam.unk_column), -1: none"""
    if opt.get('suppress_UNK', 0) and hasattr(model, 'vocab') and model.vocab.get(str(V1 - 1)) == 'UNK':
        return V1 - 1
    if getattr(model, 'unk_idx', None) is not None:
        return int(model.unk_idx)
    return -1


def tables(constraints, V1, L, b, vocab=None, unk=-1):
    """constraints (see the module docstring) -> Request.  ValueError: more than C_MAX constraints, an empty set or one above W_MAX,
    S * b > SLOTS_MAX, L < C + 1, and -- all of them named in one message -- unknown words, token 0 or an id outside the vocabulary,
    the suppressed UNK column."""
    if not isinstance(constraints, (list, tuple)):
        raise ValueError("opt['constraints'] is a list with one list of constraints per image")
    B = len(constraints)
    inv = None
    words = torch.full((max(B, 1), C_MAX, W_MAX), -1, dtype=torch.int32)
    ncons = torch.zeros(max(B, 1), dtype=torch.int32)
    unknown, bad_ids, unk_hits = [], [], []
    for k, cons in enumerate(constraints):
        cons = [] if cons is None else list(cons)
        if len(cons) > C_MAX:
            raise ValueError("opt['constraints']: image %d has %d constraints, at most %d are supported" % (k, len(cons), C_MAX))
        for c, ws in enumerate(cons):
            ws = [ws] if isinstance(ws, (str, int)) else list(ws)
            if not ws:
                raise ValueError("opt['constraints']: constraint %d of image %d is empty" % (c, k))
            if len(ws) > W_MAX:
                raise ValueError("opt['constraints']: constraint %d of image %d lists %d words, at most %d are supported"
                                 % (c, k, len(ws), W_MAX))
            for j, w in enumerate(ws):
                if isinstance(w, str):
                    if inv is None:
                        inv = {v: int(i) for i, v in (vocab or {}).items()}
                    ix = inv.get(w)
                    if ix is None:
                        unknown.append(w)
                        continue
                else:
                    ix = int(w)
                if ix == unk and unk >= 0:
                    unk_hits.append(w)
                elif not 1 <= ix < V1:
                    bad_ids.append(w)
                else:
                    words[k, c, j] = ix
        ncons[k] = len(cons)
    msgs = []
    if unknown:
        msgs.append('words that are not in the vocabulary: %s' % ', '.join(repr(w) for w in sorted(set(unknown))))
    if bad_ids:
        msgs.append('ids outside [1, %d) (0 is the end token): %s' % (V1, ', '.join(repr(w) for w in bad_ids)))
    if unk_hits:
        msgs.append('the suppressed UNK column %d: %s' % (unk, ', '.join(repr(w) for w in unk_hits)))
    if msgs:
        raise ValueError("opt['constraints'] cannot be required: " + '; '.join(msgs))
    C = int(ncons.max()) if B else 0
    S = 1 << C
    if S * b > SLOTS_MAX:
        raise ValueError("opt['constraints']: %d constraints make S = %d states of beam_size = %d slots each, S * beam_size = %d > %d"
                         % (C, S, b, S * b, SLOTS_MAX))
    if L < C + 1:
        raise ValueError("opt['constraints']: a caption of L = %d words cannot hold %d required words and its end (L >= C + 1)" % (L, C))
    return Request(words[:B], ncons[:B], b, S)


def prepare(model, opt):
    """every refusal of a constrained call, before any device work -> Request"""
    b = check_options(model, opt)
    V1 = model.vocab_size + 1
    return tables(opt['constraints'], V1, model.seq_length, b, getattr(model, 'vocab', None), unk_column(model, opt, V1))


def publish(model, state, ncons, score):
    """model.last_cbs from the finalisation's outputs (device tensors)"""
    state = state.long()
    sat = torch.zeros_like(state)
    for c in range(C_MAX):
        sat += (state >> c) & 1
    model.last_cbs = dict(state=state, satisfied=sat, total=ncons.long(), score=score)
