"""Host-stepped samplers for the decode-time options the one-call rollouts have no hooks for (evaluation only, no gradient):

    sample_steps          AttModel._sample           AttModel.py:258-352  decoding_constraint, remove_bad_endings,
                                                                          block_trigrams (+ every sample_method)
    diverse_sample_steps  AttModel._diverse_sample   AttModel.py:354-447  group_size > 1 without beam search

    contrastive_steps     (none: Su et al. 2022)                          sample_method 'contrastive'

All drive a stepper (step.py protocol; any model family) and keep every per-step edit on the device: normalisation,
constraints (capmi_decode_constrain), group penalties (capmi_column_penalty) and the token choice
(capmi_select_logp) are kernels of libcapmi, the finished flags never leave the device, there is no `.item()` in the loop.
Results follow the reference value for value, including its quirks (noted inline).
"""
import ctypes as C

import torch

from . import _lib, logits_proc
from ._lib import lib, ptr, check, stream_ptr

_f32 = torch.float32
_MODES = {'greedy': 0, 'sample': 1}


def wants_options(opt):
    """True when `opt` asks for something only the host-stepped samplers implement."""
    return bool(opt.get('decoding_constraint', 0) or opt.get('block_trigrams', 0) or opt.get('remove_bad_endings', 0)
                or opt.get('group_size', 1) > 1 or truncation(opt) is not None or contrastive(opt) or logits_proc.wanted(opt))


_KINDS = {'minp': _lib.TRUNCATE_MINP, 'eps': _lib.TRUNCATE_EPS, 'eta': _lib.TRUNCATE_ETA, 'typ': _lib.TRUNCATE_TYP}


def truncation(opt):
    """(rule, parameter) when opt['sample_method'] names min-p, epsilon, eta or typical sampling, else None"""
    from .captioning.models.utils import parse_truncation
    return parse_truncation(opt.get('sample_method', 'greedy')) if opt else None


def check_truncation(model, opt):
    """the refusals of a sample call with a truncation rule, before any device work"""
    if truncation(opt) is None:
        return
    name = opt['sample_method']
    if model.training:
        raise NotImplementedError('sample_method %r is a test-time option: call model.eval() first' % name)
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError('output_logsoftmax=0 is only used by margin structure losses; sample_method %r truncates '
                                  'log-probabilities' % name)


def contrastive(opt):
    """True when opt['sample_method'] names contrastive search"""
    return bool(opt) and opt.get('sample_method', 'greedy') == 'contrastive'


def contrastive_params(opt):
    """(penalty_alpha, contrastive_k) of a contrastive-search call, range-checked"""
    alpha, k = opt.get('penalty_alpha', 0.6), opt.get('contrastive_k', 4)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0 <= alpha <= 1:
        raise ValueError("sample_method 'contrastive': penalty_alpha must satisfy 0 <= alpha <= 1, got %r" % (alpha,))
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.CONTRASTIVE_KMAX:
        raise ValueError("sample_method 'contrastive': contrastive_k must be an integer in [1, %d], got %r" % (_lib.CONTRASTIVE_KMAX, k))
    return float(alpha), int(k)


def check_contrastive(model, opt):
    """the refusals of a sample call with sample_method 'contrastive', before any device work"""
    if not contrastive(opt):
        return
    name = "sample_method 'contrastive'"
    if model.training:
        raise NotImplementedError('%s is a test-time option: call model.eval() first' % name)
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError('output_logsoftmax=0 is only used by margin structure losses; %s scores the candidates by their '
                                  'probabilities' % name)
    refusal = getattr(model, '_contrastive_refusal', None)
    if refusal is not None:
        raise NotImplementedError('%s is not implemented for %s: %s' % (name, type(model).__name__, refusal))
    if int(opt.get('sample_n', 1)) > 1:
        raise ValueError('%s is deterministic: sample_n = %d would return n identical rows per image' % (name, opt['sample_n']))
    if opt.get('beam_size', 1) > 1:
        raise ValueError('%s is a search of its own (one look-ahead step over contrastive_k candidates): beam_size must be 1, got %r'
                         % (name, opt['beam_size']))
    if opt.get('group_size', 1) > 1:
        raise ValueError('%s has no groups: group_size must be 1, got %r' % (name, opt['group_size']))
    contrastive_params(opt)
    if float(opt.get('temperature', 1.0)) != 1.0:
        raise ValueError("%s scores the candidates by the model's own probabilities: temperature must be 1, got %r"
                         % (name, opt['temperature']))
    if opt.get('distractors') is not None:
        raise NotImplementedError("%s with opt['distractors']: the pragmatic row of discriminative decoding mixes 1 + D decoder rows "
                                  'and has no single hidden state' % name)
    if opt.get('constraints') is not None:
        raise NotImplementedError("%s with opt['constraints']: constrained decoding is a beam search" % name)
    if opt.get('return_attention', 0):
        raise NotImplementedError('%s with return_attention: the recorder layout assumes one row per caption per step, the '
                                  'look-ahead steps contrastive_k' % name)


def _truncate(trunc, x, q, rows, V1, temperature, store, store_ld, unf, st):
    """q = the renormalised truncated distribution of the rows of x (capmi_truncate_rows); store: the rows of x times the flags"""
    check(lib.capmi_truncate_rows(ptr(x), V1, ptr(q), V1, rows, V1, _KINDS[trunc[0]], float(trunc[1]), float(temperature), None,
                                  None, store, store_ld, unf, st), 'capmi_truncate_rows')


def _filter(top_k, top_p):
    return C.byref(_lib.SampleFilter(int(top_k), float(top_p))) if (top_k or top_p) else None


def _flags(opt, t):
    f = 0
    if t > 0 and opt.get('decoding_constraint', 0):
        f |= _lib.DECODE_NO_REPEAT
    if t > 0 and opt.get('remove_bad_endings', 0):
        f |= _lib.DECODE_NO_BAD_ENDING
    if t >= 3 and opt.get('block_trigrams', 0):
        f |= _lib.DECODE_BLOCK_TRIGRAMS
    return f


def _prev(seq, t):
    """address of seq[0, t-1] (int64 rows of length L): the previous token of every row with stride L."""
    return seq.data_ptr() + 8 * (t - 1) if t > 0 else None


def sample_steps(model, stepper, B, L, opt, dev, seed=0):
    """Returns (seq [B*sample_n, L] int64, seqLogprobs [B*sample_n, L, V1])."""
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError('output_logsoftmax=0 is only used by margin structure losses')
    from .captioning.models.utils import parse_sample_method
    n = int(opt.get('sample_n', 1))
    mode, temperature, top_k, top_p = parse_sample_method(opt.get('sample_method', 'greedy'), opt.get('temperature', 1.0))
    V1 = stepper.V1
    N = B * n
    seq = torch.zeros(N, L, dtype=torch.long, device=dev)
    seq_logp = torch.zeros(N, L, V1, dtype=_f32, device=dev)
    it = torch.zeros(N, dtype=torch.long, device=dev)                       # BOS
    unf = torch.ones(N, dtype=torch.uint8, device=dev)
    logp = torch.empty(N, V1, dtype=_f32, device=dev)
    bad = torch.tensor(sorted(getattr(model, 'bad_endings_ix', [])), dtype=torch.long, device=dev)
    gumbel = opt.get('_gumbel')                                              # test hook: injected noise [L,N,V1]
    flt = _filter(top_k, top_p)
    trunc = truncation(opt)
    q = torch.empty(N, V1, dtype=_f32, device=dev) if trunc else None
    any_flags = False
    proc = logits_proc.make(opt, L)                                          # None: the four options are at their defaults
    st = stream_ptr()
    for t in range(L):
        logits = stepper.step(t, it, n)
        check(lib.capmi_log_softmax_rows(ptr(logits), ptr(logp), N, V1, st), 'capmi_log_softmax_rows')
        flags = _flags(opt, t)
        if flags:
            any_flags = True
            # block_trigrams: the reference loops over range(batch_size) = the IMAGE count, so with sample_n > 1 only the
            # first B rows are ever blocked (AttModel.py:310, 322); kept
            check(lib.capmi_decode_constrain(ptr(logp), N, V1, _prev(seq, t), L, flags, ptr(bad), bad.numel(), ptr(seq), L, t, B,
                                             st), 'capmi_decode_constrain')
        if proc is not None:
            any_flags = True
            proc.dense(logp, N, V1, t, seq, n)                               # all N rows, each from its own history seq[:, :t]
        if trunc:
            # the rule on softmax(logp / T), then a plain draw from q; seqLogprobs keeps the constrained rows, as for every sampler
            _truncate(trunc, logp, q, N, V1, temperature, seq_logp.data_ptr() + 4 * t * V1, L * V1, ptr(unf), st)
            check(lib.capmi_select_logp(ptr(q), N, V1, t, L, 1, 1.0, None if gumbel is None else ptr(gumbel[t]),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(seq), L, ptr(it), ptr(unf), None, None, 0, None, st),
                  'capmi_select_logp')
            continue
        check(lib.capmi_select_logp(ptr(logp), N, V1, t, L, _MODES[mode], float(temperature),
                                    None if gumbel is None else ptr(gumbel[t]), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(seq), L,
                                    ptr(it), ptr(unf), ptr(seq_logp), None, 0, flt, st), 'capmi_select_logp')
    if any_flags:
        # the reference leaves the loop once every row has finished (AttModel.py:350-351), so later columns stay zero; here
        # the loop always runs L steps and finished rows hold logprobs * 0 (NaN where a constraint put -inf): blank the
        # columns the reference never wrote.  Device-side, no sync.
        alive = (seq != 0).cumprod(1).any(0)                                 # some row unfinished after step t
        written = torch.cat([alive.new_ones(1), alive[:-1]])
        seq_logp = torch.where(written.view(1, L, 1), seq_logp, torch.zeros((), dtype=_f32, device=dev))
    return seq, seq_logp


def diverse_sample_steps(model, stepper, B, L, opt, dev, seed=0):
    """AttModel._diverse_sample: group g is penalised in every column any row of groups < g picked at the same step.
    All groups advance together (one decoder step on B*group_size rows); the reference's time stagger only exists so that
    the earlier groups' choices at step t are known, which they are here because the groups choose in order.
    Returns (seq [B*group_size, L], seqLogprobs [B*group_size, L]) -- 2-D log-probs, as the reference does."""
    from .captioning.models.utils import parse_sample_method
    G = int(opt.get('group_size', 1))
    lam = float(opt.get('diversity_lambda', 0.5))
    temperature = float(opt.get('temperature', 1.0))
    mode, _, top_k, top_p = parse_sample_method(opt.get('sample_method', 'greedy'), 1.0)   # sample_next_word(.., 1): :434
    V1 = stepper.V1
    N = B * G
    seq_tab = torch.zeros(G, B, L, dtype=torch.long, device=dev)
    slp_tab = torch.zeros(G, B, L, dtype=_f32, device=dev)
    it_tab = torch.zeros(G, B, dtype=torch.long, device=dev)
    unf = torch.ones(G, B, dtype=torch.uint8, device=dev)
    logp_all = torch.empty(N, V1, dtype=_f32, device=dev)
    lp = torch.empty(G, B, V1, dtype=_f32, device=dev)
    bad = torch.tensor(sorted(getattr(model, 'bad_endings_ix', [])), dtype=torch.long, device=dev)
    gumbel = opt.get('_gumbel')                                              # test hook [L,G,B,V1]
    flt = _filter(top_k, top_p)
    trunc = truncation(opt)
    q = torch.empty(B, V1, dtype=_f32, device=dev) if trunc else None
    st = stream_ptr()
    for t in range(L):
        it = it_tab.t().reshape(N)                                           # rows image-major: b*G + g
        logits = stepper.step(t, it.contiguous(), G)
        # F.log_softmax(get_logprobs_state(..) / temperature) (:388-389)
        check(lib.capmi_beam_logsoftmax(ptr(logits), ptr(logp_all), N, V1, temperature, -1, st), 'capmi_beam_logsoftmax')
        lp.copy_(logp_all.view(B, G, V1).transpose(0, 1))
        for g in range(G):
            x = lp[g]
            for pg in range(g):                                              # :392-397
                check(lib.capmi_column_penalty(ptr(x), B, V1, seq_tab[pg].data_ptr() + 8 * t, B, L, lam, st),
                      'capmi_column_penalty')
            flags = _flags(opt, t)
            if flags:
                check(lib.capmi_decode_constrain(ptr(x), B, V1, _prev(seq_tab[g], t), L, flags, ptr(bad), bad.numel(),
                                                 ptr(seq_tab[g]), L, t, B, st), 'capmi_decode_constrain')
            if trunc:
                # per group, after the column penalties; T = 1, the rows are tempered already.  sel_logp = q[token], the nucleus
                # convention (CaptionModel.py:396-398)
                _truncate(trunc, x, q, B, V1, 1.0, None, 0, None, st)
            check(lib.capmi_select_logp(ptr(q if trunc else x), B, V1, t, L, _MODES[mode], 1.0, None if gumbel is None else ptr(gumbel[t, g]),
                                        (int(seed) + 0x9E3779B97F4A7C15 * g) & 0xFFFFFFFFFFFFFFFF, ptr(seq_tab[g]), L,
                                        ptr(it_tab[g]), ptr(unf[g]), None, ptr(slp_tab[g]), 1, flt, st), 'capmi_select_logp')
    return seq_tab.transpose(0, 1).reshape(N, L), slp_tab.transpose(0, 1).reshape(N, L)


def contrastive_steps(model, stepper, B, L, opt, dev):
    """Contrastive search (Su et al. 2022) on a stepper made with rows_per_image_max = contrastive_k.  Per generated token: the
    constraints, capmi_contrastive_topk on the N rows, the reorder that fans the chosen state out to the k rows of every image, ONE
    decoder step on the N * k candidate rows (the look-ahead: its pre-logit rows are the candidates' hidden states, its logits the
    next step's), capmi_contrastive_select, and the gather + log-softmax of the chosen rows' logits -- plus the BOS step on N rows.
    Returns (seq [B, L] int64, seqLogprobs [B, L, V1])."""
    alpha, k = contrastive_params(opt)
    V1, R, N = stepper.V1, stepper.R, B
    if k > V1:
        raise ValueError("sample_method 'contrastive': contrastive_k = %d exceeds the %d vocabulary rows" % (k, V1))
    from . import beam
    S = L + 1
    i32 = torch.int32
    seq = torch.zeros(N, L, dtype=torch.long, device=dev)
    seq_logp = torch.zeros(N, L, V1, dtype=_f32, device=dev)
    it = torch.zeros(N, dtype=torch.long, device=dev)                       # BOS
    unf = torch.ones(N, dtype=torch.uint8, device=dev)
    logp = torch.empty(N, V1, dtype=_f32, device=dev)
    picked = torch.empty(1, N, V1, dtype=_f32, device=dev)                   # the chosen candidates' logits
    hist = torch.empty(N, S, R, dtype=_f32, device=dev)
    hist_inv = torch.empty(N, S, dtype=_f32, device=dev)
    tok = torch.empty(N, k, dtype=torch.long, device=dev)
    tok_logp = torch.empty(N, k, dtype=_f32, device=dev)
    choice = torch.zeros(N, 1, dtype=i32, device=dev)
    parent = torch.empty(N, dtype=i32, device=dev)
    fan = torch.zeros(N, k, dtype=i32, device=dev)                           # zeros: the first reorder fans row b out to b * k + j
    bad = torch.tensor(sorted(getattr(model, 'bad_endings_ix', [])), dtype=torch.long, device=dev)
    st = stream_ptr()

    def select(h, rows_k, hist_len, t, with_tokens):
        # no `it` output: the look-ahead step takes its tokens from the top-k table, `it` feeds the BOS step alone
        check(lib.capmi_contrastive_select(ptr(tok) if with_tokens else None, ptr(tok_logp) if with_tokens else None, ptr(h),
                                           h.stride(0), ptr(hist), ptr(hist_inv), N, rows_k, R, S, hist_len, t, L, alpha,
                                           ptr(choice), ptr(parent), ptr(fan) if with_tokens else None,
                                           ptr(seq) if with_tokens else None, L, None,
                                           ptr(unf) if with_tokens else None, st), 'capmi_contrastive_select')

    logits = stepper.step(0, it, 1)
    select(stepper.hidden(N), 1, 0, 0, False)                                # h_0 and its inverse norm
    check(lib.capmi_log_softmax_rows(ptr(logits), ptr(logp), N, V1, st), 'capmi_log_softmax_rows')
    any_flags = False
    for t in range(L):
        flags = _flags(opt, t)
        if flags:
            any_flags = True
            check(lib.capmi_decode_constrain(ptr(logp), N, V1, _prev(seq, t), L, flags, ptr(bad), bad.numel(), ptr(seq), L, t, B,
                                             st), 'capmi_decode_constrain')
        check(lib.capmi_contrastive_topk(ptr(logp), V1, N, V1, k, ptr(unf), ptr(tok), ptr(tok_logp),
                                         seq_logp.data_ptr() + 4 * t * V1, L * V1, st), 'capmi_contrastive_topk')
        stepper.reorder(fan, 1 if t == 0 else k)                             # row i * cur + c -> all of i * k .. i * k + k - 1
        logits_k = stepper.step(t + 1, tok.view(N * k), k)
        select(stepper.hidden(N * k), k, t + 1, t, True)
        if t + 1 < L:
            beam.reorder_rows(logits_k.view(1, N * k, V1), picked, choice, N, k, 1)
            check(lib.capmi_log_softmax_rows(ptr(picked), ptr(logp), N, V1, st), 'capmi_log_softmax_rows')
    if any_flags:
        # as in sample_steps: blank the columns the reference's loop would have left before writing them
        alive = (seq != 0).cumprod(1).any(0)
        written = torch.cat([alive.new_ones(1), alive[:-1]])
        seq_logp = torch.where(written.view(1, L, 1), seq_logp, torch.zeros((), dtype=_f32, device=dev))
    return seq, seq_logp
