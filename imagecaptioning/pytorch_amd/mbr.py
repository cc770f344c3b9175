"""Consensus (minimum-Bayes-risk) reranking of the n candidate captions of an image: ``opt['rerank'] = 'mbr_ciderd' | 'mbr_bleu4'``
on ``model(..., mode='sample')`` with ``sample_n = n``.

Of an image's n candidates -- drawn by any sample_n_method, or the n beams of a beam search -- the one is kept whose expected
utility against the other candidates is highest; the utility is CIDEr-D against the training document frequencies (the table
``rewards.init_scorer`` uploads for the CIDEr-D reward) or sentence BLEU-4, each exactly as the training rewards compute it with
one reference.  ``opt['rerank_prior'] = 'model'`` weighs every candidate by its own probability under the model (the softmax,
over the image, of the sums of the selected log-probs), ``'uniform'`` (the default) weighs them equally.

    utility(seq, n, kind, scorer)   capmi_mbr_utility: U [B, n, n] float64, U[g, i, j] = candidate i against candidate j as its reference
    select(U, seq, n, weight)       capmi_mbr_select: (expected [B, n] float64, choice [B] int32)
    rerank(seq, seq_logp, n, kind, prior)   the whole job -> dict(choice, expected, utility, candidates, candidate_logp_sum)
    check_options(model, opt) / apply(model, opt, out)   what CaptionModel.forward does around the sample call

Four launches (cook, pairs, select, and the log-prob sums), nothing is read back; with the option off none of it runs.
(csrc/mbr.hip; restated in float64 in tests/mbr_ref64.py.)
"""
import torch

from . import _lib
from ._lib import lib, ptr, check, stream_ptr

KINDS = {'mbr_ciderd': _lib.MBR_CIDERD, 'mbr_bleu4': _lib.MBR_BLEU4}
PRIORS = ('uniform', 'model')
NMAX = _lib.SELF_CIDER_NMAX


def wanted(opt):
    return bool(opt.get('rerank', '')) if opt else False


def _kind(kind):
    if kind not in KINDS:
        raise ValueError("rerank %r: choose one of '' (off), %s" % (kind, ', '.join(repr(k) for k in KINDS)))
    return KINDS[kind]


def _rows(seq, n):
    if seq.dim() != 2 or seq.dtype != torch.long or not seq.is_cuda:
        raise ValueError('the candidates are an int64 device tensor [B * n, L], got %s %s' % (seq.dtype, tuple(seq.shape)))
    N, L = seq.shape
    if not 2 <= n <= NMAX or N == 0 or N % n:
        raise ValueError('reranking needs 2 <= n <= %d candidates per image, got %d rows with n = %d' % (NMAX, N, n))
    if not 1 <= L <= _lib.LANGEVAL_LMAX:
        raise ValueError('candidates of 1..%d tokens, got %d' % (_lib.LANGEVAL_LMAX, L))
    return N // n, L


def utility(seq, n, kind, scorer=None):
    """U [B, n, n] float64 of seq int64 [B * n, L] (rows g*n .. g*n+n-1 the candidates of image g).  scorer: the DeviceCiderD whose
    table weighs the n-grams ('mbr_ciderd'; None: the one of rewards.init_scorer), unused for 'mbr_bleu4'."""
    code = _kind(kind)
    B, L = _rows(seq, n)
    seq = seq.contiguous()
    keys = vals = None
    cap, log_ref_len = 0, 0.0
    if code == _lib.MBR_CIDERD:
        scorer = scorer if scorer is not None else training_scorer()
        keys, vals, cap, log_ref_len = scorer.keys, scorer.vals, scorer.cap, scorer.log_ref_len
    scratch = torch.empty(B * n * _lib.CIDERD_COOKED_BYTES // 8, dtype=torch.int64, device=seq.device)
    U = torch.empty(B, n, n, dtype=torch.float64, device=seq.device)
    check(lib.capmi_mbr_utility(ptr(seq), B, n, L, code, ptr(keys), ptr(vals), cap, log_ref_len, ptr(scratch), ptr(U),
                                stream_ptr()), 'capmi_mbr_utility')
    return U


def select(U, seq, n, weight=None):
    """(expected [B, n] float64, choice [B] int32) from U [B, n, n]; weight: float64 [B * n] log-prior of each candidate or None."""
    B, L = _rows(seq, n)
    seq = seq.contiguous()
    if U.dtype != torch.float64 or tuple(U.shape) != (B, n, n) or not U.is_contiguous():
        raise ValueError('U is a contiguous float64 [B, n, n] = %s tensor, got %s %s' % ((B, n, n), U.dtype, tuple(U.shape)))
    if weight is not None and (weight.dtype != torch.float64 or weight.numel() != B * n or not weight.is_contiguous()):
        raise ValueError('weight is a contiguous float64 [B * n] tensor')
    expected = torch.empty(B, n, dtype=torch.float64, device=seq.device)
    choice = torch.empty(B, dtype=torch.int32, device=seq.device)
    check(lib.capmi_mbr_select(ptr(U), ptr(weight), ptr(seq), B, n, L, ptr(expected), ptr(choice), stream_ptr()),
          'capmi_mbr_select')
    return expected, choice


def logp_sum(seq, seq_logp):
    """float64 [N]: the sum of each row's selected log-probs over its kept steps (losses._shifted_mask: position 0 and every step
    behind a non-zero token).  seq_logp: the dense [N, L, V1] log-probs of a decode, or the [N, L] selected ones (diverse
    sampling returns those)."""
    sel = seq_logp if seq_logp.dim() == 2 else seq_logp.gather(2, seq.unsqueeze(2)).squeeze(2)
    kept = torch.cat([torch.ones_like(seq[:, :1], dtype=torch.bool), seq[:, :-1] > 0], 1)
    return torch.where(kept, sel.to(torch.float64), sel.new_zeros((), dtype=torch.float64)).sum(1)


def training_scorer():
    """the DeviceCiderD of rewards.init_scorer(opt.cached_tokens), found the way rewards.get_self_cider_scores finds it"""
    import sys
    from .captioning.utils import rewards
    # the entrypoints import the same file as the top-level package `captioning` (tools/ puts its parent on sys.path)
    for mod in (rewards, sys.modules.get('captioning.utils.rewards')):
        if mod is not None and getattr(mod, 'CiderD_scorer', None) is not None:
            return mod.CiderD_scorer
    raise ValueError("rerank='mbr_ciderd' weighs n-grams by the training document frequencies: call "
                     "rewards.init_scorer(opt.cached_tokens) first")


def rerank(seq, seq_logp, n, kind, prior='uniform', scorer=None):
    """seq int64 [B * n, L] and its log-probs -> dict(choice [B] int32, expected [B, n], utility [B, n, n], candidates [B * n, L],
    candidate_logp_sum [B * n] float64), all on the device."""
    if prior not in PRIORS:
        raise ValueError('rerank_prior %r: choose one of %s' % (prior, ', '.join(repr(p) for p in PRIORS)))
    seq = seq.long().contiguous()
    U = utility(seq, n, kind, scorer)
    sums = logp_sum(seq, seq_logp)
    expected, choice = select(U, seq, n, sums if prior == 'model' else None)
    return dict(choice=choice, expected=expected, utility=U, candidates=seq, candidate_logp_sum=sums)


def check_options(model, opt):
    """the refusals of a sample call with opt['rerank'], before any device work -> (kind, prior, n)"""
    kind, prior = opt.get('rerank', ''), opt.get('rerank_prior', 'uniform')
    _kind(kind)
    if prior not in PRIORS:
        raise ValueError('rerank_prior %r: choose one of %s' % (prior, ', '.join(repr(p) for p in PRIORS)))
    n = int(opt.get('sample_n', 1))
    if not 2 <= n <= NMAX:
        raise ValueError('rerank=%r chooses among the sample_n captions of an image: 2 <= sample_n <= %d, got %d' % (kind, NMAX, n))
    if model.training:
        raise NotImplementedError('rerank=%r is a test-time option: call model.eval() first' % kind)
    if KINDS[kind] == _lib.MBR_CIDERD:
        training_scorer()
    if int(opt.get('beam_size', 1)) > 1 and opt.get('sample_method', 'greedy') in ('greedy', 'beam_search'):
        beams = int(opt.get('beam_size', 1)) // max(int(opt.get('group_size', 1)), 1)
        if n != beams:
            raise ValueError('rerank=%r over the beams of a beam search needs sample_n == beam_size // group_size = %d (got %d): '
                             'any other sample_n returns one caption per image' % (kind, beams, n))
    return kind, prior, n


def gather_rows(t, choice, n):
    """rows g * n + choice[g] of t [B * n, ...]"""
    B = choice.shape[0]
    return t.index_select(0, torch.arange(B, device=choice.device) * n + choice.long())


def apply(model, opt, out):
    """(seq [B * n, L], seq_logp) of the decode -> the chosen rows (seq [B, L], seq_logp [B, L, V1]); publishes model.last_rerank
    and gathers model.last_attention to the same rows"""
    kind, prior, n = opt['rerank'], opt.get('rerank_prior', 'uniform'), int(opt['sample_n'])
    seq, seq_logp = out
    res = rerank(seq, seq_logp, n, kind, prior)
    model.last_rerank = res
    if model.last_attention is not None:
        model.last_attention = {k: gather_rows(v, res['choice'], n) for k, v in model.last_attention.items()}
    return gather_rows(res['candidates'], res['choice'], n), gather_rows(seq_logp, res['choice'], n)
