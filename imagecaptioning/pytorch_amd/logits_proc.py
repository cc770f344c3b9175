"""Decode-time logits processors: four options of a sample call that edit the [rows, V1] log-probability rows of every step from the
row's own history, on the device (capmi_logits_process, csrc/logits_proc.hip; one launch per step, only when an option is on).

    opt['no_repeat_ngram_size'] = n   0 (off) .. 8: a word that would complete an n-gram the row already holds gets -inf (n = 1:
                                      every word already emitted), from step n - 1 on
    opt['repetition_penalty'] = th    1.0 (off) or > 1: logp[v] *= th, once per distinct word of the history
    opt['min_length'] = m             0 (off): the end token gets -inf while t < min(m, L - 1)
    opt['bad_words']                  <= 16 sequences of <= 4 token ids >= 1: a one-word entry is always at -inf, a longer one has
                                      its last word at -inf whenever the history ends with the words before it

Within a step they come after the existing edits (suppress_UNK, decoding_constraint, remove_bad_endings, block_trigrams): the
penalty first, then the three -inf rules.  The end token is never touched by the n-gram rule, the penalty or bad_words, and a
finished row (its history holds the end token) is left as it is.  The stored log-probabilities are the edited rows; nothing is
renormalised except where the path renormalises edited rows anyway (sbs, the truncation samplers).

The history is read where the decoder keeps it: the dense seq of decode.sample_steps, or the parent / token tables of the search
core (beam.py _search_loop) for beam, stochastic and constrained beam search -- the kernel walks the parents back itself.  In a
constrained beam search the n-gram rule never blocks a word of the image's constraint lists (a required word stays reachable).
"""
import ctypes as C

from . import _lib
from ._lib import lib, ptr, check, stream_ptr

KEYS = ('no_repeat_ngram_size', 'repetition_penalty', 'min_length', 'bad_words')
NGRAM_MAX, BAD_MAX, BAD_LEN, HIST_MAX = _lib.LP_NGRAM_MAX, _lib.LP_BAD_MAX, _lib.LP_BAD_LEN, _lib.LP_HIST_MAX


def wanted(opt):
    """True when `opt` sets one of the four options to anything but its default"""
    if not opt:
        return False
    theta = opt.get('repetition_penalty', 1.0)
    return bool(opt.get('no_repeat_ngram_size', 0)) or (theta is not None and theta != 1.0) or bool(opt.get('min_length', 0)) \
        or bool(opt.get('bad_words'))


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def params(opt):
    """(n, theta, m, bad_words as a list of id lists), range-checked: ValueError"""
    n, theta, m = opt.get('no_repeat_ngram_size', 0) or 0, opt.get('repetition_penalty', 1.0), opt.get('min_length', 0) or 0
    theta = 1.0 if theta is None else theta
    if not _is_int(n) or not 0 <= n <= NGRAM_MAX:
        raise ValueError('no_repeat_ngram_size must be an integer in [0, %d], got %r' % (NGRAM_MAX, n))
    if isinstance(theta, bool) or not isinstance(theta, (int, float)) or not theta >= 1:
        raise ValueError('repetition_penalty must be a number >= 1 (1: off), got %r' % (theta,))
    if not _is_int(m) or m < 0:
        raise ValueError('min_length must be an integer >= 0, got %r' % (m,))
    bad = opt.get('bad_words') or []
    if not isinstance(bad, (list, tuple)):
        raise ValueError('bad_words is a list of token-id sequences, got %r' % (bad,))
    if len(bad) > BAD_MAX:
        raise ValueError('bad_words lists %d sequences, at most %d are supported' % (len(bad), BAD_MAX))
    out = []
    for e in bad:
        ids = [e] if _is_int(e) else list(e) if isinstance(e, (list, tuple)) else None
        if ids is None or not ids or not all(_is_int(i) for i in ids):
            raise ValueError('bad_words: an entry is a non-empty sequence of token ids, got %r' % (e,))
        if len(ids) > BAD_LEN:
            raise ValueError('bad_words: the sequence %r has %d ids, at most %d are supported' % (e, len(ids), BAD_LEN))
        if any(i == 0 for i in ids):
            raise ValueError('bad_words: the sequence %r holds id 0, the end token (use min_length to keep a caption from ending)' % (e,))
        if any(i < 1 for i in ids):
            raise ValueError('bad_words: token ids are >= 1, got %r' % (e,))
        out.append(ids)
    return int(n), float(theta), int(m), out


def check_options(model, opt):
    """every refusal of a sample call with one of the four options, before any device work"""
    if not wanted(opt):
        return
    params(opt)
    from . import beam, decode
    what = 'no_repeat_ngram_size / repetition_penalty / min_length / bad_words'
    if beam.wants_train_beam(model, opt):
        raise NotImplementedError('%s do not support train_beam_size > 1 (beam search in train mode with gradients): they are '
                                  'test-time options' % what)
    if model.training:
        raise NotImplementedError('%s are test-time options: call model.eval() first' % what)
    if not opt.get('output_logsoftmax', 1):
        raise NotImplementedError('output_logsoftmax=0 is only used by margin structure losses; %s edit log-probabilities' % what)
    if int(opt.get('group_size', 1)) > 1:
        raise NotImplementedError('%s do not support group_size > 1 (diverse sampling / diverse beam search): the groups keep '
                                  'their histories in tables of their own' % what)
    if decode.contrastive(opt):
        raise NotImplementedError("%s do not support sample_method 'contrastive': its look-ahead select is a different kernel" % what)
    L = getattr(model, 'seq_length', 0)
    if L > HIST_MAX:
        raise ValueError('%s keep a row\'s history in %d words of LDS: seq_length = %d is too long' % (what, HIST_MAX, L))


def refuse_score(opt):
    """mode='score' scores a GIVEN caption: nothing is decoded, so nothing can be blocked"""
    if wanted(opt):
        raise NotImplementedError("mode='score' does not support no_repeat_ngram_size / repetition_penalty / min_length / bad_words: "
                                  'a given caption is not edited')


def struct(n, theta, m, bad):
    """the capmi_logits_proc of checked parameters"""
    p = _lib.LogitsProc()
    p.no_repeat_ngram_size, p.repetition_penalty, p.min_length, p.n_bad = n, theta, m, len(bad)
    for e, ids in enumerate(bad):
        p.bad_len[e] = len(ids)
        for k, i in enumerate(ids):
            p.bad_words[e * BAD_LEN + k] = i
    return p


class Processor:
    """The options of one call, ready to launch.  dense(): the history is seq [rows, L]; search(): the search core's tables."""

    def __init__(self, opt, L):
        self.p = struct(*params(opt))
        self.ref = C.byref(self.p)
        self.L = int(L)

    def dense(self, logp, rows, V1, t, seq, cur=1):
        check(lib.capmi_logits_process(ptr(logp), V1, rows, V1, t, self.L, self.ref, ptr(seq), seq.shape[1], None, None, 0, cur,
                                       None, 0, stream_ptr()), 'capmi_logits_process')

    def search(self, logp, rows, V1, t, token, parent, cur, exempt=None):
        """token int64 / parent int32 [L, B, W]; rows = B * cur rows of step t (cur = 1 at t = 0, else W); exempt int32 [B, n]"""
        check(lib.capmi_logits_process(ptr(logp), V1, rows, V1, t, self.L, self.ref, None, 0, ptr(token), ptr(parent),
                                       token.shape[2], cur, ptr(exempt), 0 if exempt is None else exempt.shape[1], stream_ptr()),
              'capmi_logits_process')


def make(opt, L):
    """Processor of a call that wants one, else None: with the options at their defaults nothing is built and nothing is launched"""
    return Processor(opt, L) if wanted(opt) else None


def bad_words_from_file(path, vocab, oov='error'):
    """--bad_words_json: a JSON list of strings ("a man" / "man") or of word lists -> token-id sequences (bad_word_ids)"""
    import json
    with open(path) as f:
        entries = json.load(f)
    if not isinstance(entries, list):
        raise ValueError('%s: a JSON list of strings or of word lists is expected' % path)
    return bad_word_ids(entries, vocab, oov, path)


def bad_word_ids(entries, vocab, oov='error', path='--bad_words'):
    """strings ("a man" / "man") or word lists -> token-id sequences through `vocab` (ix -> word); ids pass through.
    Out-of-vocabulary words as --constraints_oov handles them: 'error' raises, 'drop' leaves the sequence out."""
    inv = {w: int(i) for i, w in (vocab or {}).items()}
    out, unknown = [], []
    for e in entries:
        words = e.split() if isinstance(e, str) else list(e)
        ids = [w if _is_int(w) else inv.get(w) for w in words]
        missing = [w for w, i in zip(words, ids) if i is None]
        if missing:
            unknown.extend(missing)
            continue
        if ids:
            out.append(ids)
    if unknown and oov != 'drop':
        raise ValueError('%s: words that are not in the vocabulary: %s (--constraints_oov drop leaves their sequences out)'
                         % (path, ', '.join(repr(w) for w in sorted(set(unknown)))))
    return out
