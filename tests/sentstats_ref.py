"""eval_utils.language_eval's counting numbers, restated twice (eval_utils.py:31-36 count_bad, :55-68 novel_sentences and
vocab_size, :121 bad_count_rate; :79-80 the means):

  on_strings  as the reference writes them: captions decoded with misc.decode_sequence, Python sets of strings.  The reference's
              training sentences are the RAW tokens of the dataset file, which spell a rare word out where the label file holds the
              id of 'UNK'; `raw_word` stands for such a word (any string outside the vocabulary does).
  on_ids      on tuples of ids: a training row that holds unk_id is left out, a generated one that holds it is novel.

Both return the same dict: the integer counts ('rows', 'distinct', 'novel', 'vocab_size', 'first', 'bad') and the ratios the
reference reports ('novel_sentences', 'bad_count_rate'; 'novel_sentences' and 'vocab_size' only when there are rows, :54).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'imagecaptioning', 'pytorch_amd')

# eval_utils.py:27-28
BAD_ENDINGS = ['a', 'an', 'the', 'in', 'for', 'at', 'of', 'with', 'before', 'after', 'on', 'upon', 'near', 'to', 'is', 'are', 'am']
BAD_ENDINGS += ['the']


def count_bad(sen):
    """eval_utils.py:31-36"""
    sen = sen.split(' ')
    return 1 if sen[-1] in BAD_ENDINGS else 0


def _decode(ix_to_word, rows):
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from captioning.utils import misc
    rows = np.asarray(rows, dtype=np.int64)
    return misc.decode_sequence(ix_to_word, rows) if rows.size else []


def _finish(out, n_rows, n_first):
    if n_rows > 0:
        out['novel_sentences'] = float(out['novel']) / n_rows
    else:
        del out['vocab_size']
    out['bad_count_rate'] = out['bad'] / float(n_first) if n_first else 0.0
    return out


def strings_stats(training_sentences, captions_n, captions_first):
    """eval_utils.py:55-68, 121 on what the reference holds: the set of training strings, the captions of preds_n and of preds"""
    preds_n = [{'caption': s} for s in captions_n]
    generated_sentences = set([_['caption'] for _ in preds_n])                           # :61
    novels = generated_sentences - training_sentences                                    # :62
    tmp = [_.split() for _ in generated_sentences]                                       # :64-68
    words = []
    for _ in tmp:
        words += _
    out = {'rows': len(preds_n), 'distinct': len(generated_sentences), 'novel': len(novels), 'vocab_size': len(set(words)),
           'first': len(captions_first), 'bad': sum(count_bad(s) for s in captions_first)}        # :121
    return _finish(out, len(preds_n), len(captions_first))


def training_strings(ix_to_word, train_rows, raw_word='zyzzyva'):
    """the reference's set of training sentences (:60) from label rows: the id of 'UNK' stands for a word the raw tokens spell out"""
    assert raw_word not in ix_to_word.values()
    raw = {k: (raw_word if v == 'UNK' else v) for k, v in ix_to_word.items()}
    return set(_decode(raw, train_rows))


def on_strings(ix_to_word, train_rows, rows_n, rows_first, raw_word='zyzzyva'):
    """train_rows / rows_n / rows_first: integer rows (0 = end and pad).  ix_to_word: {id string: word}, 'UNK' among them or not."""
    return strings_stats(training_strings(ix_to_word, train_rows, raw_word), _decode(ix_to_word, rows_n),
                         _decode(ix_to_word, rows_first))


def sentence(row):
    """the ids of a row before its first 0"""
    out = []
    for t in row:
        if int(t) <= 0:
            break
        out.append(int(t))
    return tuple(out)


def on_ids(train_rows, rows_n, rows_first, unk_id, bad_ix):
    """unk_id: 0 / None when the vocabulary has no 'UNK'; bad_ix: the ids of the bad endings"""
    unk = int(unk_id or 0)
    bad_ix = set(int(i) for i in bad_ix)
    training = set(s for s in map(sentence, train_rows) if not (unk and unk in s))
    gen = [sentence(r) for r in rows_n]
    generated = set(gen)
    novels = set(s for s in generated if s not in training or (unk and unk in s))
    first = [sentence(r) for r in rows_first]
    out = {'rows': len(gen), 'distinct': len(generated), 'novel': len(novels), 'vocab_size': len(set(t for s in generated for t in s)),
           'first': len(first), 'bad': sum(1 for s in first if s and s[-1] in bad_ix)}
    return _finish(out, len(gen), len(first))


def means(perplexity, entropy):
    """eval_utils.py:79-80 in float64"""
    p, e = np.asarray(perplexity, dtype=np.float64), np.asarray(entropy, dtype=np.float64)
    return float(p.sum() / len(p)), float(e.sum() / len(e))
