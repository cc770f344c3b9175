"""The semantics of the logits processors (no_repeat_ngram_size, repetition_penalty, min_length, bad_words), restated in plain
Python / numpy.  Nothing else defines them: the kernel (csrc/logits_proc.hip) is tested bit for bit against process()."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def process(row, history, t, L, opts, exempt=()):
    """row [V1] float32 log-probabilities of step t, history = the t tokens the row has emitted -> the edited row (a copy).
    opts: no_repeat_ngram_size n, repetition_penalty theta, min_length m, bad_words (lists of ids).  exempt: words the n-gram
    rule spares (constrained beam search: the image's constraint words)."""
    row = np.array(row, dtype=np.float32, copy=True)
    h = [int(v) for v in history[:t]]
    V1 = row.shape[0]
    if 0 in h:                                                   # a finished row is left untouched
        return row
    n, theta, m = opts.get('no_repeat_ngram_size', 0), opts.get('repetition_penalty', 1.0), opts.get('min_length', 0)
    if theta > 1:
        for v in sorted(set(h)):                                 # once per distinct word; h holds no 0 here
            row[v] = row[v] * np.float32(theta)                  # one float32 multiply
    if t < min(m, L - 1):
        row[0] = NEG_INF
    if n >= 1 and t >= n - 1:
        last = h[t - (n - 1):]                                   # the n - 1 words the next one would follow ([] for n = 1)
        for i in range(0, t - n + 1):
            v = h[i + n - 1]
            if h[i:i + n - 1] == last and v != 0 and v not in exempt:
                row[v] = NEG_INF
    for ids in opts.get('bad_words') or []:
        k = len(ids)
        if t >= k - 1 and h[t - (k - 1):] == [int(i) for i in ids[:-1]] and 0 < ids[-1] < V1:
            row[ids[-1]] = NEG_INF
    return row


def history_from_parents(tokens, parents, t, row):
    """The history of search row `row` at step t from the search core's tables tokens / parents [L, B, W] (numpy): at t > 0 the rows
    of an image are the W slots of step t - 1, row = b * W + j; at t = 0 the history is empty."""
    if t == 0:
        return []
    W = tokens.shape[2]
    b, slot = divmod(row, W)
    h = []
    for s in range(t - 1, -1, -1):
        h.append(int(tokens[s, b, slot]))
        slot = int(parents[s, b, slot])
    return h[::-1]
