"""Float64 replay of constrained beam search (Anderson, Fernando, Johnson and Gould 2017), written from its definition; it imports
nothing of the package.

Per image: C <= 4 constraints, each a set of <= 8 token ids (words [C_MAX, W_MAX], padded with -1), satisfied once one of its
tokens has been emitted.  A hypothesis's state is the bitmask of its satisfied constraints; there is one beam of b slots per state,
slot = state * b + j, S states.  sat(v) = the mask of every constraint whose set holds v.

select_step: the candidates of target state s' are all (valid source slot r in state s, token v) with s | sat(v) == s' and a score
sums[r] + logp[r, v] > -inf; a source slot is valid when its sum is > -inf.  The b best per target state are kept, by descending
score, ties to the lower flat index r * V1 + v; the other slots are empty (valid 0, score / next_sums -inf, parent 0, token 0).
A kept candidate with token 0 -- every kept candidate under force_end -- is `ended`: it keeps its state and goes on 1000 lower.
finalize: of all recorded (ended, valid) candidates the best by (a) state == the image's full mask, else the larger popcount,
(b) the larger score / len_div[t], (c) the lower t, then the lower slot; its parents are walked back.
search: the whole search over a decoder given as a function of the prefix."""
import numpy as np

C_MAX, W_MAX = 4, 8


def sat_masks(words, ncons, V1):
    """words [C_MAX, W_MAX], ncons -> sat [V1] int"""
    sat = np.zeros(V1, dtype=np.int64)
    for c in range(int(ncons)):
        for v in words[c]:
            if v >= 0:
                sat[int(v)] |= 1 << c
    return sat


def select_step(logp, sums, words, ncons, b, S, force_end=False):
    """logp [B, cur, V1] (cur = 1: the root, state 0; else cur = S * b), sums [B, S * b] -> dict of [B, S * b] arrays parent, token,
    score, next_sums, ended, valid and gap [B, S]: the last kept score minus the first dropped one (inf where nothing was dropped)"""
    logp, sums = np.asarray(logp, dtype=np.float64), np.asarray(sums, dtype=np.float64)
    B, cur, V1 = logp.shape
    SB = S * b
    out = dict(parent=np.zeros((B, SB), np.int32), token=np.zeros((B, SB), np.int64), score=np.full((B, SB), -np.inf),
               next_sums=np.full((B, SB), -np.inf), ended=np.zeros((B, SB), bool), valid=np.zeros((B, SB), bool),
               gap=np.full((B, S), np.inf))
    for k in range(B):
        sat = sat_masks(words[k], ncons[k], V1)
        flat, sc, tg = [], [], []
        for r in range(cur):
            if not sums[k, r] > -np.inf:
                continue
            s = 0 if cur == 1 else r // b
            with np.errstate(invalid='ignore'):
                x = sums[k, r] + logp[k, r]
            ok = x > -np.inf
            v = np.flatnonzero(ok)
            flat.append(r * V1 + v)
            sc.append(x[v])
            tg.append(s | sat[v])
        if not flat:
            continue
        flat, sc, tg = np.concatenate(flat), np.concatenate(sc), np.concatenate(tg)
        for t in range(S):
            m = tg == t
            f, x = flat[m], sc[m]
            order = np.lexsort((f, -x))
            keep = order[:b]
            n = len(keep)
            o = slice(t * b, t * b + n)
            out['parent'][k, o] = f[keep] // V1
            out['token'][k, o] = f[keep] % V1
            out['score'][k, o] = x[keep]
            end = (f[keep] % V1 == 0) | bool(force_end)
            out['ended'][k, o] = end
            out['next_sums'][k, o] = np.where(end, x[keep] - 1000.0, x[keep])
            out['valid'][k, o] = True
            if len(order) > b:
                out['gap'][k, t] = x[order[b - 1]] - x[order[b]]
    return out


def popcount(s):
    return bin(int(s)).count('1')


def rank_key(state, full, key, t, slot):
    """sorts ascending to the best candidate first"""
    return (0 if state == full else 1, -popcount(state), -key, t, slot)


def finalize(parent, token, score, ended, valid, ncons, b, S, len_div=None):
    """tables [L, B, S * b] -> dict seq [B, L], lineage [L, B], length [B], state [B], score [B]"""
    L, B, SB = parent.shape
    out = dict(seq=np.zeros((B, L), np.int64), lineage=np.full((L, B), -1, np.int32), length=np.zeros(B, np.int32),
               state=np.zeros(B, np.int32), score=np.zeros(B))
    for k in range(B):
        full = (1 << int(ncons[k])) - 1
        best = None
        for t in range(L):
            for j in range(SB):
                if ended[t, k, j] and valid[t, k, j]:
                    key = float(score[t, k, j]) / (float(len_div[t]) if len_div is not None else 1.0)
                    cand = rank_key(j // b, full, key, t, j)
                    if best is None or cand < best:
                        best = cand
        if best is None:
            continue
        _, _, nkey, t, j = best
        out['length'][k], out['state'][k], out['score'][k] = t + 1, j // b, -nkey
        for s in range(t, -1, -1):
            out['seq'][k, s] = token[s, k, j]
            par = int(parent[s, k, j])
            out['lineage'][s, k] = k if s == 0 else k * SB + par
            j = par
    return out


def search(decoder, B, V1, L, words, ncons, b, S, len_div=None):
    """decoder(k, prefix tuple) -> log-probabilities [V1] of image k's next token.  Returns finalize()'s dict plus 'tables': the per-step arrays."""
    SB = S * b
    prefixes = [[()] for _ in range(B)]
    sums = np.zeros((B, SB))
    tabs = {n: [] for n in ('parent', 'token', 'score', 'ended', 'valid')}
    cur = 1
    for t in range(L):
        logp = np.zeros((B, cur, V1))
        for k in range(B):
            for r in range(cur):
                logp[k, r] = decoder(k, prefixes[k][r])
        st = select_step(logp, sums, words, ncons, b, S, force_end=t == L - 1)
        for n in tabs:
            tabs[n].append(st[n])
        prefixes = [[prefixes[k][st['parent'][k, j]] + (int(st['token'][k, j]),) for j in range(SB)] for k in range(B)]
        sums = st['next_sums']
        cur = SB
    tabs = {n: np.stack(v) for n, v in tabs.items()}
    out = finalize(tabs['parent'], tabs['token'], tabs['score'], tabs['ended'], tabs['valid'], ncons, b, S, len_div)
    out['tables'] = tabs
    return out
