"""Float64 restatement of the stochastic beam search (imagecaptioning/pytorch_amd/sbs.py, csrc/sbs.hip; Kool, van Hoof and Welling
2019): one selection step, the whole search over a TABLE decoder -- a decoder whose logits depend on the prefix alone, read from a
small random tree -- the importance weights, and the exact sampling-without-replacement probabilities of such a tree by brute force.
Not a test.  Everything is numpy, vectorised over the images (the host test runs 20 000 "images" at once)."""
import itertools

import numpy as np

LN2 = float(np.log(2.0))


def log1mexp(d):
    """log(1 - exp(d)), d <= 0"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(d > -LN2, np.log(-np.expm1(d)), np.log1p(-np.exp(d)))


def select_step(logp, phi, g, alive, gumbel, bd, step0=False, force_end=False):
    """logp, gumbel [B, cur, V1]; phi, g [B, cur]; alive [B, cur] bool -> dict of parent, token, phi, g, alive [B, bd] (by descending
    value, ties to the lower flat index) and gap [B]: the bd-th minus the (bd+1)-th candidate value (inf without a finite one)."""
    logp, gumbel, phi, g = (np.asarray(a, dtype=np.float64) for a in (logp, gumbel, phi, g))
    alive = np.asarray(alive).astype(bool)
    B, cur, V1 = logp.shape
    blocked = np.isneginf(logp)
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.where(blocked, -np.inf, phi[..., None] + logp + gumbel)
        Z = s.max(-1, keepdims=True)
        if step0:
            val = s.copy()
        else:
            u = g[..., None] - s + log1mexp(s - Z)
            val = g[..., None] - np.maximum(0.0, u) - np.log1p(np.exp(-np.abs(u)))
            bi, ji = np.indices((B, cur))
            val[bi, ji, s.argmax(-1)] = g                                   # exactly g at the arg-max
        val = np.where(blocked, -np.inf, val)
    child_phi = phi[..., None] + np.where(blocked, 0.0, logp)
    dead = ~alive
    val[dead] = -np.inf
    val[dead, 0] = g[dead]                                                  # one candidate: token 0, phi and g unchanged
    child_phi[dead] = phi[dead][:, None]
    flat = val.reshape(B, cur * V1)
    order = np.argsort(-flat, axis=1, kind='stable')                        # stable: equal values by the lower flat index
    top = order[:, :bd]
    parent, token = top // V1, top % V1
    rows = np.arange(B)[:, None]
    g_out = flat[rows, top]
    phi_out = child_phi.reshape(B, cur * V1)[rows, top]
    alive_out = alive[rows, parent] & (token != 0) & (not force_end)
    if cur * V1 > bd:
        nxt = flat[np.arange(B), order[:, bd]]
        with np.errstate(invalid='ignore'):
            gap = np.where(np.isneginf(nxt), np.inf, g_out[:, bd - 1] - nxt)
    else:
        gap = np.full(B, np.inf)
    return dict(parent=parent, token=token, phi=phi_out, g=g_out, alive=alive_out, gap=gap)


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def make_tree(V1, L, seed, scale=1.0):
    """logits of a table decoder: tree[t][w_0, .., w_{t-1}] is the [V1] row after that prefix"""
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(V1,) * (t + 1)) * scale for t in range(L)]


def tree_logp(tree, t, prefix, temperature=1.0):
    """prefix int [N, t] -> normalised rows [N, V1]"""
    rows = np.broadcast_to(tree[t][tuple(prefix[:, i] for i in range(t))], (prefix.shape[0], tree[0].shape[0]))
    return log_softmax(rows / temperature)


def search(tree, B, k, gumbel, temperature=1.0):
    """The whole search over a table decoder shared by the B images.  gumbel [L, B * k, V1] by search row (step 0 reads the first B
    rows).  -> seq [B * k, L], phi / g [B, k], min_gap (the smallest selection gap of any step and image)."""
    L, V1 = len(tree), tree[0].shape[0]
    prefix = np.zeros((B, 1, 0), dtype=np.int64)
    phi, g, alive = np.zeros((B, 1)), np.zeros((B, 1)), np.ones((B, 1), dtype=bool)
    rows = np.arange(B)[:, None]
    min_gap = np.inf
    for t in range(L):
        cur = prefix.shape[1]
        lp = tree_logp(tree, t, prefix.reshape(B * cur, t), temperature).reshape(B, cur, V1)
        r = select_step(lp, phi, g, alive, np.asarray(gumbel[t][:B * cur], dtype=np.float64).reshape(B, cur, V1), k, step0=t == 0,
                        force_end=t == L - 1)
        prefix = np.concatenate([prefix[rows, r['parent']], r['token'][..., None]], 2)
        phi, g, alive = r['phi'], r['g'], r['alive']
        min_gap = min(min_gap, float(r['gap'].min()))
    return dict(seq=prefix.reshape(B * k, L), phi=phi, g=g, min_gap=min_gap)


def log_weights(phi, g):
    """sbs.py's formulae, written out: kappa = g[:, k-1]; w_i = exp(phi_i) / (1 - exp(-exp(phi_i - kappa))), i < k - 1; normalised;
    the k-th caption -inf; k = 1: 0"""
    phi, g = np.asarray(phi, dtype=np.float64), np.asarray(g, dtype=np.float64)
    B, k = phi.shape
    if k == 1:
        return np.zeros((B, 1))
    kappa = g[:, k - 1:k]
    w = np.exp(phi[:, :k - 1]) / (1.0 - np.exp(-np.exp(phi[:, :k - 1] - kappa)))
    with np.errstate(divide='ignore'):
        return np.concatenate([np.log(w / w.sum(1, keepdims=True)), np.full((B, 1), -np.inf)], 1)


def backtrack(parent, token, alive):
    """numpy backtrack of the [L, B, bd] tables -> seq [B * bd, L], length [B * bd], lineage [L, B * bd] (capmi_beam_finalize's
    conventions: the search row of the ancestor at step t, b at step 0, -1 at and behind the end)"""
    L, B, bd = parent.shape
    seq = np.zeros((B * bd, L), dtype=np.int64)
    length = np.zeros(B * bd, dtype=np.int32)
    lineage = np.full((L, B * bd), -1, dtype=np.int32)
    for b in range(B):
        for j in range(bd):
            path, jj = [], j
            for s in range(L - 1, -1, -1):
                path.append((s, jj))
                jj = int(parent[s, b, jj])
            path.reverse()
            ln = next((s + 1 for s, q in path if not alive[s, b, q]), L)
            for s, q in path[:ln]:
                seq[b * bd + j, s] = token[s, b, q]
                lineage[s, b * bd + j] = b if s == 0 else b * bd + int(parent[s, b, q])
            length[b * bd + j] = ln
    return seq, length, lineage


# ---- the exact distribution of a tree ---------------------------------------------------------------------------------------------
def sequences(tree, temperature=1.0):
    """every complete sequence of the tree (token 0 ends one; the last step ends all), padded with 0 -> (seqs [n, L], p [n])"""
    L, V1 = len(tree), tree[0].shape[0]
    out = []

    def walk(prefix, lp):
        t = len(prefix)
        row = tree_logp(tree, t, np.array([prefix], dtype=np.int64).reshape(1, t), temperature)[0]
        for w in range(V1):
            if w == 0 or t == L - 1:
                out.append((prefix + [w] + [0] * (L - 1 - t), lp + row[w]))
            else:
                walk(prefix + [w], lp + row[w])
    walk([], 0.0)
    return np.array([s for s, _ in out], dtype=np.int64), np.exp(np.array([p for _, p in out]))


def inclusion_probabilities(p, k):
    """P(sequence i is among k draws without replacement), by enumerating every ordered k-tuple"""
    n = len(p)
    inc = np.zeros(n)
    for tup in itertools.permutations(range(n), k):
        q, rest = 1.0, 1.0
        for i in tup:
            q *= p[i] / rest
            rest -= p[i]
        for i in tup:
            inc[i] += q
    return inc


# ---- the table decoder on the device (step.py protocol) ---------------------------------------------------------------------------
class TableDecoder:
    """make_decoder for beam.stochastic_beam_search_steps: B images share the tree; the state of a row is its prefix"""

    def __init__(self, tree, B, rows_per_image, dev):
        import torch
        self.torch = torch
        self.tree = [torch.from_numpy(np.ascontiguousarray(t)).float().to(dev) for t in tree]
        self.B, self.cap, self.V1 = B, rows_per_image, tree[0].shape[0]
        self.prefix = torch.zeros(B, 0, dtype=torch.long, device=dev)

    def step(self, t, it, rows_per_image):
        if t > 0:
            self.prefix = self.torch.cat([self.prefix, it.view(-1, 1)], 1)
        assert self.prefix.shape == (self.B * rows_per_image, t)
        return self.tree[t][tuple(self.prefix[:, i] for i in range(t))].expand(self.prefix.shape[0], self.V1).contiguous()

    def reorder(self, parent, cur):
        B, bd = parent.shape
        src = (self.torch.arange(B, device=parent.device).view(B, 1) * cur + parent.long()).reshape(-1)
        self.prefix = self.prefix[src]
