"""Device-resident CIDEr-D scorer (host side): builds the open-addressing document-frequency table
consumed by ``capmi_ciderd_score`` and wraps the launch.

Replaces ``CiderD(df=cached_tokens)`` + ``CiderD_scorer.compute_score`` as used by
captioning/utils/rewards.py:25-31, 64, 101 (external pyciderevalcap; see oracle/ciderd.py for the
provenance note: PARITY UNPINNED).  The pickle format is the one written by
scripts/prepro_ngrams.py:79-80: ``{'document_frequency': {tuple[str] -> count}, 'ref_len': int}``.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, check, stream_ptr

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(x):
    """splitmix64 finaliser on a uint64 array (twin of mix64 in csrc/ngram_metrics.h)."""
    x = x.copy()
    with np.errstate(over='ignore'):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xbf58476d1ce4e5b9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94d049bb133111eb)
        x ^= x >> np.uint64(31)
    return x


def pack_ngram(tokens):
    """<= 4 token ids (each < 65535) -> uint64 key: 16-bit fields of (id + 1), first token lowest."""
    k = 0
    for q, t in enumerate(tokens):
        t = int(t)
        assert 0 <= t < 65535
        k |= (t + 1) << (16 * q)
    return k


def table_cap(n, load_factor=0.5):
    """slots of the table of n distinct n-grams: the power of two (at least 16) that keeps the load at or below load_factor"""
    return 1 << max(4, int(math.ceil(math.log2(max(1, n) / load_factor))))


def build_table(document_frequency, load_factor=0.5):
    """dict {tuple[int|str] -> count} -> (keys uint64[cap], vals float64[cap]); empty slot = key 0.
    Vectorised linear-probing insertion (the COCO table has a few million n-grams)."""
    n = len(document_frequency)
    cap = table_cap(n, load_factor)
    keys = np.zeros(cap, dtype=np.uint64)
    vals = np.zeros(cap, dtype=np.float64)
    if n == 0:
        return keys, vals
    k = np.fromiter((pack_ngram([int(t) for t in g]) for g in document_frequency.keys()), dtype=np.uint64, count=n)
    v = np.fromiter((float(c) for c in document_frequency.values()), dtype=np.float64, count=n)
    slot = (_mix64(k) & np.uint64(cap - 1)).astype(np.int64)
    pending = np.arange(n)
    while pending.size:
        s = slot[pending]
        free = keys[s] == 0
        # among the candidates for the same free slot keep the first
        cand = pending[free]
        cs = slot[cand]
        _, first = np.unique(cs, return_index=True)
        win = cand[first]
        keys[slot[win]] = k[win]
        vals[slot[win]] = v[win]
        placed = np.zeros(n, dtype=bool)
        placed[win] = True
        pending = pending[~placed[pending]]
        slot[pending] = (slot[pending] + 1) & (cap - 1)
    return keys, vals


def save_df_image(document_frequency, ref_len, path):
    """One-time conversion of the scripts/prepro_ngrams.py pickle content into the flat hash image the
    kernel probes: an .npz with `keys` uint64[cap], `vals` float64[cap], `ref_len`.  Loading it is two array reads
    instead of unpickling and re-hashing a few million tuple keys at every start-up."""
    keys, vals = build_table(document_frequency)
    np.savez(path, keys=keys, vals=vals, ref_len=np.float64(ref_len), n=np.int64(len(document_frequency)))
    return path if str(path).endswith('.npz') else str(path) + '.npz'


def load_df_image(path):
    z = np.load(path)
    keys, vals = z['keys'], z['vals']
    if keys.dtype != np.uint64 or vals.dtype != np.float64 or keys.shape != vals.shape or keys.shape[0] & (keys.shape[0] - 1):
        raise ValueError('%s is not a capmi document-frequency image' % path)
    return keys, vals, float(z['ref_len'])


def save_table_image(keys, vals, ref_len, path):
    """save_df_image for a table that is already hashed (build_df_image): the same .npz layout, read by load_df_image"""
    np.savez(path, keys=keys, vals=vals, ref_len=np.float64(ref_len), n=np.int64(np.count_nonzero(keys)))
    return path if str(path).endswith('.npz') else str(path) + '.npz'


_DF_ERRORS = ((_lib.LANGEVAL_E_TABLE_FULL, 'table full: more distinct n-grams than slots'),
              (_lib.LANGEVAL_E_TOKEN, 'a token id outside [0, 65535)'),
              (_lib.DF_E_OFFSETS, 'malformed caption / image offsets'))


def _df_tables(tok, cap_off, img_off, device, count_cap=None):
    """The document-frequency image of a ragged corpus, built on the device (capmi_df_count + capmi_df_finalize, csrc/df_build.hip)
    -> (keys int64 [cap] holding the bits of uint64, vals float64 [cap], ref_len), device tensors.  One host read (error bits and
    the number of distinct n-grams, which sizes the image) between the two launches."""
    from . import ops
    dev = torch.device(device)

    def put(a, keep_int32=False):
        """-> (int64 device tensor -- int32 where kept --, the host array it came from or None)"""
        if torch.is_tensor(a) and a.is_cuda:
            return (a if keep_int32 and a.dtype == torch.int32 else a.to(torch.int64)).contiguous(), None
        a = a.numpy() if torch.is_tensor(a) else np.asarray(a)
        a = np.ascontiguousarray(a if keep_int32 and a.dtype == np.int32 else a.astype(np.int64))
        return torch.from_numpy(a).to(dev), a

    tok_d, _ = put(tok, keep_int32=True)
    cap_d, cap_h = put(cap_off)
    img_d, img_h = put(img_off)
    if tok_d.dim() != 1 or cap_d.dim() != 1 or img_d.dim() != 1 or cap_d.numel() < 1 or img_d.numel() < 1:
        raise ValueError('a corpus is tok [total_tokens], cap_off [n_caps + 1], img_off [n_img + 1]')
    # every token starts at most four n-grams: a counting table that the corpus cannot fill beyond one half
    count_cap = int(count_cap) if count_cap is not None else table_cap(4 * tok_d.numel())
    if count_cap < 1 or count_cap & (count_cap - 1) or count_cap > 1 << 31:
        raise ValueError('the counting table needs a power of two of slots, at most 2^31: got %d' % count_cap)
    ckeys = torch.zeros(count_cap, dtype=torch.int64, device=dev)
    counts = torch.zeros(count_cap, dtype=torch.int32, device=dev)
    meta = torch.zeros(2, dtype=torch.int32, device=dev)                 # error bits, distinct n-grams
    with torch.cuda.device(dev):
        ops.df_count(tok_d, cap_d, img_d, ckeys, counts, meta, cap_h, img_h)
        err, n = (int(x) for x in meta.tolist())                         # the one host read
        if err:
            raise _lib.CapmiError('capmi_df_count: ' + '; '.join(msg for bit, msg in _DF_ERRORS if err & bit))
        cap = table_cap(n)
        keys = torch.zeros(cap, dtype=torch.int64, device=dev)
        vals = torch.zeros(cap, dtype=torch.float64, device=dev)
        ops.df_finalize(ckeys, counts, keys, vals, meta)                 # cap >= 2 n: it cannot fill
    # scripts/prepro_ngrams.py:22 returns len(tmp.crefs), and cook_append adds an entry for every image of the split, one that
    # owns no caption included: ref_len is the number of images
    return keys, vals, float(img_d.numel() - 1)


def build_df_image(tok, cap_off, img_off, device=None, count_cap=None):
    """scripts/prepro_ngrams.py's document frequencies on the device -> (keys uint64 [cap], vals float64 [cap], ref_len), the host
    arrays load_df_image returns and save_table_image writes.  tok: the token ids of every caption back to back, each caption
    exactly as it counts (the caller appends the <eos> = 0; nothing is cut); cap_off [n_caps + 1]: where each caption starts;
    img_off [n_img + 1]: the first caption of each image (an image may own none).  Arrays, CPU tensors or device tensors; offsets
    given on the host are checked there.  cap is the size build_table gives the same number of distinct n-grams; the slots may
    differ from build_table's, a lookup does not see them."""
    device = device or torch.device('cuda', torch.cuda.current_device())
    keys, vals, ref_len = _df_tables(tok, cap_off, img_off, device, count_cap)
    return keys.cpu().numpy().view(np.uint64), vals.cpu().numpy(), ref_len


class PackedRefs(tuple):
    """(refs int32 [B,max_refs,w], n_refs int32 [B]) -- unpacks like the pair it used to be -- plus `.cooked`"""

    def __new__(cls, refs, n_refs, cooked=None):
        self = super().__new__(cls, (refs, n_refs))
        self.cooked = cooked
        return self


def nsc_advantage(scores, n, add=None, add_w=0.0):
    """new_self_critical's weights from float64 device scores [N] in one launch (capmi_nsc_advantage): (reward float32 [B,n] = the
    scores, adv float32 [N] = leave-one-out advantage + add_w * add[image]); add: float64 [B] or None."""
    N = scores.shape[0]
    assert scores.dtype == torch.float64 and scores.is_contiguous() and (add is None or (add.dtype == torch.float64 and add.is_contiguous()))
    buf = torch.empty(2, N, dtype=torch.float32, device=scores.device)
    check(lib.capmi_nsc_advantage(ptr(scores), ptr(add), float(add_w), N, n, ptr(buf), buf.data_ptr() + 4 * N, stream_ptr()),
          'capmi_nsc_advantage')
    return buf[0].view(-1, n), buf[1]


class DeviceCiderD:
    def __init__(self, document_frequency, ref_len, device, _table=None):
        keys, vals = _table if _table is not None else build_table(document_frequency)
        self.cap = int(keys.shape[0])
        self.keys = torch.from_numpy(keys.view(np.int64)).to(device)     # bit pattern preserved
        self.vals = torch.from_numpy(vals).to(device)
        self.log_ref_len = math.log(float(ref_len))
        self.device = device

    @classmethod
    def from_image(cls, path, device):
        keys, vals, ref_len = load_df_image(path)
        return cls(None, ref_len, device, _table=(keys, vals))

    @classmethod
    def from_corpus(cls, tok, cap_off, img_off, device, count_cap=None):
        """the scorer of a ragged caption corpus (build_df_image's arguments), its table built on the device and left there"""
        self = cls.__new__(cls)
        self.keys, self.vals, ref_len = _df_tables(tok, cap_off, img_off, device, count_cap)
        self.cap = int(self.keys.shape[0])
        self.log_ref_len = math.log(ref_len)
        self.device = device
        return self

    @classmethod
    def from_pickle(cls, path, device):
        import pickle
        with open(path, 'rb') as f:
            pkl = pickle.load(f, encoding='latin1')
        return cls(pkl['document_frequency'], pkl['ref_len'], device)

    def pack_refs(self, gts):
        """list (per image) of [n_ref_i, w] integer arrays -> (refs int32 [B,max_refs,w], n_refs int32 [B])."""
        B = len(gts)
        max_refs = max(len(g) for g in gts)
        w = max(np.asarray(g).shape[1] for g in gts)
        refs = np.zeros((B, max_refs, w), dtype=np.int32)
        n_refs = np.zeros(B, dtype=np.int32)
        for i, g in enumerate(gts):
            g = np.asarray(g).astype(np.int32)
            refs[i, :g.shape[0], :g.shape[1]] = g
            # rows of a NARROWER array that are completely filled carry no terminating 0 (array_to_str, rewards.py:33-39):
            # mark the first padded column with -1 so the kernel does not read the zero padding as an EOS token
            if g.shape[1] < w:
                full = (g != 0).all(1)
                refs[i, :g.shape[0], g.shape[1]][full] = -1
            n_refs[i] = g.shape[0]
        refs_d, n_refs_d = torch.from_numpy(refs).to(self.device), torch.from_numpy(n_refs).to(self.device)
        return PackedRefs(refs_d, n_refs_d, self.cook(refs_d, n_refs_d))

    COOKED_BYTES = _lib.CIDERD_COOKED_BYTES

    def cook(self, refs, n_refs):
        """references cooked once per batch (capmi_ciderd_cook_refs): uint8 [B*max_refs, COOKED_BYTES] on the device"""
        B, max_refs, w = refs.shape
        # (slots >= n_refs[image] are never read by the scoring kernel, valid slots are written whole: no zero fill)
        cooked = torch.empty(B * max_refs, self.COOKED_BYTES, dtype=torch.uint8, device=refs.device)
        check(lib.capmi_ciderd_cook_refs(ptr(refs), ptr(n_refs), B, max_refs, w, ptr(self.keys), ptr(self.vals), self.cap,
                                         self.log_ref_len, ptr(cooked), stream_ptr()), 'capmi_ciderd_cook_refs')
        return cooked

    def score(self, hyp, hyp_img, refs, n_refs, cooked=None):
        """hyp int64 [H,L] (device), hyp_img int32 [H] -> float64 [H] CIDEr-D, no host sync."""
        assert hyp.dtype == torch.long and hyp.is_contiguous() and hyp.is_cuda
        H, L = hyp.shape
        scores = torch.empty(H, dtype=torch.float64, device=hyp.device)
        if cooked is not None:
            check(lib.capmi_ciderd_score_cooked(ptr(hyp), H, L, ptr(hyp_img), ptr(cooked), ptr(n_refs), refs.shape[1],
                                                ptr(self.keys), ptr(self.vals), self.cap, self.log_ref_len, ptr(scores),
                                                stream_ptr()), 'capmi_ciderd_score_cooked')
            return scores
        check(lib.capmi_ciderd_score(ptr(hyp), H, L, ptr(hyp_img), ptr(refs), ptr(n_refs), refs.shape[1], refs.shape[2],
                                     ptr(self.keys), ptr(self.vals), self.cap, self.log_ref_len, ptr(scores),
                                     stream_ptr()), 'capmi_ciderd_score')
        return scores

    SELF_CIDER_NMAX = _lib.SELF_CIDER_NMAX

    def bleu4(self, hyp, hyp_img, packed, cw, bw, base=None, stats=None):
        """cw * base + bw * BLEU-4 of every row of hyp int64 [H,L] against the references of image hyp_img[h] (`packed`: what
        pack_refs returns), float64 [H], one launch (capmi_reward_bleu4).  base: the CIDEr-D scores [H], mixed IN PLACE and
        returned; None: a new tensor of bw * BLEU-4.  Tokens follow the training convention (the first 0 is a word).
        stats: an int32 [H,10] tensor to receive guess 1..4, correct 1..4, length, closest reference length."""
        assert hyp.dtype == torch.long and hyp.is_contiguous() and hyp.is_cuda
        refs, n_refs = packed
        H, L = hyp.shape
        if base is not None:
            assert base.dtype == torch.float64 and base.is_contiguous() and base.shape == (H,)
        out = base if base is not None else torch.empty(H, dtype=torch.float64, device=hyp.device)
        check(lib.capmi_reward_bleu4(ptr(hyp), H, L, ptr(hyp_img), ptr(refs), ptr(n_refs), refs.shape[0], refs.shape[1],
                                     refs.shape[2], ptr(base), float(cw), float(bw), ptr(out), ptr(stats), stream_ptr()),
              'capmi_reward_bleu4')
        return out

    def self_cider(self, hyp, n, parts=False):
        """self-CIDEr diversity of each image's n sampled rows (hyp int64 [B*n, L]) against this table's document frequencies:
        float64 [B], two launches (capmi_self_cider_reward), no host sync.  An image whose n-grams all weigh 0 scores 0.0
        (numpy's eigvalsh route gives NaN).  parts: also return K [B,n,n] and the ascending eigenvalues of K/10 [B,n]."""
        assert hyp.dtype == torch.long and hyp.is_contiguous() and hyp.is_cuda
        N, L = hyp.shape
        if not 2 <= n <= self.SELF_CIDER_NMAX or N % n or N == 0:
            raise ValueError('self-CIDEr needs 2 <= n <= %d samples per image, got %d rows with n = %d' % (self.SELF_CIDER_NMAX, N, n))
        B = N // n
        scratch = torch.empty(N * 4 * (1 + n), dtype=torch.float64, device=hyp.device)      # norm [N,4] | dots [N,n,4]
        out = torch.empty(B, dtype=torch.float64, device=hyp.device)
        K = torch.empty(B, n, n, dtype=torch.float64, device=hyp.device) if parts else None
        eig = torch.empty(B, n, dtype=torch.float64, device=hyp.device) if parts else None
        check(lib.capmi_self_cider_reward(ptr(hyp), B, n, L, ptr(self.keys), ptr(self.vals), self.cap, self.log_ref_len,
                                          scratch.data_ptr(), scratch.data_ptr() + 8 * N * 4, ptr(out), ptr(K), ptr(eig),
                                          stream_ptr()), 'capmi_self_cider_reward')
        return (out, K, eig) if parts else out

    def self_critical_reward(self, greedy, sampled, refs, n_refs, n, hyp_all=None, cooked=None, mix=None):
        """rewards.py:41-81 on device: scores of N sampled + B greedy rows, advantage [N] float32.
        hyp_all: the [N+B, L] tensor holding `sampled` then `greedy` already side by side (the fused SCST rollout writes them
        that way): scored in place, no concatenation.
        mix: (cw, bw) with bw > 0 -- the scores are cw * CIDEr-D + bw * BLEU-4 (CIDEr-D not launched when cw == 0)."""
        N = sampled.shape[0]
        B = greedy.shape[0]
        hyp = hyp_all if hyp_all is not None else torch.cat([sampled, greedy], 0).contiguous()
        key = (N, B, n, str(hyp.device))
        img = self._img_cache.get(key) if hasattr(self, '_img_cache') else None
        if img is None:
            if not hasattr(self, '_img_cache'):
                self._img_cache = {}
            img = torch.cat([torch.arange(N, device=hyp.device) // n, torch.arange(B, device=hyp.device)]).to(torch.int32)
            self._img_cache[key] = img
        if mix is None:
            scores = self.score(hyp, img, refs, n_refs, cooked)
        else:
            cw, bw = mix
            scores = self.bleu4(hyp, img, (refs, n_refs), cw, bw, self.score(hyp, img, refs, n_refs, cooked) if cw > 0 else None)
        buf = torch.empty(N + 1, dtype=torch.float32, device=hyp.device)      # [advantage of the N rows | their mean]
        reward = buf[:N]
        check(lib.capmi_scst_advantage_mean(ptr(scores), N, n, ptr(buf), buf.data_ptr() + 4 * N, stream_ptr()),
              'capmi_scst_advantage_mean')
        reward._capmi_mean = buf[N]             # 0-dim view: LossWrapper's out['reward'] without an ATen mean launch
        return reward, scores
