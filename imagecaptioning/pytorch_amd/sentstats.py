"""The counting numbers of eval_utils.language_eval on the device (host side) -- ``capmi_sentset_*`` of csrc/sentset.hip.

Replaces eval_utils.py:55-68 (novel_sentences: the share of the sample_n captions that are distinct and occur nowhere in the
training captions; vocab_size: their distinct words), :27-36 + :121 (bad_count_rate: the share of the first captions that end in
one of bad_endings) and :79-80 + :92-93 (the mean perplexity / entropy of the scored captions).  The reference compares strings;
here a caption is the label vocabulary's ids of its row before the first 0, and ids and words map one to one
(tests/sentstats_ref.py restates both and tests/test_sentstats_host.py holds them equal).  The training captions are the rows of
the label file the loader already reads, kept in HBM as a set, built once per run.  A training caption that contains the id of
'UNK' is left out: the reference's training strings are the raw tokens, which never spell UNK, so a generated caption with an UNK
in it is always novel.

Deviation from the reference: the label file cuts a caption at its width, so a training caption of more than W words is stored as
its first W words.  A generated caption of exactly W words that equals such a prefix counts as seen here and as novel in the
reference.  (label_length cannot tell a cut row from a full one, so this is not repaired.)  A vocabulary whose words carry BPE
continuation marks, which misc.decode_sequence joins, does not map words to ids one to one either.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, check, stream_ptr

FIRST_KEYS = ('bad_count_rate', 'perplexity', 'entropy')
N_KEYS = ('novel_sentences', 'vocab_size')
FULL_HASH = (1 << 64) - 1


def table_cap_for(n_rows):
    """a power of two that keeps n_rows distinct sentences at a load of at most one half"""
    return 2 << max(0, int(math.ceil(math.log2(max(1, n_rows)))))


def unk_id_of(vocab):
    """the id of the vocabulary word 'UNK' (ix_to_word: id string -> word), 0 when the vocabulary has none"""
    for k, v in vocab.items():
        if v == 'UNK':
            return int(k)
    return 0


class SentenceStats:
    """``train_rows`` [M, W] integer rows (int64, or the label file's uint32; 0 = end and pad; None or empty: no training set, every
    generated sentence is novel), ``vocab_size`` the number of words (ids 1 .. vocab_size), ``unk_id`` the id of 'UNK' (0 / None:
    nothing is skipped), ``bad_endings_ix`` the ids of the bad endings, ``capacity_rows`` the most rows ``add`` will see between
    two ``reset()``s (split x sample_n).  The constructor builds the training set on the device.  ``add`` / ``add_first`` accumulate
    decoded rows without a host sync, ``compute`` reads the record back."""

    def __init__(self, train_rows, device, vocab_size, unk_id, bad_endings_ix, capacity_rows, table_cap=None, gen_table_cap=None,
                 hash_mask=FULL_HASH):
        self.device = dev = torch.device(device)
        if train_rows is None:
            train_rows = np.zeros((0, 1), dtype=np.int64)
        if torch.is_tensor(train_rows):
            train_rows = train_rows.cpu().numpy()
        train_rows = np.ascontiguousarray(train_rows)
        if train_rows.dtype == np.uint32:
            elem, train = 4, torch.from_numpy(train_rows.view(np.int32))        # the same bits: the kernel reads uint32
        else:
            elem, train = 8, torch.from_numpy(train_rows.astype(np.int64))
        if train.dim() != 2 or train.shape[1] < 1 or train.shape[1] > _lib.LANGEVAL_LMAX:
            raise ValueError('training rows must be [M, W] with W <= %d, got %s' % (_lib.LANGEVAL_LMAX, tuple(train.shape)))
        if not 0 <= int(vocab_size) < 65535:
            raise ValueError('vocab_size %r: ids must stay below 65535' % (vocab_size,))
        self.V1 = int(vocab_size) + 1
        self.unk_id = int(unk_id or 0)
        self.capacity_rows = int(capacity_rows)
        if self.capacity_rows < 0:
            raise ValueError('capacity_rows must not be negative')
        self.n_train, self.train_w, self.train_elem = int(train.shape[0]), int(train.shape[1]), elem
        self.table_cap = int(table_cap) if table_cap is not None else table_cap_for(self.n_train)
        self.gen_table_cap = int(gen_table_cap) if gen_table_cap is not None else table_cap_for(self.capacity_rows)
        for cap in (self.table_cap, self.gen_table_cap):
            if cap < 1 or cap & (cap - 1):
                raise ValueError('a table size must be a power of two, got %d' % cap)
        self.hash_mask = int(hash_mask)
        self.train_rows = train.to(dev) if self.n_train else None
        self.train_table = torch.zeros(self.table_cap, dtype=torch.int64, device=dev)           # uint64 slot words
        self.gen_rows = torch.zeros(max(1, self.capacity_rows), _lib.LANGEVAL_LMAX, dtype=torch.int16, device=dev)   # uint16
        self.bad = torch.tensor(sorted(int(i) for i in bad_endings_ix), dtype=torch.int64, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._out = torch.zeros(_lib.SENTSET_NOUT, dtype=torch.float64, device=dev)
        self.reset()
        with torch.cuda.device(dev):
            check(lib.capmi_sentset_build(self._desc(), stream_ptr()), 'capmi_sentset_build')
        if self.n_train:
            self._raise_on(int(self.err.item()), 'training')

    @classmethod
    def for_loader(cls, loader, split, device, model, sample_n):
        """the statistics of one split of a loader (SyntheticLoader / FeatureLoader, bare or wrapped) decoded by ``model``.  With
        sample_n <= 1 only the single-caption numbers are asked for and the training captions are not loaded."""
        n_img = len(loader.language_eval_refs(split)[2])
        sample_n = int(sample_n)
        train = loader.training_captions() if sample_n > 1 else None
        return cls(train, device, model.vocab_size, unk_id_of(model.vocab), model.bad_endings_ix,
                   n_img * sample_n if sample_n > 1 else 0)

    def reset(self):
        """forget every generated row (the training set stays)"""
        dev = self.device
        self.gen_table = torch.zeros(self.gen_table_cap, dtype=torch.int64, device=dev)
        self.vocab_bits = torch.zeros((self.V1 + 31) // 32, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(_lib.SENTSET_NCOUNT, dtype=torch.int64, device=dev)
        self.sums = torch.zeros(2, dtype=torch.float64, device=dev)
        self.err.zero_()
        self.rows_added = 0
        self._d = None

    def _desc(self):
        if getattr(self, '_d', None) is None:
            d = _lib.SentSet()
            d.n_train, d.train_w, d.train_elem, d.unk_id = self.n_train, self.train_w, self.train_elem, self.unk_id
            d.train_cap, d.gen_cap, d.gen_capacity, d.V1 = self.table_cap, self.gen_table_cap, self.capacity_rows, self.V1
            d.n_bad, d.hash_mask = int(self.bad.numel()), self.hash_mask
            d.bad = ptr(self.bad) if self.bad.numel() else None
            for k in ('train_rows', 'train_table', 'gen_rows', 'gen_table', 'vocab_bits', 'counts', 'sums', 'err'):
                setattr(d, k, ptr(getattr(self, k)))
            self._d = d
        return self._d

    @staticmethod
    def _raise_on(err, which='generated'):
        if err & _lib.LANGEVAL_E_TABLE_FULL:
            raise _lib.CapmiError('sentence_stats: a table is too small for the %s sentences' % which)
        if err & _lib.LANGEVAL_E_TOKEN:
            raise _lib.CapmiError('sentence_stats: a token id outside [0, 65535) or beyond the vocabulary')

    def _rows(self, seq, what):
        if not torch.is_tensor(seq) or seq.dtype != torch.long or not seq.is_cuda or seq.dim() not in (2, 3):
            raise ValueError('%s must be an int64 [rows, L] device tensor' % what)
        if seq.dim() == 3:
            seq = seq.reshape(-1, seq.shape[2])
        if seq.shape[1] < 1 or seq.shape[1] > _lib.LANGEVAL_LMAX:
            raise ValueError('sentence_stats: rows of %d tokens, the compiled bound is %d' % (seq.shape[1], _lib.LANGEVAL_LMAX))
        return seq.contiguous()

    def add(self, seqs):
        """seqs int64 [rows, L] (or [B, sample_n, L]) on the device: the sample_n captions of a decoded batch.  No host sync."""
        seqs = self._rows(seqs, 'seqs')
        if self.rows_added + seqs.shape[0] > self.capacity_rows:
            raise ValueError('sentence_stats: %d rows after %d, sized for %d' % (seqs.shape[0], self.rows_added, self.capacity_rows))
        with torch.cuda.device(self.device):
            check(lib.capmi_sentset_add(self._desc(), ptr(seqs), seqs.shape[0], seqs.shape[1], self.rows_added, stream_ptr()),
                  'capmi_sentset_add')
        self.rows_added += seqs.shape[0]

    def add_first(self, seq, perplexity, entropy):
        """seq int64 [rows, L] on the device: the first caption of each image; perplexity / entropy [rows], as ops.caption_stats
        returns them.  No host sync."""
        seq = self._rows(seq, 'seq')
        stats = [torch.as_tensor(x).to(self.device, torch.float32).reshape(-1).contiguous() for x in (perplexity, entropy)]
        if any(x.shape[0] != seq.shape[0] for x in stats):
            raise ValueError('sentence_stats: one perplexity and one entropy per row')
        with torch.cuda.device(self.device):
            check(lib.capmi_sentset_add_first(self._desc(), ptr(seq), seq.shape[0], seq.shape[1], ptr(stats[0]), ptr(stats[1]),
                                              stream_ptr()), 'capmi_sentset_add_first')

    def compute(self):
        """-> {'bad_count_rate', 'perplexity', 'entropy'} and, when ``add`` saw rows (the reference: ``if len(preds_n) > 0``),
        'novel_sentences' = novel distinct sentences / rows seen and 'vocab_size'.  The one host sync; the raw record stays in
        ``self.record`` (float64 [9]: rows seen, distinct, novel distinct, first rows, bad rows, words, sums, error bits)."""
        with torch.cuda.device(self.device):
            check(lib.capmi_sentset_reduce(self._desc(), ptr(self._out), stream_ptr()), 'capmi_sentset_reduce')
        self.record = out = self._out.cpu().numpy().copy()
        self._raise_on(int(out[8]))
        rows, first = int(out[0]), int(out[3])
        stats = {'bad_count_rate': out[4] / max(1, first), 'perplexity': out[6] / max(1, first), 'entropy': out[7] / max(1, first)}
        if rows > 0:
            stats['novel_sentences'] = out[2] / rows
            stats['vocab_size'] = int(out[5])
        return {k: (v if isinstance(v, int) else float(v)) for k, v in stats.items()}
