"""Corpus language evaluation on the device (host side): coco-caption's Cider, Bleu ('closest') and Rouge over token ids,
without Java -- ``capmi_langeval_*`` of csrc/langeval.hip.

Replaces the three Java-free scorers behind eval_utils.language_eval (COCOEvalCap.evaluate -> Bleu(4), Rouge(), Cider()), whose
result the reference's trainer reads as ``lang_stats['CIDEr']`` (tools/train.py:252-266).  METEOR and SPICE need Java and are
absent.  PARITY UNPINNED, as ciderd.py: coco-caption is not part of the reference checkout, the arithmetic is restated from its
published formulas (tests/langeval_ref64.py); the PTB tokenizer is not reproduced -- captions are compared as the label
vocabulary's ids, a caption being the ids of its row before the first 0.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, check, stream_ptr

KEYS = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDEr')
NG = 4


def min_table_cap(n_keys):
    """the smallest table the kernels accept for n_keys distinct n-grams (a power of two; probing wraps round)"""
    return 1 << max(0, int(math.ceil(math.log2(max(1, n_keys)))))


class LanguageEval:
    """Built once per split from its reference captions: ``refs`` [total_refs, L] integer rows (0 = end and pad), ``offsets``
    [n_img + 1] -- image i owns rows offsets[i] .. offsets[i+1].  The constructor builds the document-frequency table on the
    device.  ``add`` accumulates decoded rows without a host sync, ``compute`` reads the scores back."""

    def __init__(self, refs, offsets, device, table_cap=None, image_ids=None):
        refs = torch.as_tensor(np.asarray(refs).astype(np.int64) if not torch.is_tensor(refs) else refs).to(torch.int64)
        off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets).astype(np.int64)
        if refs.dim() != 2 or refs.shape[1] < 1 or refs.shape[1] > _lib.LANGEVAL_LMAX:
            raise ValueError('references must be [total_refs, L] with L <= %d, got %s' % (_lib.LANGEVAL_LMAX, tuple(refs.shape)))
        if off.ndim != 1 or off.shape[0] < 2 or off[0] != 0 or off[-1] != refs.shape[0] or (np.diff(off) < 0).any():
            raise ValueError('offsets must rise from 0 to total_refs = %d' % refs.shape[0])
        self.device = torch.device(device)
        self.n_img, self.total_refs, self.ref_w = int(off.shape[0] - 1), int(refs.shape[0]), int(refs.shape[1])
        # every n-gram instance distinct is the most the table can be asked to hold; load factor <= 0.5 then
        if table_cap is None:
            table_cap = 2 * min_table_cap(max(1, self.total_refs * NG * self.ref_w))
        if table_cap < 1 or table_cap & (table_cap - 1):
            raise ValueError('table_cap must be a power of two')
        self.table_cap = int(table_cap)
        dev = self.device
        self.refs = refs.to(dev).contiguous()
        self.ref_off = torch.from_numpy(off.astype(np.int32)).to(dev)
        self.table_keys = torch.zeros(self.table_cap, dtype=torch.int64, device=dev)       # uint64 bit patterns
        self.table_counts = torch.zeros(self.table_cap, dtype=torch.int32, device=dev)
        self.ref_norm = torch.zeros(max(1, self.total_refs), NG, dtype=torch.float64, device=dev)
        self.lcs = torch.zeros(max(1, self.total_refs), dtype=torch.int32, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.image_ids = list(image_ids) if image_ids is not None else list(range(self.n_img))
        self.index_of = {k: i for i, k in enumerate(self.image_ids)}
        self.pos_of_id = {}              # infos[k]['id'] of the rows add_batch saw -> position in the split
        self._out = torch.zeros(8, dtype=torch.float64, device=dev)
        self._totals = torch.zeros(10, dtype=torch.int64, device=dev)
        self.reset()
        with torch.cuda.device(dev):
            check(lib.capmi_langeval_build(self._desc(), stream_ptr()), 'capmi_langeval_build')
        self._raise_on(int(self.err.item()))

    @classmethod
    def from_gts(cls, gts, device, **kw):
        """list (per image) of [n_ref_i, L] integer arrays, as the loaders' batch['gts']"""
        w = max(np.asarray(g).shape[1] for g in gts)
        rows = np.zeros((sum(len(g) for g in gts), w), dtype=np.int64)
        off, r = [0], 0
        for g in gts:
            g = np.asarray(g)
            rows[r:r + g.shape[0], :g.shape[1]] = g
            r += g.shape[0]
            off.append(r)
        return cls(rows, off, device, **kw)

    @classmethod
    def for_loader(cls, loader, split, device):
        """the evaluator of one split of a loader (SyntheticLoader / FeatureLoader, bare or wrapped)"""
        rows, off, ids = loader.language_eval_refs(split)
        return cls(rows, off, device, image_ids=ids)

    def reset(self):
        """forget every hypothesis (the table and the reference norms stay)"""
        dev = self.device
        self.cider = torch.zeros(self.n_img, dtype=torch.float64, device=dev)
        self.rouge = torch.zeros(self.n_img, dtype=torch.float64, device=dev)
        self.bleu_stats = torch.zeros(self.n_img, NG, 2, dtype=torch.int32, device=dev)
        self.lens = torch.zeros(self.n_img, 2, dtype=torch.int32, device=dev)
        self.seen = torch.zeros(self.n_img, dtype=torch.int32, device=dev)
        self._d = None

    def _desc(self):
        if getattr(self, '_d', None) is None:
            d = _lib.LangEval()
            d.n_img, d.total_refs, d.ref_w, d.table_cap = self.n_img, self.total_refs, self.ref_w, self.table_cap
            for k in ('refs', 'ref_off', 'table_keys', 'table_counts', 'ref_norm', 'cider', 'rouge', 'bleu_stats', 'lens', 'lcs',
                      'seen', 'err'):
                setattr(d, k, ptr(getattr(self, k)))
            self._d = d
        return self._d

    @staticmethod
    def _raise_on(err):
        if err & _lib.LANGEVAL_E_TABLE_FULL:
            raise _lib.CapmiError('language_eval: the document-frequency table is too small for the references')
        if err & _lib.LANGEVAL_E_TOKEN:
            raise _lib.CapmiError('language_eval: a token id outside [0, 65535)')
        if err & _lib.LANGEVAL_E_IMAGE:
            raise _lib.CapmiError('language_eval: an image index outside the split')

    def add(self, image_index, seq):
        """seq int64 [H, L] decoded rows (device), image_index [H] (tensor or list of positions in the split): per-image results
        are written on the device, no host sync.  A hypothesis for an image that already has one replaces it."""
        if seq.dtype != torch.long or not seq.is_cuda or seq.dim() != 2:
            raise ValueError('seq must be an int64 [H, L] device tensor')
        if seq.shape[1] > _lib.LANGEVAL_LMAX:
            raise ValueError('language_eval: rows of %d tokens exceed the compiled bound %d' % (seq.shape[1], _lib.LANGEVAL_LMAX))
        idx = torch.as_tensor(image_index, dtype=torch.int64)
        if not idx.is_cuda:
            idx = idx.pin_memory().to(self.device, non_blocking=True) if idx.numel() else idx.to(self.device)
        if idx.shape[0] != seq.shape[0]:
            raise ValueError('one image index per row: %d rows, %d indices' % (seq.shape[0], idx.shape[0]))
        seq = seq.contiguous()
        with torch.cuda.device(self.device):
            check(lib.capmi_langeval_add(self._desc(), ptr(seq), seq.shape[0], seq.shape[1], ptr(idx), stream_ptr()),
                  'capmi_langeval_add')

    def add_batch(self, infos, seq):
        """rows of one loader batch: infos[k]['ix'] names the image of row k"""
        pos = [self.index_of[inf['ix']] for inf in infos]
        self.pos_of_id.update((inf['id'], p) for inf, p in zip(infos, pos))
        self.add(pos, seq)

    def compute(self):
        """-> ({'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'} as floats, per-image CIDEr float64 numpy [n_img], NaN where no hypothesis
        was added).  The one host sync of an evaluation."""
        with torch.cuda.device(self.device):
            check(lib.capmi_langeval_reduce(self._desc(), ptr(self._out), ptr(self._totals), stream_ptr()), 'capmi_langeval_reduce')
        out = self._out.cpu().numpy()
        self._raise_on(int(out[7]))
        self.n_added = int(out[6])
        stats = {k: float(out[i]) for i, k in enumerate(KEYS)}
        per_image = self.cider.cpu().numpy().copy()
        per_image[self.seen.cpu().numpy() == 0] = np.nan
        return stats, per_image
