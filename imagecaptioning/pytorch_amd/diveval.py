"""Diversity evaluation of sample_n captions per image on the device (host side) -- ``capmi_diveval_*`` of csrc/langeval.hip.

Replaces captioning/utils/eval_multi.py behind eval_utils.language_eval (eval_utils.py:104-119): eval_div_stats (Div1, Div2, gDiv1
of div_utils.py, mBLeu_1..4), eval_self_cider (Wang & Chan 2019) and eval_oracle (oracle_X / avg_X for the Java-free X).  AllSPICE
needs Java and is absent; novel_sentences and vocab_size are sentstats.py's.  div_utils.py is pinned by
tests/golden/diveval_ref.npz; the mBLEU and self-CIDEr arithmetic is PARITY UNPINNED, as langeval.py: coco-caption and the cider
submodule are not part of the reference checkout, the formulas are restated in tests/diveval_ref64.py.  Captions are compared as
the label vocabulary's ids, a caption being the ids of its row before the first 0.

Deviation from the reference: an image whose captions are all empty has no positive eigenvalue, numpy's 0 / 0 makes its self_cider
NaN and poisons the mean; here that image scores 0.0 and is counted.
"""
import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, check, stream_ptr
from .langeval import NG

ORACLE_KEYS = ('CIDEr', 'Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L')       # order of capmi_diveval.oracle_scores
DIV_KEYS = ('Div1', 'Div2', 'gDiv1', 'mBLeu_1', 'mBLeu_2', 'mBLeu_3', 'mBLeu_4')


class DiversityEval:
    """``sample_n`` captions per image on the tables of ``lang``, a langeval.LanguageEval of the split (its document-frequency
    table and its references are shared, nothing is built twice).  ``add`` accumulates decoded groups without a host sync,
    ``compute`` reads the scores back.  A later group for an image replaces the earlier one; gDiv1 counts the distinct tokens of
    everything added since ``reset()``, replaced groups included (its bitmap is a union)."""

    def __init__(self, lang, sample_n, oracle=False):
        if not isinstance(sample_n, int) or sample_n < 2 or sample_n > _lib.DIVEVAL_NMAX:
            raise ValueError('sample_n must be in [2, %d], got %r' % (_lib.DIVEVAL_NMAX, sample_n))
        self.lang, self.n, self.oracle = lang, sample_n, bool(oracle)
        self.device, self.n_img = lang.device, lang.n_img
        self.pos_of_id = {}
        self._out = torch.zeros(_lib.DIVEVAL_NOUT, dtype=torch.float64, device=self.device)
        self._totals = torch.zeros(self.n, 10, dtype=torch.int64, device=self.device)
        self.reset()

    def reset(self):
        """forget every group and every token seen"""
        dev, m, n = self.device, self.n_img, self.n

        def z(*shape, dtype=torch.float64):
            return torch.zeros(*shape, dtype=dtype, device=dev)
        self.norm, self.sent_bleu2, self.K, self.eig, self.self_cider = z(m, n, NG), z(m, n), z(m, n, n), z(m, n), z(m)
        self.slot_distinct, self.distinct, self.tokens = (z(m, n, 2, dtype=torch.int32), z(m, 2, dtype=torch.int32),
                                                          z(m, dtype=torch.int32))
        self.mbleu_stats, self.seen, self.err = z(m, n, 10, dtype=torch.int32), z(m, dtype=torch.int32), z(1, dtype=torch.int32)
        self.vocab_bits = z(_lib.DIVEVAL_VOCAB_WORDS, dtype=torch.int32)
        self.oracle_scores = z(m, n, len(ORACLE_KEYS)) if self.oracle else None
        # the scratch the oracle launch writes through the langeval descriptor, one row per (image, slot)
        self._or = ({'cider': z(m * n), 'rouge': z(m * n), 'bleu_stats': z(m * n, NG, 2, dtype=torch.int32),
                     'lens': z(m * n, 2, dtype=torch.int32)} if self.oracle else {})
        self.pos_of_id.clear()
        self._d = None

    def _desc(self):
        if self._d is None:
            d, src = _lib.DivEval(), self.lang._desc()
            for name, _ in _lib.LangEval._fields_:
                setattr(d.lang, name, getattr(src, name))
            d.lang.lcs = d.lang.seen = None
            for k in ('cider', 'rouge', 'bleu_stats', 'lens'):
                setattr(d.lang, k, ptr(self._or.get(k)))
            d.lang.err = ptr(self.err)
            d.n, d.oracle = self.n, int(self.oracle)
            for k in ('norm', 'slot_distinct', 'distinct', 'tokens', 'mbleu_stats', 'sent_bleu2', 'K', 'eig', 'self_cider',
                      'oracle_scores', 'seen', 'err', 'vocab_bits'):
                setattr(d, k, ptr(getattr(self, k)))
            self._d = d
        return self._d

    def add(self, image_index, seqs):
        """seqs int64 [B * sample_n, L] (or [B, sample_n, L]) decoded rows on the device, rows k*n .. k*n+n-1 the captions of
        image_index[k] (positions in the split, tensor or list).  No host sync."""
        if not torch.is_tensor(seqs) or seqs.dtype != torch.long or not seqs.is_cuda or seqs.dim() not in (2, 3):
            raise ValueError('seqs must be an int64 [B * sample_n, L] device tensor')
        if seqs.dim() == 3:
            if seqs.shape[1] != self.n:
                raise ValueError('seqs: %d captions per image, sample_n is %d' % (seqs.shape[1], self.n))
            seqs = seqs.reshape(-1, seqs.shape[2])
        if seqs.shape[1] < 1 or seqs.shape[1] > _lib.LANGEVAL_LMAX:
            raise ValueError('seqs: rows of %d tokens, the compiled bound is %d' % (seqs.shape[1], _lib.LANGEVAL_LMAX))
        idx = torch.as_tensor(image_index, dtype=torch.int64)
        if idx.dim() != 1 or seqs.shape[0] != idx.shape[0] * self.n:
            raise ValueError('seqs: %d rows for %d entries of image_index, sample_n is %d' % (seqs.shape[0], idx.numel(), self.n))
        if not idx.is_cuda:
            idx = idx.pin_memory().to(self.device, non_blocking=True) if idx.numel() else idx.to(self.device)
        seqs = seqs.contiguous()
        with torch.cuda.device(self.device):
            check(lib.capmi_diveval_add(self._desc(), ptr(seqs), idx.shape[0], seqs.shape[1], ptr(idx), stream_ptr()),
                  'capmi_diveval_add')

    def add_batch(self, infos, seqs):
        """groups of one loader batch: infos[k]['ix'] names the image of rows k*n .. k*n+n-1"""
        pos = [self.lang.index_of[inf['ix']] for inf in infos]
        self.pos_of_id.update((inf['id'], p) for inf, p in zip(infos, pos))
        self.add(pos, seqs)

    def compute(self):
        """-> (overall, per_image).  overall: Div1, Div2, gDiv1, mBLeu_1..4, self_cider and, with oracle, oracle_X / avg_X for X in
        ORACLE_KEYS, as floats.  per_image: numpy arrays over the split -- 'seen' bool [n_img], 'Div1' 'Div2' 'self_cider' 'mBleu_2'
        [n_img], 'individual_mBleu_2' [n_img, n], 'self_cider_mat' [n_img, n, n], 'eig' [n_img, n] and, with oracle, 'scores'
        [n_img, n, 6] in ORACLE_KEYS order, 'oracle_X' / 'avg_X' [n_img]; rows of images without a group are meaningless.  The one
        host sync of an evaluation."""
        with torch.cuda.device(self.device):
            check(lib.capmi_diveval_reduce(self._desc(), ptr(self._out), ptr(self._totals), stream_ptr()), 'capmi_diveval_reduce')
        out = self._out.cpu().numpy()
        self.lang._raise_on(int(out[9]))
        self.n_added = int(out[8])
        overall = {k: float(out[i]) for i, k in enumerate(DIV_KEYS)}
        overall['self_cider'] = float(out[7])
        tokens = 1e-6 + self.tokens.cpu().numpy().astype(np.float64)
        distinct = self.distinct.cpu().numpy().astype(np.float64)
        bleu2 = self.sent_bleu2.cpu().numpy()
        per_image = {'seen': self.seen.cpu().numpy() != 0, 'Div1': distinct[:, 0] / tokens, 'Div2': distinct[:, 1] / tokens,
                     'self_cider': self.self_cider.cpu().numpy(), 'mBleu_2': bleu2.mean(axis=1), 'individual_mBleu_2': bleu2,
                     'self_cider_mat': self.K.cpu().numpy(), 'eig': self.eig.cpu().numpy()}
        if self.oracle:
            scores = self.oracle_scores.cpu().numpy()
            per_image['scores'] = scores
            for x, k in enumerate(ORACLE_KEYS):
                overall['oracle_' + k], overall['avg_' + k] = float(out[10 + x]), float(out[10 + len(ORACLE_KEYS) + x])
                per_image['oracle_' + k], per_image['avg_' + k] = scores[:, :, x].max(axis=1), scores[:, :, x].mean(axis=1)
        return overall, per_image
