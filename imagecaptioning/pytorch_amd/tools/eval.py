#!/usr/bin/env python3
"""Evaluation entrypoint on the MI355X backend -- the decode half of the reference's tools/eval.py:23-125 +
eval_utils.eval_split / eval_split_n (eval_utils.py:128-290): XE validation loss, decode with every sampler option of the
command line (beam / diverse beam search, sampling variants, decoding constraints), sample_n captions per image,
per-caption entropy and perplexity from seqLogprobs (:173-174), decoded strings.  --language_eval 1 (eval_utils.py:47-125): corpus
CIDEr, BLEU-1..4 and ROUGE-L of the single-caption pass, scored on the device over token ids (imagecaptioning/pytorch_amd/langeval.py)
and written to <eval_results_dir>/<id>_<split>.json as {'overall', 'imgToEval'}; METEOR and SPICE need Java and are absent.
With --sample_n N > 1 the N captions per image are also scored for diversity on the device (captioning/utils/eval_multi.py ->
imagecaptioning/pytorch_amd/diveval.py): Div1, Div2, gDiv1, mBLeu_1..4, self_cider and, with --eval_oracle 1, oracle_X / avg_X; they
join lang_stats and are written to <id>_<split>_n.json.  AllSPICE needs Java and is absent.
--sentence_stats 1 adds the counting numbers of eval_utils.language_eval (:27-36, 55-68, 79-80, 121) to lang_stats and to
<id>_<split>.json: bad_count_rate and the mean perplexity / entropy of the first captions and, with --sample_n N > 1, novel_sentences
and vocab_size of the N captions per image against the training captions of the label file (imagecaptioning/pytorch_amd/sentstats.py).
--dump_attention 1 (updown / topdown, att2in2, adaatt, adaattmo) decodes with opt['return_attention'] and writes, per image id, the
caption's per-word region attention to <eval_results_dir>/<id>_<split>_att.npz: <image id>/att [L, regions (+ 1 sentinel column in front
for AdaAtt)], /top, /top_w, /entropy [L], /regions, and -- with the real-file loader and --input_box_dir -- /box (the attention-weighted
box per word) and /top_box (the top region's own box); one device-to-host transfer per batch (imagecaptioning/pytorch_amd/att_trace.py).

--sample_n_method sbs (stochastic beam search, imagecaptioning/pytorch_amd/sbs.py) draws the N <= 16 captions of an image WITHOUT
replacement in one search: N distinct captions; the predictions carry 'perplexity' and, with --verbose_beam 1, the caption's
importance weight 'log_w'.

--constraints_json FILE (constrained beam search, imagecaptioning/pytorch_amd/cbs.py) holds {"<image id>": [["zebra", "zebras"],
["grass"]], ...}: the caption of such an image must contain one word of each list (at most 4 lists of at most 8 words; 2^lists *
beam_size <= 64); images the file does not name are decoded without constraints.  --constraints_oov error (default) stops at a word
that is not in the vocabulary, drop leaves such words -- and the lists they empty -- out and prints how many.  Every prediction
gains 'constraints_satisfied' / 'constraints_total'; <eval_results_dir>/<id>_<split>_cbs.json holds the share of images whose
constraints were all satisfied and the mean satisfied fraction.

--no_repeat_ngram_size N, --repetition_penalty X, --min_length M, --bad_words "a man" top ... and --bad_words_json FILE (a JSON list of
strings or of word lists; words outside the vocabulary as --constraints_oov says) are the logits processors of
imagecaptioning/pytorch_amd/logits_proc.py: they reach every decoder that keeps a history, and with --language_eval 1 the settings
are recorded as 'logits_processors' in <eval_results_dir>/<id>_<split>.json (the key is absent when all are off).

--self_retrieval 1 [--retrieval_pool 1000] [--score_norm none|length] (imagecaptioning/pytorch_amd/score.py): after decoding, the first
caption of every evaluated image is scored against every image of its pool -- consecutive blocks of retrieval_pool images, the last
one possibly smaller -- by log p(caption | image) (divided by the scored length under --score_norm length); every prediction gains
'retrieval_rank' (1: the caption picks its own image; ties go to the lower image) and 'retrieval_log_post', and
<eval_results_dir>/<id>_<split>_ret.json holds R@1, R@5, R@10, the median and mean rank, MRR, the pool size and the pools.  It does
not combine with --constraints_json, or with --sample_n > 1 without --rerank.
--score_json FILE holds {"<image id>": ["a caption", ...]}: the captions are scored under the model for their image; words outside
the vocabulary become UNK, or are dropped with --constraints_oov drop; captions are cut at seq_length words.
<eval_results_dir>/<id>_<split>_scores.json holds per caption 'logp', 'len' (scored tokens, the end token included), 'perplexity'
and the words it lacked, and lists the image ids of the file that the evaluated split did not hold.

--rerank mbr_ciderd | mbr_bleu4 with --sample_n N (2..32) and --sample_n_method sample / gumbel / top<k|p> / sbs / bs decodes N captions per
image and keeps the one with the highest expected CIDEr-D / BLEU-4 against the others (imagecaptioning/pytorch_amd/mbr.py;
--rerank_prior model weighs them by the model's own probabilities): that caption is the image's prediction, scored and written
as for --sample_n 1; every prediction gains 'mbr_choice' and 'mbr_expected', and <eval_results_dir>/<id>_<split>_mbr.npz holds
image_id, choice [images], expected [images, N] and candidates [images, N, L].

--disc_lambda X [--disc_distractors D] [--disc_mode suppress|listener] [--disc_pick nearest|random] (discriminative decoding,
imagecaptioning/pytorch_amd/disc.py): every image of an eval batch is decoded against D <= 7 other images of the same batch, so that
its caption tells it from them -- opt['distractors'] with lambda = X in [0, 1] (1: the plain decoder; the flag absent: off).  nearest
picks the D images whose mean-pooled region features have the highest cosine similarity to the image's, random draws them with
--seed; a batch with fewer than D + 1 images leaves the missing slots empty.  Every prediction gains 'distractors' (image ids);
<eval_results_dir>/<id>_<split>_disc.json holds the settings and the distractors per image.  It combines with --language_eval,
--beam_size, --sample_n_method sbs, --constraints_json and --self_retrieval 1 (one command then shows what the option is for: the
R@1 of the captions it decodes), not with --dump_attention.

--sample_method / --sample_n_method minp<a> | eps<e> | eta<e> | typ<tau> (min-p, epsilon, eta and locally typical sampling,
capmi_truncate_rows in front of the token choice of imagecaptioning/pytorch_amd/decode.py): wherever sample / top<k|p> are accepted,
e.g. --sample_n 5 --sample_n_method typ0.9 --language_eval 1; the predictions and the _n.json carry no new fields.

--sample_method contrastive [--penalty_alpha 0.6] [--contrastive_k 4] (contrastive search, Su et al. 2022: decode.contrastive_steps)
decodes one caption per image that avoids repeating itself: at every step the contrastive_k most probable words are re-scored by
(1 - penalty_alpha) p(word) - penalty_alpha max cos(hidden state after the word, hidden states so far).  updown / topdown, newfc,
att2in2, adaatt, adaattmo, aoa (out_res 0); with --decoding_constraint, --remove_bad_endings, --block_trigrams and --language_eval, not with
--beam_size, --sample_n_method contrastive, --temperature, --disc_lambda, --constraints_json or --dump_attention; tools/eval_ensemble.py
reports that an ensemble has no single hidden state.

    python -m imagecaptioning.pytorch_amd.tools.eval --caption_model updown --beam_size 5 --num_images 20 [--start_from DIR | --model FILE]
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


SAMPLE_KEYS = ('sample_method', 'beam_size', 'temperature', 'suppress_UNK', 'length_penalty', 'group_size', 'diversity_lambda',
               'decoding_constraint', 'block_trigrams', 'remove_bad_endings', 'max_length', 'penalty_alpha', 'contrastive_k',
               'no_repeat_ngram_size', 'repetition_penalty', 'min_length', 'bad_words')


def eval_kwargs_of(opt):
    """eval_utils.eval_split hands vars(opt) to the sampler (eval.py:103, eval_utils.py:169-171): every decode option of
    the command line reaches model._sample."""
    return {k: getattr(opt, k) for k in SAMPLE_KEYS if hasattr(opt, k)}


def eval_split_n(model, n_predictions, fc, att, att_masks, data, opt, extra=None):
    """eval_utils.eval_split_n (eval_utils.py:228-290): sample_n captions per image by beam search ('bs'), sampling
    ('sample' / 'gumbel' / 'top<k|p>'), stochastic beam search ('sbs': distinct captions, drawn without replacement), diverse beam
    search ('dbs') or diverse sampling ('d<method>').  Returns the token rows of
    what it decoded, int64 [B, sample_n, L] on the device (finished beams padded with 0), in the order of the appended predictions.
    extra: further options of every decode of the batch (--disc_lambda: the batch's distractors)."""
    from captioning.utils import misc
    kw = eval_kwargs_of(opt)
    kw.update(extra or {})
    sample_n, method, beam_size = opt.sample_n, opt.sample_n_method, opt.beam_size
    refuse_contrastive_n(method)
    with torch.no_grad():
        if method == 'bs':                                                  # :243-252
            kw.update(sample_n=1, beam_size=sample_n, group_size=1, sample_method='beam_search')
            model(fc, att, att_masks, opt=kw, mode='sample')
            rows = _pad_stack([model.done_beams[k][i]['seq'] for k in range(fc.shape[0]) for i in range(sample_n)])
            for k in range(fc.shape[0]):
                for sent in misc.decode_sequence(model.vocab, rows[k * sample_n:(k + 1) * sample_n]):
                    n_predictions.append({'image_id': data['infos'][k]['id'], 'caption': sent})
        elif method in ('sample', 'gumbel') or method.startswith('top') or _is_truncation(method):   # :254-264; minp / eps / eta / typ
            kw.update(sample_n=sample_n, sample_method=method, beam_size=1)
            seq, logp = model(fc, att, att_masks, opt=kw, mode='sample')
            ppl = -logp.gather(2, seq.unsqueeze(2)).squeeze(2).sum(1) / ((seq > 0).to(logp).sum(1) + 1)
            for k, sent in enumerate(misc.decode_sequence(model.vocab, seq)):
                n_predictions.append({'image_id': data['infos'][k // sample_n]['id'], 'caption': sent, 'perplexity': ppl[k].item()})
            rows = seq
        elif method == 'sbs':
            # stochastic beam search (imagecaptioning/pytorch_amd/sbs.py; not a method of the reference): sample_n DISTINCT captions,
            # drawn without replacement in one search
            kw.update(sample_n=sample_n, sample_method='sbs', beam_size=1, group_size=1)
            seq, logp = model(fc, att, att_masks, opt=kw, mode='sample')
            ppl = -logp.gather(2, seq.unsqueeze(2)).squeeze(2).sum(1) / ((seq > 0).to(logp).sum(1) + 1)
            log_w = model.last_sbs['log_w'].reshape(-1).tolist() if getattr(opt, 'verbose_beam', 0) else None
            for k, sent in enumerate(misc.decode_sequence(model.vocab, seq)):
                n_predictions.append({'image_id': data['infos'][k // sample_n]['id'], 'caption': sent, 'perplexity': ppl[k].item()})
                if log_w is not None:          # the importance weight of the caption among the image's sample_n (-inf: the threshold)
                    n_predictions[-1]['log_w'] = log_w[k]
            rows = seq
        elif method == 'dbs':                                               # :265-274
            kw.update(beam_size=sample_n * beam_size, group_size=sample_n, sample_method='beam_search', sample_n=1)
            model(fc, att, att_masks, opt=kw, mode='sample')
            rows = _pad_stack([model.done_beams[k][i]['seq'] for k in range(fc.shape[0])
                               for i in range(0, sample_n * beam_size, beam_size)])      # the first beam of each group
            for k in range(fc.shape[0]):
                for sent in misc.decode_sequence(model.vocab, rows[k * sample_n:(k + 1) * sample_n]):
                    n_predictions.append({'image_id': data['infos'][k]['id'], 'caption': sent})
        else:                                                               # :275-283 diverse sampling, 'd' + method
            kw.update(sample_method=method[1:], group_size=sample_n, beam_size=1)
            seq, _ = model(fc, att, att_masks, opt=kw, mode='sample')
            for k, sent in enumerate(misc.decode_sequence(model.vocab, seq)):
                n_predictions.append({'image_id': data['infos'][k // sample_n]['id'], 'caption': sent})
            rows = seq
    return rows.to(torch.long).reshape(fc.shape[0], sample_n, -1)


def refuse_contrastive_n(method):
    """--sample_n_method contrastive: contrastive search is deterministic, there are no n captions to draw"""
    if method == 'contrastive':
        raise ValueError('sample_n_method %r: contrastive search is deterministic and would return sample_n identical captions per '
                         'image; it is a --sample_method (with --penalty_alpha, --contrastive_k)' % method)


def _is_truncation(method):
    """--sample_method / --sample_n_method minp<a>, eps<e>, eta<e>, typ<tau> (a parameter outside its range raises here)"""
    from imagecaptioning.pytorch_amd.captioning.models.utils import parse_truncation
    return parse_truncation(method) is not None


def _pad_stack(seqs):
    """torch.stack of the beams' token rows; finished beams are shorter than seq_length here (the reference stacks rows that
    all ran to the same length only when none ended early), so pad with the end token."""
    ln = max(s.shape[0] for s in seqs)
    return torch.stack([torch.cat([s, s.new_zeros(ln - s.shape[0])]) for s in seqs])


def batch_boxes(loader, opt, data, K, dev):
    """[B, K, 4] float32 boxes (x1, y1, x2, y2 in pixels, zero rows behind an image's regions) of a batch of the real-file loader, in
    the order of its region rows (use_box re-orders them by area), or None without --input_box_dir / with the synthetic loader"""
    box_dir = getattr(opt, 'input_box_dir', None)
    if not getattr(opt, 'input_json', '') or not box_dir or not os.path.isdir(box_dir):
        return None
    import numpy as np
    from captioning.data import feature_loader as fl
    out = np.zeros((len(data['infos']), K, 4), dtype=np.float32)
    for i, info in enumerate(data['infos']):
        b = fl._load_rows(box_dir, info['id'], 'box')
        if getattr(opt, 'use_box', 0):
            im = loader.info['images'][info['ix']]
            b = fl.append_boxes(b, b, int(im['height']), int(im['width']), bool(getattr(opt, 'norm_box_feat', 0)))[:, :4]
        out[i, :min(K, b.shape[0])] = b[:K]
    return torch.from_numpy(out).to(dev)


def rerank_kwargs(opt):
    """--rerank: the decode options of the single-caption pass -- the sample_n_method decode of eval_split_n with the reranking
    on top -- or {} without the flag"""
    kind = getattr(opt, 'rerank', '')
    if not kind:
        return {}
    n, method = opt.sample_n, opt.sample_n_method
    refuse_contrastive_n(method)
    kw = dict(rerank=kind, rerank_prior=getattr(opt, 'rerank_prior', 'uniform'), sample_n=n)
    if method == 'bs':
        kw.update(beam_size=n, group_size=1, sample_method='beam_search')
    elif method in ('sample', 'gumbel', 'sbs') or method.startswith('top') or _is_truncation(method):
        kw.update(sample_method=method, beam_size=1)
    else:
        raise NotImplementedError('--rerank chooses among the captions of --sample_n_method sample / gumbel / top<k|p> / minp<a> / '
                                  'eps<e> / eta<e> / typ<tau> / sbs / bs; %r '
                                  'returns the first beam of every group or one row per group, not sample_n rows of one decode'
                                  % method)
    return kw


class RerankDump:
    """--rerank: what the reranking chose, kept on the device per batch and written as one .npz"""

    def __init__(self):
        self.ids, self.parts = [], []

    def add_batch(self, last, infos, keep):
        n = last['expected'].shape[1]
        self.ids += [info['id'] for info in infos[:keep]]
        self.parts.append((last['choice'][:keep], last['expected'][:keep], last['candidates'].view(-1, n, last['candidates'].shape[1])[:keep]))

    def write(self, opt, split):
        import numpy as np
        out_dir = getattr(opt, 'eval_results_dir', 'eval_results')
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, '%s_%s_mbr.npz' % (getattr(opt, 'id', 'capmi'), split))
        choice, expected, candidates = (torch.cat(p).cpu().numpy() for p in zip(*self.parts))
        np.savez(path, image_id=np.array(self.ids), choice=choice, expected=expected, candidates=candidates)
        return path


class ConstraintSet:
    """--constraints_json: the file's lists by image id, checked against the vocabulary when it is loaded; the satisfied / total
    counts of the decoded images, and their summary"""

    def __init__(self, by_id, vocab, oov='error'):
        if oov not in ('error', 'drop'):
            raise ValueError("--constraints_oov is 'error' or 'drop', got %r" % (oov,))
        known = set(vocab.values())
        self.by_id, self.dropped_words, self.dropped_constraints, self.rows = {}, 0, 0, []
        missing = sorted({w for cons in by_id.values() for ws in cons for w in ws if w not in known})
        if missing and oov == 'error':
            raise ValueError('--constraints_json: words that are not in the vocabulary (--constraints_oov drop leaves them out): %s'
                             % ', '.join(repr(w) for w in missing))
        for key, cons in by_id.items():
            kept = []
            for ws in cons:
                ok = [w for w in ws if w in known]
                self.dropped_words += len(ws) - len(ok)
                if ok:
                    kept.append(ok)
                else:
                    self.dropped_constraints += 1
            self.by_id[str(key)] = kept
        if oov == 'drop':
            print('--constraints_oov drop: %d words outside the vocabulary dropped, %d constraints left empty and dropped'
                  % (self.dropped_words, self.dropped_constraints))

    @classmethod
    def load(cls, opt, vocab):
        path = getattr(opt, 'constraints_json', '')
        if not path:
            return None
        with open(path) as f:
            return cls(json.load(f), vocab, getattr(opt, 'constraints_oov', 'error'))

    def for_batch(self, infos):
        return [self.by_id.get(str(info['id']), []) for info in infos]

    def add_batch(self, last, infos, keep):
        sat, total = last['satisfied'].tolist(), last['total'].tolist()                 # one small transfer each per batch
        self.rows += [(info['id'], sat[i], total[i]) for i, info in enumerate(infos[:keep])]
        return sat, total

    def summary(self):
        con = [(s, t) for _, s, t in self.rows if t > 0]
        return {'images': len(self.rows), 'constrained_images': len(con),
                'fully_satisfied': (sum(1 for s, t in con if s == t) / len(con)) if con else 1.0,
                'mean_satisfied_fraction': (sum(s / t for s, t in con) / len(con)) if con else 1.0,
                'dropped_words': self.dropped_words, 'dropped_constraints': self.dropped_constraints}

    def write(self, opt, split):
        out_dir = getattr(opt, 'eval_results_dir', 'eval_results')
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, '%s_%s_cbs.json' % (getattr(opt, 'id', 'capmi'), split))
        with open(path, 'w') as f:
            json.dump({'overall': self.summary(),
                       'images': [{'image_id': i, 'constraints_satisfied': s, 'constraints_total': t} for i, s, t in self.rows]}, f)
        return path


class Distractors:
    """--disc_lambda: the distractors of every eval batch (disc.pick_nearest / disc.pick_random), the decode options that carry them,
    and the image ids they stand for, per evaluated image"""

    PICKS = ('nearest', 'random')

    def __init__(self, lam, D=1, mode='suppress', pick='nearest', seed=1234):
        from imagecaptioning.pytorch_amd import disc
        if not 0.0 <= float(lam) <= 1.0:
            raise ValueError('--disc_lambda lies in [0, 1], got %r' % (lam,))
        if not 1 <= int(D) <= disc.D_MAX:
            raise ValueError('--disc_distractors is a number of images in 1..%d, got %r' % (disc.D_MAX, D))
        if mode not in disc.MODES:
            raise ValueError("--disc_mode is 'suppress' or 'listener', got %r" % (mode,))
        if pick not in self.PICKS:
            raise ValueError("--disc_pick is 'nearest' or 'random', got %r" % (pick,))
        self.lam, self.D, self.mode, self.pick, self.seed = float(lam), int(D), mode, pick, int(seed)
        self.gen = torch.Generator().manual_seed(self.seed)
        self.rows = {}

    @classmethod
    def load(cls, opt):
        lam = getattr(opt, 'disc_lambda', -1.0)
        if lam is None or lam < 0:
            return None
        return cls(lam, getattr(opt, 'disc_distractors', 1), getattr(opt, 'disc_mode', 'suppress'), getattr(opt, 'disc_pick', 'nearest'),
                   getattr(opt, 'seed', 1234))

    def for_batch(self, att, att_masks, infos, keep):
        """-> the decode options of this batch; the kept images' distractor ids are noted (one small transfer per batch)"""
        from imagecaptioning.pytorch_amd import disc
        if self.pick == 'nearest':
            table = disc.pick_nearest(att, att_masks, self.D)
        else:
            table = disc.pick_random(att.shape[0], self.D, self.gen)
        for k, row in enumerate(table.tolist()[:keep]):
            self.rows[infos[k]['id']] = [infos[j]['id'] for j in row if j >= 0]
        return dict(distractors=table, disc_lambda=self.lam, disc_mode=self.mode)

    def settings(self):
        return {'disc_lambda': self.lam, 'disc_distractors': self.D, 'disc_mode': self.mode, 'disc_pick': self.pick, 'seed': self.seed}

    def write(self, opt, split):
        path = _results_path(opt, split, 'disc.json')
        with open(path, 'w') as f:
            json.dump({'settings': self.settings(),
                       'images': [{'image_id': i, 'distractors': d} for i, d in self.rows.items()]}, f)
        return path


def _results_path(opt, split, suffix):
    out_dir = getattr(opt, 'eval_results_dir', 'eval_results')
    os.makedirs(out_dir, exist_ok=True)
    return os.path.join(out_dir, '%s_%s_%s' % (getattr(opt, 'id', 'capmi'), split, suffix))


class SelfRetrieval:
    """--self_retrieval: the evaluated images are collected into pools of `pool` consecutive images (features and first captions
    stay on the device); a full pool -- and at the end the rest -- is scored caption by image (score.score_captions, pairing
    'cross') and ranked (capmi_retrieval_rank).  The predictions of the pool gain their rank and log-posterior then."""

    def __init__(self, pool, norm='none'):
        from imagecaptioning.pytorch_amd import score
        if int(pool) < 1:
            raise ValueError('--retrieval_pool is a number of images >= 1, got %r' % (pool,))
        if norm not in score.NORMS:
            raise ValueError("--score_norm is 'none' or 'length', got %r" % (norm,))
        self.pool, self.norm = int(pool), norm
        self.pending, self.ranks, self.sizes = [], [], []

    @classmethod
    def load(cls, opt, cons, rerank_kw):
        if not getattr(opt, 'self_retrieval', 0):
            return None
        if cons is not None:
            raise NotImplementedError('--self_retrieval does not combine with --constraints_json: a caption that was made to contain '
                                      'given words says nothing about how well the model tells the images apart')
        if opt.sample_n > 1 and not rerank_kw:
            raise NotImplementedError('--self_retrieval ranks ONE caption per image: with --sample_n > 1 say which one with --rerank '
                                      '(the first of sample_n sampled captions is an arbitrary one)')
        return cls(getattr(opt, 'retrieval_pool', 1000), getattr(opt, 'score_norm', 'none'))

    def add_batch(self, model, fc, att, att_masks, seq_first, preds):
        """the kept images of a batch: their features, first captions [keep, L] and prediction dicts, in order"""
        for k, p in enumerate(preds):
            self.pending.append((fc[k], att[k], None if att_masks is None else att_masks[k], seq_first[k], p))
            if len(self.pending) == self.pool:
                self._flush(model)

    def finish(self, model):
        if self.pending:
            self._flush(model)

    def _flush(self, model):
        from imagecaptioning.pytorch_amd import ops, score
        items, self.pending = self.pending, []
        k, K = len(items), max(it[1].shape[0] for it in items)
        fc = torch.stack([it[0] for it in items])
        att = torch.stack([torch.nn.functional.pad(it[1], (0, 0, 0, K - it[1].shape[0])) for it in items])
        masks = None
        if any(it[2] is not None or it[1].shape[0] != K for it in items):       # ragged pools: the loader's masks, padded
            masks = att.new_zeros(k, K)
            for j, it in enumerate(items):
                if it[2] is None:
                    masks[j, :it[1].shape[0]] = 1
                else:
                    masks[j, :it[2].shape[0]] = it[2]
        seqs = torch.stack([it[3] for it in items]).long()
        S = score.score_captions(model, fc, att, masks, seqs, {'pairing': 'cross', 'score_norm': self.norm})
        rank, post = ops.retrieval_rank(S, torch.arange(k))
        rank, post = rank.tolist(), post.tolist()                                # one transfer each per pool
        for j, it in enumerate(items):
            it[4].update(retrieval_rank=rank[j], retrieval_log_post=post[j])
        self.ranks += rank
        self.sizes.append(k)

    def summary(self):
        from imagecaptioning.pytorch_amd import score
        return dict(score.retrieval_summary(self.ranks, self.pool, len(self.sizes)), pool_sizes=self.sizes, score_norm=self.norm)

    def write(self, opt, split):
        path = _results_path(opt, split, 'ret.json')
        with open(path, 'w') as f:
            json.dump({'overall': self.summary(), 'ranks': self.ranks}, f)
        return path


class CaptionScores:
    """--score_json: the file's captions by image id as token rows; the scores of the images the pass met, and those it did not"""

    def __init__(self, by_id, vocab, L, oov='error', norm='none'):
        from imagecaptioning.pytorch_amd import score
        if norm not in score.NORMS:
            raise ValueError("--score_norm is 'none' or 'length', got %r" % (norm,))
        self.norm, self.by_id, self.done, self.L = norm, {}, {}, L
        for key, caps in by_id.items():
            caps = [caps] if isinstance(caps, str) else list(caps)
            if not caps:
                continue
            rows, missing = score.encode_captions(caps, vocab, L, 'drop' if oov == 'drop' else 'unk')
            self.by_id[str(key)] = (caps, rows, missing)

    @classmethod
    def load(cls, opt, vocab, L):
        path = getattr(opt, 'score_json', '')
        if not path:
            return None
        with open(path) as f:
            return cls(json.load(f), vocab, L, getattr(opt, 'constraints_oov', 'error'), getattr(opt, 'score_norm', 'none'))

    def add_batch(self, model, fc, att, att_masks, infos, keep):
        idx = [k for k in range(keep) if str(infos[k]['id']) in self.by_id and str(infos[k]['id']) not in self.done]
        if not idx:
            return
        n = max(self.by_id[str(infos[k]['id'])][1].shape[0] for k in idx)
        seqs = torch.zeros(len(idx), n, self.L, dtype=torch.long)          # images with fewer captions: empty rows, not reported
        for j, k in enumerate(idx):
            rows = self.by_id[str(infos[k]['id'])][1]
            seqs[j, :rows.shape[0]] = rows
        sel = torch.tensor(idx, device=fc.device)
        out = model(fc[sel], att[sel], seqs.to(fc.device), None if att_masks is None else att_masks[sel], mode='score',
                    opt={'score_norm': self.norm})
        last = model.last_score
        val, logp, ln, ppl = out.tolist(), last['logp'].tolist(), last['len'].tolist(), last['perplexity'].tolist()
        for j, k in enumerate(idx):
            caps, rows, missing = self.by_id[str(infos[k]['id'])]
            self.done[str(infos[k]['id'])] = [
                {'caption': c, 'score': val[j][i], 'logp': logp[j][i], 'len': ln[j][i], 'perplexity': ppl[j][i], 'oov_words': missing[i]}
                for i, c in enumerate(caps)]

    def missing_ids(self):
        return sorted(k for k in self.by_id if k not in self.done)

    def write(self, opt, split):
        path = _results_path(opt, split, 'scores.json')
        with open(path, 'w') as f:
            json.dump({'score_norm': self.norm, 'images': self.done, 'missing_image_ids': self.missing_ids()}, f)
        return path


class AttentionDump:
    """--dump_attention: the first caption row of every image of a batch, as ONE device-to-host transfer (every array of
    model.last_attention packed into one float32 block), kept by image id and written as one .npz"""

    def __init__(self):
        self.arrays = {}

    def add_batch(self, last, infos, keep, att_masks, boxes, col0):
        att = last['att']
        N, L, Kw = att.shape
        B = len(infos)
        rows = slice(0, N, max(N // B, 1))                   # the first row of each image: the caption that is reported
        parts = [att[rows], last['top'][rows].to(att.dtype).unsqueeze(2), last['top_w'][rows].unsqueeze(2),
                 last['entropy'][rows].unsqueeze(2)]
        regions = att.new_full((B, L, 1), Kw - col0) if att_masks is None else \
            att_masks.to(att.dtype).sum(1).view(B, 1, 1).expand(B, L, 1)
        parts.append(regions)
        if boxes is not None:
            # the top region's own box: column top - col0 of the image's boxes (zeros for the sentinel column and on zeroed steps)
            k = last['top'][rows].long() - col0
            own = boxes.gather(1, k.clamp(min=0).unsqueeze(2).expand(B, L, 4)) * (k >= 0).unsqueeze(2).to(att.dtype)
            parts += [last['box'][rows], own]
        host = torch.cat(parts, 2).cpu().numpy()            # the one transfer
        for i, info in enumerate(infos[:keep]):              # images past num_images are left out, like their predictions
            h, key = host[i], str(info['id'])
            n_reg = int(h[0, Kw + 3])
            self.arrays[key + '/att'] = h[:, :n_reg + col0].copy()
            self.arrays[key + '/top'] = h[:, Kw].astype('int32')
            self.arrays[key + '/top_w'] = h[:, Kw + 1].copy()
            self.arrays[key + '/entropy'] = h[:, Kw + 2].copy()
            self.arrays[key + '/regions'] = h[0, Kw + 3].astype('int32')
            if boxes is not None:
                self.arrays[key + '/box'] = h[:, Kw + 4:Kw + 8].copy()
                self.arrays[key + '/top_box'] = h[:, Kw + 8:Kw + 12].copy()

    def write(self, opt, split):
        import numpy as np
        out_dir = getattr(opt, 'eval_results_dir', 'eval_results')
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, '%s_%s_att.npz' % (getattr(opt, 'id', 'capmi'), split))
        np.savez(path, **self.arrays)
        return path


def eval_split(model, crit, loader, opt):
    from captioning.utils import misc
    dev = next(model.parameters()).device
    model.eval()
    n, loss_sum, loss_n, preds, n_preds = 0, 0.0, 0, [], []
    split = getattr(opt, 'split', 'val')
    lang = None
    if getattr(opt, 'language_eval', 0):
        from imagecaptioning.pytorch_amd.langeval import LanguageEval
        lang = LanguageEval.for_loader(loader, split, dev)
    rerank_kw = rerank_kwargs(opt)
    redump = RerankDump() if rerank_kw else None
    sample_n = 1 if rerank_kw else opt.sample_n      # --rerank: the sample_n captions become one, the pass is the single-caption one
    div, groups = None, []               # groups: (image_id, the image's n prediction dicts in slot order), before any sorting
    if lang is not None and sample_n > 1:
        from imagecaptioning.pytorch_amd.diveval import DiversityEval
        div = DiversityEval(lang, sample_n, oracle=bool(getattr(opt, 'eval_oracle', 0)))
    sent = None
    if lang is not None and getattr(opt, 'sentence_stats', 0):
        from imagecaptioning.pytorch_amd.sentstats import SentenceStats
        sent = SentenceStats.for_loader(loader, split, dev, model, sample_n)
    dump = AttentionDump() if getattr(opt, 'dump_attention', 0) else None
    cons = ConstraintSet.load(opt, model.vocab)
    if getattr(opt, 'bad_words_json', '') or getattr(opt, 'bad_words', None):
        # --bad_words "a man" top ... and --bad_words_json FILE: word sequences -> opt['bad_words'], token-id sequences
        from imagecaptioning.pytorch_amd import logits_proc
        oov = getattr(opt, 'constraints_oov', 'error')
        ids = logits_proc.bad_word_ids(list(getattr(opt, 'bad_words', None) or []), model.vocab, oov)
        if getattr(opt, 'bad_words_json', ''):
            ids = ids + [e for e in logits_proc.bad_words_from_file(opt.bad_words_json, model.vocab, oov) if e not in ids]
        opt.bad_words = ids
    if cons is not None and (rerank_kw or opt.sample_n > 1):
        raise NotImplementedError('--constraints_json decodes one caption per image: it does not combine with --sample_n > 1 or --rerank')
    retr = SelfRetrieval.load(opt, cons, rerank_kw)
    given = CaptionScores.load(opt, model.vocab, model.seq_length)
    dist = Distractors.load(opt)
    if dist is not None and dump is not None:
        raise NotImplementedError('--dump_attention does not combine with --disc_lambda: a discriminative call steps every '
                                  'hypothesis under several images and keeps no per-word attention')
    if hasattr(loader, 'reset_iterator'):
        loader.reset_iterator(split)                                                                           # eval_utils.py:145
    num_images = opt.num_images
    while num_images < 0 or n < num_images:
        data = loader.get_batch(split)
        # eval_utils.py:200-207: ix1 = min(it_max, num_images) -- never more than the split holds (a larger request would make the
        # non-wrapping loader start the split over and every image would be predicted twice)
        num_images = data['bounds']['it_max'] if num_images < 0 else min(num_images, data['bounds']['it_max'])
        # eval_utils.py:157-159: fc_feats, att_feats, labels, masks AND att_masks go to the device -- with 10..100 adaptive
        # regions per image the padded rows of att_feats must stay out of the attention (None when the batch is not ragged)
        fc, att, labels, masks = (data[k].to(dev) for k in ('fc_feats', 'att_feats', 'labels', 'masks'))
        att_masks = None if data.get('att_masks') is None else data['att_masks'].to(dev)
        kw = eval_kwargs_of(opt)
        kw['sample_n'] = 1                                                                                     # :169-170
        kw.update(rerank_kw)
        if cons is not None:
            kw['constraints'] = cons.for_batch(data['infos'])
        disc_kw = {}
        if dist is not None:
            disc_kw = dist.for_batch(att, att_masks, data['infos'], max(0, min(len(data['infos']), num_images - n)))
            kw.update(disc_kw)
        if dump is not None:
            kw['return_attention'] = 1
            boxes = batch_boxes(loader, opt, data, att.shape[1], dev)
            if boxes is not None:
                kw['boxes'] = boxes
        with torch.no_grad():
            loss = crit(model(fc, att, labels[..., :-1], att_masks), labels[..., 1:], masks[..., 1:]).item()  # eval_utils.py:163
            seq, seq_logp = model(fc, att, att_masks, mode='sample', opt=kw)                                   # :171
        if dump is not None:
            dump.add_batch(model.last_attention, data['infos'], max(0, min(len(data['infos']), num_images - n)), att_masks,
                           kw.get('boxes'), model._trace_col0)
        if redump is not None:
            redump.add_batch(model.last_rerank, data['infos'], max(0, min(len(data['infos']), num_images - n)))
            mbr_choice = model.last_rerank['choice'].tolist()
            mbr_expected = model.last_rerank['expected'].gather(1, model.last_rerank['choice'].long().unsqueeze(1)).squeeze(1).tolist()
        if cons is not None:
            cbs_sat, cbs_total = cons.add_batch(model.last_cbs, data['infos'], max(0, min(len(data['infos']), num_images - n)))
        loss_sum += loss
        loss_n += 1
        if seq_logp.dim() == 3:
            # eval_utils.py:173-174: sums over ALL L steps (rows after the end are zero) over (#tokens + 1); the only deviation:
            # 0 * -inf of a constrained token counts as 0 instead of making the whole caption's entropy NaN.  r6: one pass of
            # capmi_caption_stats over the log-probs the decode returned -- the ATen formula built three dense [N, L, V1] temporaries
            from imagecaptioning.pytorch_amd import ops
            entropy, perplexity = ops.caption_stats(seq_logp.contiguous(), seq.contiguous())
        else:                                  # _diverse_sample returns the chosen tokens' log-probs only (AttModel.py:449)
            entropy = perplexity = torch.full((seq.shape[0],), float('nan'))
        if opt.beam_size > 1 and getattr(opt, 'verbose_beam', 0) and cons is None:                                             # :177-181
            for i in range(fc.shape[0]):
                print('\n'.join(misc.decode_sequence(model.vocab, b['seq'].unsqueeze(0))[0] for b in model.done_beams[i]))
                print('--' * 10)
        sents = misc.decode_sequence(model.vocab, seq)
        rows_per_image = max(1, len(sents) // len(data['infos']))
        if lang is not None:
            # the first row of each image, images past num_images left out (eval_utils.py:209-210 pops their predictions); the rows
            # stay on the device, nothing is read back before lang.compute()
            keep = max(0, min(len(data['infos']), num_images - n))
            lang.add_batch(data['infos'][:keep], seq[::rows_per_image][:keep])
            if sent is not None:
                sent.add_first(seq[::rows_per_image][:keep], perplexity[::rows_per_image][:keep], entropy[::rows_per_image][:keep])
        first_pred = len(preds)
        for k, s in enumerate(sents):
            preds.append({'image_id': data['infos'][k // rows_per_image]['id'], 'caption': s, 'perplexity': perplexity[k].item(),
                          'entropy': entropy[k].item()})
            if redump is not None:
                preds[-1].update(mbr_choice=mbr_choice[k], mbr_expected=mbr_expected[k])
            if cons is not None:
                preds[-1].update(constraints_satisfied=cbs_sat[k], constraints_total=cbs_total[k])
            if dist is not None:
                preds[-1]['distractors'] = dist.rows.get(preds[-1]['image_id'], [])
        if retr is not None or given is not None:
            kept = max(0, min(len(data['infos']), num_images - n))
            if retr is not None:
                retr.add_batch(model, fc, att, att_masks, seq[::rows_per_image][:kept], preds[first_pred::rows_per_image][:kept])
            if given is not None:
                given.add_batch(model, fc, att, att_masks, data['infos'], kept)
        if sample_n > 1:                                                                                       # :199-200
            first = len(n_preds)
            rows = eval_split_n(model, n_preds, fc, att, att_masks, data, opt, disc_kw)                       # :198
            if dist is not None:
                for p in n_preds[first:]:
                    p['distractors'] = dist.rows.get(p['image_id'], [])
            if div is not None:          # the same cut at num_images as the single-caption pass; the rows stay on the device
                div.add_batch(data['infos'][:keep], rows[:keep])
                if sent is not None:
                    sent.add(rows[:keep])
                groups += [(data['infos'][k]['id'], n_preds[first + k * opt.sample_n:first + (k + 1) * opt.sample_n])
                           for k in range(keep)]
        n += len(data['infos'])
    if n_preds and 'perplexity' in n_preds[0]:
        n_preds = sorted(n_preds, key=lambda x: x['perplexity'])                                               # :217-218
    if dump is not None:
        print('attention written to', dump.write(opt, split))
    if redump is not None:
        print('reranking written to', redump.write(opt, split))
    if cons is not None:
        print('constraints: %s written to %s' % (cons.summary(), cons.write(opt, split)))
    if dist is not None:
        print('discriminative decoding: %s written to %s' % (dist.settings(), dist.write(opt, split)))
    if retr is not None:
        retr.finish(model)
        print('self-retrieval: %s written to %s' % (retr.summary(), retr.write(opt, split)))
    if given is not None:
        if given.missing_ids():
            print('--score_json: %d image ids of the file are not among the evaluated images of split %r: %s'
                  % (len(given.missing_ids()), split, ', '.join(given.missing_ids())))
        print('caption scores written to', given.write(opt, split))
    model.n_predictions = n_preds
    model.train()                                                                                              # :224-225
    preds = preds[:num_images * max(1, len(preds) // max(n, 1))]
    if lang is not None:
        lang_stats = language_eval(lang, preds, opt, split, sent)
        if div is not None:
            lang_stats.update(language_eval_n(div, groups, opt, split))
        return loss_sum / max(loss_n, 1), preds, lang_stats
    return loss_sum / max(loss_n, 1), preds


def language_eval(lang, preds, opt, split, sent=None):
    """eval_utils.language_eval (:47-125) for the Java-free scorers: lang_stats = {'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'}, written
    with the per-image CIDEr and caption as {'overall', 'imgToEval'} to <eval_results_dir>/<id>_<split>.json (:122-124).  sent: a
    sentstats.SentenceStats of the same rows; its numbers join lang_stats before the file is written."""
    lang_stats, img_cider = lang.compute()
    if sent is not None:
        lang_stats.update(sent.compute())
    img_to_eval = {}
    for p in preds:                                            # one entry per image: the first caption, the one that was scored
        pos = lang.pos_of_id.get(p['image_id'])
        if pos is not None and p['image_id'] not in img_to_eval and img_cider[pos] == img_cider[pos]:
            img_to_eval[p['image_id']] = {'image_id': p['image_id'], 'CIDEr': float(img_cider[pos]), 'caption': p['caption']}
    out_dir = getattr(opt, 'eval_results_dir', 'eval_results')
    os.makedirs(out_dir, exist_ok=True)
    out = {'overall': lang_stats, 'imgToEval': img_to_eval}
    from imagecaptioning.pytorch_amd import logits_proc
    settings = {k: getattr(opt, k) for k in logits_proc.KEYS if hasattr(opt, k)}
    if logits_proc.wanted(settings):
        out['logits_processors'] = settings            # the settings the captions were decoded with; absent when all are off
    with open(os.path.join(out_dir, '%s_%s.json' % (getattr(opt, 'id', 'capmi'), split)), 'w') as f:
        json.dump(out, f)
    return lang_stats


def assemble_n(overall, per_image, groups, pos_of_id, oracle):
    """The reference's <id>_<split>_n.json (eval_utils.py:104-119) from DiversityEval.compute(): {'div_stats': eval_div_stats's
    {'overall', 'ImgToEval'}, 'self_cider': eval_self_cider's {'overall', 'imgToEval'}[, 'oracle': eval_oracle's {'overall',
    'ImgToEval'}]}.  groups: (image_id, the image's prediction dicts in slot order); as in the reference each dict gains its
    'mBleu_2' (and, with oracle, its 'scores')."""
    from imagecaptioning.pytorch_amd.diveval import DIV_KEYS, ORACLE_KEYS
    oracle_keys = [p + k for k in ORACLE_KEYS for p in ('oracle_', 'avg_')]
    out = {'div_stats': {'overall': {k: overall[k] for k in DIV_KEYS}, 'ImgToEval': {}},
           'self_cider': {'overall': {'self_cider': overall['self_cider']}, 'imgToEval': {}}}
    if oracle:
        out['oracle'] = {'overall': {k: overall[k] for k in oracle_keys}, 'ImgToEval': {}}
    for image_id, caps in groups:
        pos = pos_of_id[image_id]
        for j, p in enumerate(caps):
            p['mBleu_2'] = float(per_image['individual_mBleu_2'][pos, j])
            if oracle:
                p['scores'] = {k: float(per_image['scores'][pos, j, x]) for x, k in enumerate(ORACLE_KEYS)}
        out['div_stats']['ImgToEval'][image_id] = {'mBleu_2': float(per_image['mBleu_2'][pos]), 'individuals': caps}
        out['self_cider']['imgToEval'][image_id] = {'self_cider': float(per_image['self_cider'][pos]),
                                                    'self_cider_mat': per_image['self_cider_mat'][pos].tolist()}
        if oracle:
            entry = {k: float(per_image[k][pos]) for k in oracle_keys}
            entry['captions'] = caps
            out['oracle']['ImgToEval'][image_id] = entry
    return out


def language_eval_n(div, groups, opt, split):
    """the diversity half of eval_utils.language_eval (:104-119): the overall numbers, <eval_results_dir>/<id>_<split>_n.json"""
    overall, per_image = div.compute()
    out_dir = getattr(opt, 'eval_results_dir', 'eval_results')
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, '%s_%s_n.json' % (getattr(opt, 'id', 'capmi'), split)), 'w') as f:
        json.dump(assemble_n(overall, per_image, groups, div.pos_of_id, div.oracle), f)
    return overall


def build_loader(opt, dev):
    """tools/eval.py:97-104: the reference evaluates on its DataLoader (precomputed bottom-up features, 10-100 regions per image
    => ragged batches with att_masks).  --input_json selects the same real-file loader tools/train.py uses (FeatureLoader, kept
    resident in HBM unless --resident_features 0); without it the synthetic fixed-36-region loader stands in."""
    if getattr(opt, 'input_json', ''):
        from captioning.data.feature_loader import FeatureLoader
        loader = FeatureLoader(opt)
        loader.check_att_feat_size(getattr(opt, 'att_feat_size', 0))     # use_box: rows are 5 wider than the feature files
        opt.vocab_size, opt.seq_length = loader.vocab_size, loader.seq_length
        if not getattr(opt, 'max_length', None) or opt.max_length > opt.seq_length:
            opt.max_length = opt.seq_length
        vocab = loader.get_vocab()
        if getattr(opt, 'resident_features', 1):
            from captioning.data.resident import ResidentFeatures
            budget = int(opt.resident_budget_gb * (1 << 30)) if getattr(opt, 'resident_budget_gb', 0) > 0 else None
            loader = ResidentFeatures(loader, dev, budget_bytes=budget, dtype=getattr(opt, 'resident_dtype', 'fp32'))
        return loader, vocab
    from captioning.data.synthetic_loader import SyntheticLoader
    loader = SyntheticLoader(opt)
    return loader, loader.get_vocab()


def main(opt):
    from captioning import models
    from captioning.modules import losses
    dev = torch.device(opt.device if opt.device != 'cuda' else 'cuda:0')
    loader, opt.vocab = build_loader(opt, dev)
    torch.manual_seed(1234)
    model = models.setup(opt).to(dev)
    if getattr(opt, 'model', ''):       # tools/eval.py:25, :96 --model: one state-dict file by path (a run's model_ema.pth, model-best.pth, ...)
        model.load_state_dict(torch.load(opt.model, map_location=dev))
    elif opt.start_from:
        model.load_state_dict(torch.load(os.path.join(opt.start_from, 'model.pth'), map_location=dev))
    if getattr(opt, 'rerank', '') == 'mbr_ciderd':
        # the document frequencies of the CIDEr-D reward, as tools/train.py finds them: the prepro_ngrams pickle (or its converted
        # image) when it exists, else the same table rebuilt from the training references
        from captioning.utils import rewards
        ct = str(opt.cached_tokens)
        have = any(os.path.exists(p_) for p_ in (ct, os.path.join('data', ct + '.p'), os.path.join('data', ct + '.capmi.npz')))
        rewards.init_scorer(ct if (opt.input_json and have) else loader.document_frequency(), device=dev)
    crit =losses.LabelSmoothing(smoothing=opt.label_smoothing) if opt.label_smoothing > 0 else losses.LanguageModelCriterion()
    res = eval_split(model, crit, loader, opt)
    report(res)
    return res


def report(res):
    """tools/eval.py:107-109: the loss, the first captions, and lang_stats when the pass computed them"""
    print('loss: ', res[0])
    for p in res[1][:5]:
        print('image %s: %s' % (p['image_id'], p['caption']))
    if len(res) > 2:
        print(res[2])
        print('(METEOR and SPICE are absent: they need Java)')


if __name__ == '__main__':
    from captioning.utils import opts
    main(opts.parse_opt())
