#!/usr/bin/env python3
"""Test-time ensemble evaluation on the MI355X backend -- the reference's tools/eval_ensemble.py on top of tools/eval.py:
every --ids entry names a training run's log directory, log_<id>/infos_<id>[-suffix].pkl and log_<id>/model[-suffix].pth
(an id may carry a -suffix: the checkpoint misc.save_checkpoint(..., append=suffix) wrote).  Each member is rebuilt from its own
infos' options, the vocabulary comes from the first infos, the ensemble (captioning.models.AttEnsemble) decodes for max_length
steps, and eval.eval_split reports the validation loss of the teacher-forced ensemble and the captions (with --language_eval 1
also lang_stats: corpus CIDEr, BLEU-1..4 and ROUGE-L, as tools/eval.py).

    python -m imagecaptioning.pytorch_amd.tools.eval_ensemble --ids A B-best --weights 0.5 0.5 --beam_size 5 [--log_root DIR]

Eval options (beam_size, sample_method, num_images, ...) come from the command line; model and data options from the first
member's infos unless given on the command line.
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# the options of the reference's add_eval_options / add_diversity_opts: command line or default, never the training run's
EVAL_KEYS = ('beam_size', 'sample_method', 'temperature', 'suppress_UNK', 'length_penalty', 'group_size', 'diversity_lambda',
             'decoding_constraint', 'block_trigrams', 'remove_bad_endings', 'max_length', 'num_images', 'device', 'sample_n',
             'sample_n_method', 'verbose_beam', 'split', 'language_eval', 'eval_results_dir', 'eval_oracle',
             'sentence_stats', 'penalty_alpha', 'contrastive_k', 'no_repeat_ngram_size', 'repetition_penalty', 'min_length',
             'bad_words', 'bad_words_json')


def split_id(entry):
    """'a' -> ('a', ''), 'a-best' -> ('a', 'best')"""
    id_, _, suffix = entry.partition('-')
    return id_, suffix


def member_paths(ids, log_root='.'):
    """[(log dir, id, suffix, infos path, model path)] of the --ids entries (eval_ensemble.py:38-46)"""
    out = []
    for entry in ids:
        id_, suffix = split_id(entry)
        app = ('-' + suffix) if suffix else ''
        d = os.path.join(log_root, 'log_%s' % id_)
        out.append((d, id_, suffix, os.path.join(d, 'infos_%s%s.pkl' % (id_, app)), os.path.join(d, 'model%s.pth' % app)))
    return out


def parse_args(argv=None):
    """(ids, weights, log_root, explicit options): the options parse like tools/eval.py's, but only those given on the command
    line are returned, so that the others can come from the members' infos"""
    from captioning.utils import opts
    ap = argparse.ArgumentParser()
    ap.add_argument('--ids', nargs='+', required=True, help='id[-suffix] of the runs to ensemble')
    ap.add_argument('--weights', nargs='+', type=float, default=None, help='one weight per id (default: all equal)')
    ap.add_argument('--log_root', type=str, default='.', help='directory holding the log_<id> directories')
    for k, v in opts.DEFAULTS.items():
        opts.add_flag(ap, k, v)
    ns = ap.parse_args(argv)
    explicit = {k: getattr(ns, k) for k in opts.DEFAULTS if getattr(ns, k) is not None}
    return ns.ids, ns.weights, ns.log_root, explicit


def build_opt(infos0, explicit):
    """defaults < first member's options (model / data) < command line; eval options: defaults < command line"""
    from captioning.utils import opts
    opt = dict(opts.DEFAULTS)
    opt.update({k: v for k, v in vars(infos0['opt']).items() if k not in EVAL_KEYS})
    opt.update(explicit)
    o = argparse.Namespace(**opt)
    if o.max_length is None:
        o.max_length = o.seq_length
    return o


def main(argv=None):
    from captioning import models
    from captioning.models import AttEnsemble
    from captioning.modules import losses
    from captioning.utils import misc
    from imagecaptioning.pytorch_amd.tools import eval as E
    ids, weights, log_root, explicit = parse_args(argv)
    paths = member_paths(ids, log_root)
    infos = [misc.load_infos_suffixed(d, id_, suffix) for d, id_, suffix, _, _ in paths]
    opt = build_opt(infos[0], explicit)
    dev = torch.device(opt.device if opt.device != 'cuda' else 'cuda:0')
    loader, _ = E.build_loader(opt, dev)
    vocab = infos[0]['vocab']                                           # eval_ensemble.py:64
    members = []
    for inf, (_, _, _, _, model_path) in zip(infos, paths):
        mopt = argparse.Namespace(**vars(inf['opt']))
        mopt.start_from, mopt.vocab = None, vocab                       # :72-73
        m = models.setup(mopt).to(dev)
        m.load_state_dict(torch.load(model_path, map_location=dev))
        members.append(m)
    model = AttEnsemble(members, weights=weights).to(dev)
    model.seq_length = opt.max_length                                   # :82
    model.eval()
    if hasattr(loader, 'ix_to_word'):
        loader.ix_to_word = vocab                                       # :96
    opt.vocab = vocab
    opt.id = '+'.join('%s%s' % (i, w) for i, w in zip(ids, weights or [1.0] * len(ids)))   # :98
    crit = losses.LanguageModelCriterion()                              # :84
    res = E.eval_split(model, crit, loader, opt)           # (loss, preds), or (loss, preds, lang_stats) with --language_eval 1
    E.report(res)
    return res


if __name__ == '__main__':
    main()
