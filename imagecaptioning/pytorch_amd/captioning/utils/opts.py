"""Option parsing for the entrypoints: the subset of the reference's flags (captioning/utils/opts.py:18-277) that
the hot path reads, with the reference's defaults; ``--cfg`` yaml files (with ``_BASE_``) and CLI overrides are
applied in the reference's order (defaults < yaml < CLI)."""
import argparse

from . import config

DEFAULTS = dict(
    caption_model='updown', rnn_size=512, num_layers=1, input_encoding_size=512, att_hid_size=512, fc_feat_size=2048,
    att_feat_size=2048, logit_layers=1, use_bn=0, drop_prob_lm=0.5, seq_length=20, max_length=20, seq_per_img=5, batch_size=10,
    max_epochs=-1, max_iters=100, learning_rate=4e-4, optim='adam', optim_alpha=0.9, optim_beta=0.999, optim_epsilon=1e-8,
    weight_decay=0.0, grad_clip_mode='value', grad_clip_value=0.1, label_smoothing=0.0, self_critical_after=-1, structure_after=-1,
    structure_loss_weight=1.0, structure_loss_type='seqnll', train_sample_n=16, train_sample_method='sample', train_beam_size=1,
    sc_sample_method='greedy', sc_beam_size=1, cider_reward_weight=1.0, bleu_reward_weight=0.0, cached_tokens='coco-train-idxs',
    use_ppo=0, entropy_reward_weight=0.0, self_cider_reward_weight=0.0, struc_use_logsoftmax=0, drop_worst_after=-1, drop_worst_rate=0.0,
    ppo_old_model_path=None, ppo_cliprange=0.2, ppo_kl_coef=0.02,                       # opts.py:189-196
    learning_rate_decay_start=-1, learning_rate_decay_every=3, learning_rate_decay_rate=0.8, noamopt=0, noamopt_warmup=2000,
    noamopt_factor=1.0, use_warmup=0, reduce_on_plateau=0, reduce_on_plateau_factor=0.5, reduce_on_plateau_patience=3,
    scheduled_sampling_start=-1, scheduled_sampling_increase_every=5, scheduled_sampling_increase_prob=0.05,
    scheduled_sampling_max_prob=0.25, val_every=0, val_images=0,
    # exponential moving average of the weights (flat.FlatParams.enable_ema; not a flag of the reference).  ema_decay 0: off -- no buffer,
    # no launch, no file.  ema_warmup: decay = min(ema_decay, (1 + step) / (10 + step)).  ema_eval: validate (and pick "best") on the
    # averaged weights.  Checkpoints gain model_ema[-best].pth, optimizer.pth carries the average
    ema_decay=0.0, ema_warmup=1, ema_eval=1,
    # knowledge distillation (losses.DistillCriterion / DistillTeacher; not a flag of the reference).  distill_from: id[-suffix] of saved
    # runs, named as tools/eval_ensemble.py --ids names them (log_<id>/ under distill_log_root); distill_weights: their mixture weights
    # (default: equal); distill_weight: lambda of (1 - lambda) NLL + lambda tau^2 KL(teacher || student), 0: off -- no teacher, no launch;
    # distill_temperature: tau
    distill_from=[], distill_weights=[], distill_weight=0.0, distill_temperature=1.0, distill_log_root='.',
    checkpoint_path='log_capmi', id='capmi', save_checkpoint_every=0, losses_log_every=10, start_from=None, seed=1234,
    # transformer / aoa
    N_enc=6, N_dec=6, d_model=512, d_ff=2048, num_att_heads=8, dropout=0.1, refine=1, refine_aoa=1, use_ff=0, decoder_type='AoA',
    use_multi_head=2, num_heads=8, multi_head_scale=1, mean_feats=1, ctx_drop=1, dropout_aoa=0.3, out_res=0,
    # eval
    beam_size=1, sample_method='greedy', temperature=1.0, suppress_UNK=1, length_penalty='', num_images=20, device='cuda',
    group_size=1, diversity_lambda=0.5, decoding_constraint=0, block_trigrams=0, remove_bad_endings=0, sample_n=1,
    # logits processors (imagecaptioning/pytorch_amd/logits_proc.py; not flags of the reference): hard n-gram blocking (0 off, 1..8),
    # the multiplicative penalty on words already emitted (1.0 off), the least caption length (0 off) and a JSON file of banned
    # word sequences (a list of strings or of word lists; words outside the vocabulary as constraints_oov says); bad_words: the
    # same on the command line, --bad_words "a man" top
    no_repeat_ngram_size=0, repetition_penalty=1.0, min_length=0, bad_words=[], bad_words_json='',
    sample_n_method='sample', verbose_beam=0,                                # opts.py:288-330 add_eval_sample_opts
    split='test',                                                            # opts.py:314 add_eval_options
    model='',                                                                # tools/eval.py:25 --model: the state-dict file tools/eval.py loads (else <start_from>/model.pth)
    # opts.py:127 / :311 language_eval: corpus CIDEr / BLEU-1..4 / ROUGE-L on the device (imagecaptioning/pytorch_amd/langeval.py; METEOR
    # and SPICE need Java).  eval_results_dir: where tools/eval.py writes <id>_<split>.json (the reference: always ./eval_results)
    language_eval=0, eval_results_dir='eval_results',
    # opts.py:331 eval_oracle: with language_eval and sample_n > 1, also oracle_X / avg_X over the sample_n captions (diveval.py)
    eval_oracle=1,
    # eval_utils.py:27-36, 55-68, 79-80, 121: with language_eval, also bad_count_rate and the mean perplexity / entropy and, with
    # sample_n > 1, novel_sentences and vocab_size, counted on the device (imagecaptioning/pytorch_amd/sentstats.py)
    sentence_stats=0,
    # tools/eval.py: write every decoded caption's per-word region attention (opt['return_attention'], imagecaptioning/pytorch_amd/
    # att_trace.py) to <eval_results_dir>/<id>_<split>_att.npz; updown / topdown, att2in2, adaatt, adaattmo
    dump_attention=0,
    # consensus (minimum-Bayes-risk) reranking of the sample_n captions of every image (opt['rerank'], imagecaptioning/pytorch_amd/mbr.py;
    # not a flag of the reference): '' off, 'mbr_ciderd' / 'mbr_bleu4' keep the caption with the highest expected CIDEr-D / BLEU-4
    # against the others; rerank_prior: 'uniform', or 'model' -- every candidate weighs as much as the model believes in it
    rerank='', rerank_prior='uniform',
    # constrained beam search (opt['constraints'], imagecaptioning/pytorch_amd/cbs.py; not a flag of the reference): constraints_json
    # names a file {"<image id>": [["zebra", "zebras"], ["grass"]], ...} of words the image's caption must contain (one of each
    # list); constraints_oov: 'error' stops at a word outside the vocabulary, 'drop' leaves such words out
    constraints_json='', constraints_oov='error',
    # scoring given captions (imagecaptioning/pytorch_amd/score.py; not flags of the reference).  self_retrieval 1: after decoding, every
    # image's first caption is scored against all images of its pool (consecutive blocks of retrieval_pool images) -> R@1/5/10,
    # median rank; score_json names a file {"<image id>": ["a caption", ...]} of captions to score under the model (words outside
    # the vocabulary: UNK, or dropped under constraints_oov drop); score_norm: 'none' the joint log-probability, 'length' per token
    self_retrieval=0, retrieval_pool=1000, score_norm='none', score_json='',
    # discriminative decoding (opt['distractors'], imagecaptioning/pytorch_amd/disc.py; not flags of the reference).  disc_lambda in
    # [0, 1] turns it on (below 0, the default: off; 1 is the plain decoder): every image of an eval batch is decoded against
    # disc_distractors (1..7) other images of the batch, picked by disc_pick 'nearest' (cosine similarity of the mean-pooled region
    # features) or 'random' (seeded by seed); disc_mode: 'suppress' | 'listener'
    disc_lambda=-1.0, disc_distractors=1, disc_mode='suppress', disc_pick='nearest',
    # contrastive search (sample_method 'contrastive', decode.contrastive_steps; not flags of the reference): the weight of the
    # degeneration penalty in [0, 1] (0: greedy) and the number of candidates per step, 1..32
    penalty_alpha=0.6, contrastive_k=4,
    # data (synthetic only: the reference's h5/lmdb loaders are outside the hot path)
    input_synthetic=1, vocab_size=9487, synthetic_regions=36, synthetic_images=200,
    # real precomputed features (captioning/data/feature_loader.py; opts.py:23-37 of the reference)
    input_json='', input_label_h5='', input_fc_dir='', input_att_dir='', use_fc=1, norm_att_feat=0, train_only=0, resident_features=1, resident_budget_gb=0.0,
    # the element format of the HBM-resident store's region rows (captioning/data/resident.py): 'fp32', or 'bf16' / 'fp16' -- twice the
    # images in the same budget, rounded once at insertion
    resident_dtype='fp32',
    # opts.py:29-37, 103-106: box geometry appended to every region row (att_feat_size grows by 5: the user sets it, as in the reference)
    use_box=0, norm_box_feat=0, input_box_dir='data/cocotalk_box',
)

RESIDENT_DTYPES = ('fp32', 'bf16', 'fp16')


LIST_ELEMENTS = dict(distill_from=str, distill_weights=float, bad_words=str)      # the list-valued flags: --flag A B ...


def add_flag(ap, k, v):
    """--k with the type of its default v, default None (= not given on the command line)"""
    if k in LIST_ELEMENTS:
        ap.add_argument('--' + k, nargs='*', type=LIST_ELEMENTS[k], default=None)
    else:
        ap.add_argument('--' + k, type=(type(v) if v is not None else str), default=None)


def parse_opt(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', type=str, default=None)
    for k, v in DEFAULTS.items():
        add_flag(ap, k, v)
    ns = ap.parse_args(argv)
    opt = {k: (list(v) if isinstance(v, list) else v) for k, v in DEFAULTS.items()}
    if ns.cfg:
        for k, v in config.load(ns.cfg).items():
            opt[k] = v
    for k in DEFAULTS:
        v = getattr(ns, k)
        if v is not None:
            opt[k] = v
    opt['cfg'] = ns.cfg
    o = argparse.Namespace(**opt)
    if o.resident_dtype not in RESIDENT_DTYPES:
        ap.error("--resident_dtype %r: choose one of 'fp32', 'bf16', 'fp16'" % (o.resident_dtype,))
    if o.max_length is None:
        o.max_length = o.seq_length
    return o
