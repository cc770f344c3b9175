"""CaptionModel base: mode dispatch (reference CaptionModel.py:29-33) and the decode-option plumbing every family shares."""
import torch
import torch.nn as nn

from imagecaptioning.pytorch_amd import att_trace, cbs, disc, mbr, sbs
from imagecaptioning.pytorch_amd.ops import clip_len

BAD_ENDINGS = ['a', 'an', 'the', 'in', 'for', 'at', 'of', 'with', 'before', 'after', 'on', 'upon', 'near', 'to', 'is',
               'are', 'am', 'the']       # AttModel.py:27


class CaptionModel(nn.Module):
    def forward(self, *args, **kwargs):
        """``model(..., mode='forward'|'sample')`` -> ``self._forward`` / ``self._sample``."""
        mode = kwargs.pop('mode', 'forward')
        if mode == 'sample':
            return self._sample_entry(*args, **kwargs)
        return getattr(self, '_' + mode)(*args, **kwargs)

    # ---- opt['return_attention'] (imagecaptioning.pytorch_amd.att_trace): the per-word region attention of a sample call
    last_attention = None       # dict of device tensors (att, top, top_w, entropy[, box]) after a sample call with the option on
    _trace_req = None           # att_trace.Request while such a call runs
    _trace_col0 = 0             # leading columns of the trace that are no region (AdaAtt: the sentinel)
    # why a family has no trace (None: it has one)
    _trace_refusal = 'the model keeps no per-step weights over the regions'

    # ---- opt['rerank'] (imagecaptioning.pytorch_amd.mbr): consensus reranking of the sample_n captions of every image
    last_rerank = None          # dict of device tensors (choice, expected, utility, candidates, candidate_logp_sum) after such a call

    # ---- opt['sample_method'] = 'sbs' (imagecaptioning.pytorch_amd.sbs): sample_n distinct captions, drawn without replacement
    last_sbs = None             # dict of device tensors (phi, g, log_w), each [B, sample_n], after such a call
    # why a model has no stochastic beam search (None: it has one -- every family that runs beam.beam_search_steps on a stepper)
    _sbs_refusal = 'the model has no single-step decoder for the beam driver'

    # ---- opt['sample_method'] = 'contrastive' (decode.contrastive_steps): why a model has no contrastive search (None: it has one --
    # every family whose stepper keeps the pre-logit rows of its last step, stepper.hidden)
    _contrastive_refusal = 'its single-step decoder keeps no pre-logit row after a step'

    # ---- opt['constraints'] (imagecaptioning.pytorch_amd.cbs): constrained beam search, captions that must contain given words
    last_cbs = None             # dict of device tensors (state, satisfied, total, score), each [B], after such a call
    _cbs_req = None             # cbs.Request (the checked host tables) while such a call runs
    _cbs_refusal = 'the model has no single-step decoder for the beam driver'

    # ---- mode='score' (imagecaptioning.pytorch_amd.score): log p(caption | image) of GIVEN captions; test-time only, no gradient
    last_score = None           # dict of device tensors (logp, len, tok_logp, perplexity) after such a call

    # ---- opt['distractors'] (imagecaptioning.pytorch_amd.disc): discriminative decoding against other images of the batch
    last_disc = None            # {'distractors' (device int64 [B, D]), 'lambda', 'mode'} after such a call

    def _score(self, fc_feats, att_feats, seqs, att_masks=None, opt=None):
        """``model(fc_feats, att_feats, seqs, att_masks, mode='score', opt={...})``: the joint log-probability of the given captions,
        [B, n] for seqs [B, n, L] / [B * n, L], or S [C, B] for seqs [C, L] with opt['pairing'] = 'cross' (score.score_captions:
        'score_norm', 'score_rows', 'temperature', 'suppress_UNK').  Every family with a single-step decoder; AttEnsemble, train
        mode and output_logsoftmax=0 are refused before any device work."""
        from imagecaptioning.pytorch_amd import logits_proc, score
        logits_proc.refuse_score(opt)
        return score.score_captions(self, fc_feats, att_feats, att_masks, seqs, opt)

    def _sample_entry(self, *args, **kwargs):
        opt = kwargs.get('opt') or (args[3] if len(args) > 3 else None)
        if opt:
            from imagecaptioning.pytorch_amd import decode, logits_proc
            logits_proc.check_options(self, opt)                        # the logits processors: every refusal first
            decode.check_truncation(self, opt)                  # min-p / epsilon / eta / typical sampling: every refusal first
            decode.check_contrastive(self, opt)                 # contrastive search: likewise
        if self.last_disc is not None:
            self.last_disc = None
        if disc.wanted(opt):
            return self._sample_disc(opt, *args[:3], **{k: v for k, v in kwargs.items() if k != 'opt'})
        if self.last_cbs is not None:
            self.last_cbs = None
        if cbs.wanted(opt):
            self._cbs_req = cbs.prepare(self, opt)              # every refusal, before any device work
            try:
                return self._sample_traced(*args, **kwargs)
            finally:
                self._cbs_req = None
        if self.last_rerank is not None:
            self.last_rerank = None
        if self.last_sbs is not None:
            self.last_sbs = None
        if sbs.wanted(opt):
            sbs.check_options(self, opt)                        # every refusal, before any device work
        if not mbr.wanted(opt):
            return self._sample_traced(*args, **kwargs)
        mbr.check_options(self, opt)                        # every refusal, before any device work
        return mbr.apply(self, opt, self._sample_traced(*args, **kwargs))

    def _sample_disc(self, opt, fc_feats, att_feats, att_masks=None):
        """A sample call with opt['distractors'] (disc.py): every refusal first, then the stepper-driven search the options ask for
        -- constrained, stochastic or plain / diverse beam search, else the host-stepped samplers -- on a DiscStepper over the
        family's single-step decoder.  The families' one-call rollouts are not used.  Eval numerics, no gradient."""
        from imagecaptioning.pytorch_amd import beam
        B = (att_feats if torch.is_tensor(att_feats) and att_feats.dim() > 1 else fc_feats).shape[0]
        req = disc.check_options(self, opt, B)                  # cbs.prepare's refusals included, before any device work
        method = opt.get('sample_method', 'greedy')
        if method == 'sbs':
            sbs.check_options(self, opt)
        if mbr.wanted(opt):
            mbr.check_options(self, opt)
        for name in ('last_cbs', 'last_rerank', 'last_sbs', 'last_attention'):
            if getattr(self, name) is not None:
                setattr(self, name, None)
        self._cbs_req = req.cbs
        try:
            with torch.no_grad():
                make = disc.make_stepper(self, req, fc_feats, att_feats, att_masks, self.seq_length)
                if req.cbs is not None:
                    out = self._sample_cbs(make, B, opt)
                elif method == 'sbs':
                    out = self._sample_sbs(make, B, opt)
                elif opt.get('beam_size', 1) > 1 and method in ('greedy', 'beam_search'):
                    out = beam.beam_search_steps(self, make, B, self.vocab_size + 1, self.seq_length, opt, req.device)
                else:
                    out = self._sample_with_options(make, B, opt)
        finally:
            self._cbs_req = None
        self.last_disc = {'distractors': req.distractors_dev, 'lambda': req.lam, 'mode': req.mode}
        return mbr.apply(self, opt, out) if mbr.wanted(opt) else out

    def _sample_traced(self, *args, **kwargs):
        opt = kwargs.get('opt') or (args[3] if len(args) > 3 else None)
        if self.last_attention is not None:
            self.last_attention = None
        if not att_trace.wanted(opt):
            return self._sample(*args, **kwargs)
        if self._trace_refusal is not None:
            att_trace.refuse(self)
        self._trace_req = att_trace.Request(self, args[1] if len(args) > 1 else kwargs['att_feats'], opt)
        try:
            return self._sample(*args, **kwargs)
        finally:
            self._trace_req = None

    # ---- parameters without a walk of the module tree per step.  nn.Module.named_parameters() recurses through named_modules()
    # building prefixed names and a de-duplication set: 0.5 ms for the Transformer's 260 parameters, and every forward asks twice
    # (r4: the GPU idled that long at each step's start).  The walk is cached as (name, owning module's _parameters dict, key), so
    # a Parameter OBJECT that is swapped (m.weight = nn.Parameter(...)) is still found; changes of the module TREE drop the cache
    # when they go through this module's own _apply / load_state_dict / attribute assignment / add_module / register_parameter --
    # surgery on a SUBMODULE after the first forward has to call _invalidate_param_cache().
    def _invalidate_param_cache(self):
        self.__dict__.pop('_pcache', None)

    def _param_slots(self):
        c = self.__dict__.get('_pcache')
        if c is None:
            c = []
            for name, _ in nn.Module.named_parameters(self):
                prefix, _, key = name.rpartition('.')
                c.append((name, self.get_submodule(prefix)._parameters, key))
            self.__dict__['_pcache'] = c
        return c

    def _named_param_list(self):
        """[(name, Parameter)] in named_parameters() order"""
        return [(n, d[k]) for n, d, k in self._param_slots()]

    def _param_list(self):
        return [d[k] for _, d, k in self._param_slots()]

    def _param_name_list(self):
        return [n for n, _, _ in self._param_slots()]

    def _apply(self, fn, *a, **kw):
        self._invalidate_param_cache()
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._invalidate_param_cache()
        return super().load_state_dict(*a, **kw)

    def add_module(self, name, module):
        self._invalidate_param_cache()
        return super().add_module(name, module)

    def register_parameter(self, name, param):
        self._invalidate_param_cache()
        return super().register_parameter(name, param)

    def __setattr__(self, name, value):
        if isinstance(value, (nn.Module, nn.Parameter)):
            self.__dict__.pop('_pcache', None)
        super().__setattr__(name, value)

    # ---- what every family's autograd.Function and trainer ask of the model
    _flat = None            # the FlatParams of flatten_parameters_()
    _rng_calls = 0

    @property
    def _param_names(self):
        return self._param_name_list()

    def _params(self):
        return {k: v.detach() for k, v in self._named_param_list()}

    def flatten_parameters_(self, rule='adam'):
        """Move all parameters into one flat buffer (+ flat grads, the optimizer state of `rule`).  Call after .cuda()."""
        from imagecaptioning.pytorch_amd.flat import FlatParams
        self._flat = FlatParams(self, rule)
        return self._flat

    def _grad_targets(self, P):
        if self._flat is not None:
            return self._flat.grad_views
        return {k: torch.empty_like(v) for k, v in P.items()}

    def _next_seed(self):
        self._rng_calls += 1
        return (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._rng_calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF

    @property
    def bad_endings_ix(self):
        """AttModel.py:96-97 (every family derives from AttModel there); assignable for tests."""
        ix = self.__dict__.get('_bad_endings_ix')
        if ix is None:
            ix = [int(k) for k, v in self.vocab.items() if v in BAD_ENDINGS]
        return ix

    @bad_endings_ix.setter
    def bad_endings_ix(self, ix):
        self.__dict__['_bad_endings_ix'] = [int(i) for i in ix]

    # ---- the one sample dispatch of the single-model families ("Adding a decode option").  A family states what differs:
    #     _feeds(fc_feats, att_feats, att_masks)               the inputs it reads, the one whose device and batch size count first
    #     _rollout_filters                                     its one-call rollout applies top<k|p> itself (else: host-stepped)
    #     _raw_refusal                                         output_logsoftmax=0 outside the plain rollout is refused
    #     _decode_stepper(fc_feats, att_feats, att_masks, L)   the factory of every stepper-driven arm: rows_per_image -> stepper
    #     _sample_beam(fc_feats, att_feats, att_masks, opt)    beam search (default: the stepper-driven one, eval / no_grad only)
    #     _rollout(fc_feats, att_feats, att_masks, opt, how, raw)
    #                                                          its free-running rollout; how = parse_sample_method's tuple
    ss_prob = 0.0
    _rollout_filters = False
    _raw_refusal = True

    def _feeds(self, fc_feats, att_feats, att_masks):
        return fc_feats, att_feats, att_masks

    def _device_check(self, t):
        if not t.is_cuda:
            from imagecaptioning.pytorch_amd._lib import CapmiError
            raise CapmiError('the capmi backend runs on a HIP device only (got a %s tensor); there is no CPU path' % t.device.type)

    def _sample(self, fc_feats, att_feats, att_masks=None, opt={}):
        """AttModel._sample (AttModel.py:258-352): constrained, stochastic or plain beam search and the host-stepped options on the
        family's single-step decoder, else its one-call rollout.  Every decode option is classified here, once."""
        from .utils import parse_sample_method
        from imagecaptioning.pytorch_amd import decode
        method = opt.get('sample_method', 'greedy')
        stochastic = method == 'sbs'
        is_beam = opt.get('beam_size', 1) > 1 and method in ('greedy', 'beam_search')
        how = (None, 1.0, 0, 0.0) if (is_beam or stochastic or decode.contrastive(opt)) else parse_sample_method(method, opt.get('temperature', 1.0))
        stepped = decode.wants_options(opt) or (not self._rollout_filters and bool(how[2] or how[3]))
        raw = not opt.get('output_logsoftmax', 1)
        if raw and self._raw_refusal and (is_beam or stepped):
            # AttModel.py:171-175: the margin structure losses read raw LOGITS (loss_wrapper.py:31-37 samples them with sample_n and no
            # decode-time option); the one-call rollout stores them (r5, CAPMI_SELECT_RAW), beam search and the host-stepped option
            # samplers return log-probabilities -- refuse rather than hand those to a margin loss
            raise NotImplementedError('output_logsoftmax=0 is implemented for the sampled / greedy rollout; beam search and the '
                                      'decode-time options of %s return log-probabilities' % type(self).__name__)
        first = self._feeds(fc_feats, att_feats, att_masks)[0]
        self._device_check(first)
        if self._cbs_req is not None or stochastic or (stepped and not is_beam):
            make = self._decode_stepper(fc_feats, att_feats, att_masks, self.seq_length)
            return (self._sample_cbs if self._cbs_req is not None else self._sample_sbs if stochastic else self._sample_with_options)(
                make, first.size(0), opt)
        if is_beam:
            return self._sample_beam(fc_feats, att_feats, att_masks, opt)
        return self._rollout(fc_feats, att_feats, att_masks, opt, how, raw)

    def _sample_beam(self, fc_feats, att_feats, att_masks=None, opt={}):
        """AttModel._sample_beam (AttModel.py:218-256) on the family's single-step decoder"""
        from imagecaptioning.pytorch_amd import beam
        beam.refuse_train_beam(self, opt)           # train_beam_size > 1: no log-probs without a graph
        first = self._feeds(fc_feats, att_feats, att_masks)[0]
        with torch.no_grad():
            return beam.beam_search_steps(self, self._decode_stepper(fc_feats, att_feats, att_masks, self.seq_length), first.size(0),
                                          self.vocab_size + 1, self.seq_length, opt, first.device)

    def _clip_regions(self, att_feats, att_masks):
        """(att_feats, att_masks) cut to the longest mask row, float32 and contiguous (Transformer, AoA).  The cut reads the device:
        callers keep it outside a captured graph."""
        if att_masks is not None:
            ml = clip_len(att_masks)
            att_feats, att_masks = att_feats[:, :ml], att_masks[:, :ml].float().contiguous()
        return att_feats.float().contiguous(), att_masks

    # ---- the prologue of a teacher-forced _forward (AttModel.py:126-164)
    @staticmethod
    def _labels(seq):
        """seq [B, n, T] / [N, T] -> (int64 [N, T], T_eff).  AttModel.py:158-159: stop at the first all-pad column.  The labels are an
        INPUT, so this is one host decision per batch made before anything is enqueued, not a per-step sync."""
        if seq.ndim == 3:
            seq = seq.reshape(-1, seq.shape[2])
        seq = seq.long().contiguous()
        zero_cols = (seq[:, 1:].sum(0) == 0).nonzero()
        return seq, int(zero_cols[0]) + 1 if zero_cols.numel() else seq.shape[1]

    def _scheduled_sampling(self, T_eff, N, dev):
        """the rollout keywords of scheduled sampling (AttModel.py:145-154), {} when it is off: from step 1 on each row feeds, with
        probability ss_prob, a draw from the model's previous distribution instead of the ground-truth word.  The coin flips are
        made here for all steps at once (they do not depend on the model), the draws happen inside the rollout."""
        if not (self.training and self.ss_prob > 0.0):
            return {}
        coin = self._ss_coin if getattr(self, '_ss_coin', None) is not None else \
            torch.rand(T_eff, N, device=dev) < self.ss_prob            # _ss_coin / _ss_gumbel: test hooks
        cfg = dict(ss_mode=torch.where(coin, 1, 2).to(torch.uint8).contiguous(), seed=self._next_seed())
        if getattr(self, '_ss_gumbel', None) is not None:
            cfg['gumbel'] = self._ss_gumbel
        return cfg

    def _sample_sbs(self, make_stepper, B, opt):
        """sample_method 'sbs' on the family's single-step decoder (beam.stochastic_beam_search_steps).  Eval numerics, no gradient."""
        from imagecaptioning.pytorch_amd import beam
        dev = next(self.parameters()).device
        with torch.no_grad():
            return beam.stochastic_beam_search_steps(self, make_stepper, B, self.vocab_size + 1, self.seq_length, opt, dev)

    def _sample_cbs(self, make_stepper, B, opt):
        """opt['constraints'] on the family's single-step decoder (beam.constrained_beam_search_steps).  Eval numerics, no gradient."""
        from imagecaptioning.pytorch_amd import beam
        dev = next(self.parameters()).device
        with torch.no_grad():
            return beam.constrained_beam_search_steps(self, make_stepper, B, self.vocab_size + 1, self.seq_length, opt, dev)

    def _sample_with_options(self, make_stepper, B, opt):
        """AttModel._sample's option branches that need per-step hooks (AttModel.py:270-271 _diverse_sample,
        :293-330 constraints): host-stepped on the family's single-step decoder.  Eval numerics, no gradient.
        make_stepper(rows_per_image) -> stepper (imagecaptioning.pytorch_amd.step protocol)."""
        from imagecaptioning.pytorch_amd import decode
        dev = next(self.parameters()).device
        if self._trace_req is not None:
            # return_attention: the stepper keeps every step's weights, laid out like a rollout's alpha [L, rows, K]
            make_stepper, made = att_trace.recording(make_stepper, self.seq_length)
        with torch.no_grad():
            if decode.contrastive(opt):
                # one look-ahead step over contrastive_k candidate rows per image and token (check_contrastive ran first)
                return decode.contrastive_steps(self, make_stepper(decode.contrastive_params(opt)[1]), B, self.seq_length, opt, dev)
            if opt.get('group_size', 1) > 1:
                st = make_stepper(int(opt['group_size']))
                out = decode.diverse_sample_steps(self, st, B, self.seq_length, opt, dev, seed=self._next_seed())
            else:
                st = make_stepper(int(opt.get('sample_n', 1)))
                out = decode.sample_steps(self, st, B, self.seq_length, opt, dev, seed=self._next_seed())
            if self._trace_req is not None:
                att_trace.from_steps(self, made[0], out[0])
            return out
