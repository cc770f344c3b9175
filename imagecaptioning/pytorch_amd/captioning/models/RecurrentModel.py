"""RecurrentModel: the host side the LSTM families (UpDown, NewFC, Att2in2, AdaAtt) share -- one autograd.Function around a
family's one-call rollout, the teacher-forced _forward and the free-running _rollout of CaptionModel._sample -- and StepAPI, the
reference's single-step API (init_hidden, get_logprobs_state) for the attention families: NewFC has neither, and callers probe for
them with hasattr.

A family holds its parameters (nn.Module tree with the reference's names) and states, by overriding:

    _feeds(fc_feats, att_feats, att_masks)    which of the three its rollout reads, as a tuple (CaptionModel's default: all)
    _make_rollout(P, cfg, *feeds)             cfg -> (engine Rollout, whatever its _rollout_backward wants back)
    _dropout_masks(B, K, N, T, dev)           the keep masks of its dropout sites as Rollout keywords ({} in eval mode)
    _rollout_masks(B, N, T, att_feats, att_masks, dev)
                                              only a family without region features (NewFC): the default derives K from them
                                              and calls _dropout_masks
    _stepper(*feeds)                          rows_per_image -> single-step decoder on features prepared once
    _row_stepper(P, pr, fc_feats)             the same for one row per already embedded feature (StepAPI.get_logprobs_state)

and, where it differs, _rollout_backward / _publish_rollout and the hooks of the sample dispatch: _rollout_filters, _raw_refusal,
_sample_beam, _rollout ("Adding a recurrent family").
"""
import torch

from .CaptionModel import CaptionModel
from .utils import clip_len
from imagecaptioning.pytorch_amd import _lib, sparse_logp
from imagecaptioning.pytorch_amd.engine_common import Prepared, RegionBN


class _RolloutFn(torch.autograd.Function):
    """(feeds..., params...) -> (seq, dense seqLogprobs); backward = hand-written BPTT + prefill backward.
    Gradients are written into the model's flat gradient views when it has them."""

    @staticmethod
    def forward(ctx, model, cfg, *args):
        names = model._param_names
        k = len(args) - len(names)                                  # the family's feeds come first
        P = dict(zip(names, [p.detach() for p in args[k:]]))
        ctx.sink = cfg.pop('_sink', None)
        ctx.set_materialize_grads(False)        # the dense log-prob gradient may be undefined (sparse route)
        ro, ctx.kept = model._make_rollout(P, cfg, *args[:k])
        seq, logp = ro.run()
        ctx.model, ctx.ro, ctx.P, ctx.lead = model, ro, P, 2 + k
        model._publish_rollout(ro, ctx.sink)
        if model._trace_req is not None:            # return_attention: the trace is read off the rollout's own weight buffer
            from imagecaptioning.pytorch_amd import att_trace
            att_trace.from_rollout(model, ro)
        ctx.mark_non_differentiable(seq)
        # (an ALIAS of the engine's tensor is returned: autograd hangs this Function on the returned object, and returning the very
        #  tensor the saved engine holds would close a reference cycle ctx -> engine -> tensor -> grad_fn -> ctx -- every activation
        #  of the step then lives until the interpreter's cyclic collector happens to run, not until the step's graph is dropped)
        return seq, logp.detach()

    @staticmethod
    def backward(ctx, _g_seq, g_logp):
        model, ro, P = ctx.model, ctx.ro, ctx.P
        flat = model._flat
        stash = flat.begin_backward() if flat is not None else None
        grads = model._grad_targets(P)
        g_logp, sparse, keep = sparse_logp.split_grad(g_logp, ctx.sink, ro.seq_logp)       # the criteria hand their gradient over sparse
        ro._sparse_keep = keep
        model._rollout_backward(ro, ctx.kept, P, g_logp, grads, sparse, flat, stash)
        if flat is not None:
            flat.end_backward(stash)
            return (None,) * (ctx.lead + len(P))
        return (None,) * ctx.lead + tuple(grads[k] for k in model._param_names)


class RecurrentModel(CaptionModel):
    _sbs_refusal = None             # sample_method 'sbs': every family here has a stepper
    _cbs_refusal = None             # opt['constraints']: likewise
    _contrastive_refusal = None     # sample_method 'contrastive': every stepper here keeps its pre-logit rows (stepper.hidden)
    ss_prob = 0.0

    # why a family refuses use_bn (None: it runs it).  models.setup gives the same reasons for the families outside this base.
    _use_bn_refusal = 'its prefill has no BatchNorm path (UpDown and Att2in2 have)'

    def _check_supported_opt(self, opt):
        if (getattr(opt, 'bos_idx', 0), getattr(opt, 'eos_idx', 0), getattr(opt, 'pad_idx', 0)) != (0, 0, 0):
            raise NotImplementedError('capmi kernels assume bos=eos=pad=0 (the reference default, AttModel.py:65-67)')
        if getattr(opt, 'use_bn', 0):
            if self._use_bn_refusal is not None:
                raise NotImplementedError('use_bn is not supported for %s: %s' % (type(self).__name__, self._use_bn_refusal))
            if opt.use_bn not in (1, 2):
                raise NotImplementedError('use_bn is 0, 1 or 2 (AttModel.py:80-85), got %r' % (opt.use_bn,))
        if getattr(opt, 'logit_layers', 1) != 1:
            raise NotImplementedError('logit_layers > 1 is broken in the reference itself (AttModel.py:92)')

    use_bn = 0              # UpDown / Att2in2 set it from opt; the other families refuse it (models.setup)

    def _att_embed_modules(self, opt):
        """att_embed of AttModel.py:80-85: (BatchNorm1d(att_feat_size),) Linear, ReLU, Dropout (, BatchNorm1d(rnn_size))"""
        import torch.nn as nn
        self.use_bn = int(getattr(opt, 'use_bn', 0) or 0)
        return nn.Sequential(*(((nn.BatchNorm1d(opt.att_feat_size),) if self.use_bn else ()) +
                               (nn.Linear(opt.att_feat_size, opt.rnn_size), nn.ReLU(), nn.Dropout(opt.drop_prob_lm)) +
                               ((nn.BatchNorm1d(opt.rnn_size),) if self.use_bn == 2 else ())))

    def _region_bn(self, train):
        """the BatchNorm state of one prefill (None without use_bn).  train: batch statistics and ONE update of the running buffers;
        steppers, _prepare_feature, beam search, get_logprobs_state and ensemble members are eval-mode prefills."""
        return RegionBN.of_module(self.att_embed, self.use_bn, train) if self.use_bn else None

    # ------------------------------------------------------------------ the family's hooks
    def _dropout_masks(self, B, K, N, T, dev):
        return {}

    def _rollout_masks(self, B, N, T, att_feats, att_masks, dev):
        self._device_check(att_feats)             # the masks are the first launches of a rollout
        return self._dropout_masks(B, clip_len(att_masks, att_feats.shape[1]), N, T, dev)

    def _rollout_backward(self, ro, kept, P, g_logp, grads, sparse, flat, stash):
        ro.backward(g_logp, grads, sparse=sparse)

    def _publish_rollout(self, ro, sink):
        pass

    # ------------------------------------------------------------------ rollouts
    def _run(self, cfg, *feeds):
        """one rollout of the family's feeds (in _feeds order) -> (seq, seqLogprobs attached to the autograd graph)"""
        self._device_check(feeds[0])
        feeds = [None if t is None else t.float().contiguous() for t in feeds]
        cfg['_sink'] = sink = sparse_logp.LogpSink()
        seq, logp = _RolloutFn.apply(self, cfg, *feeds, *self._param_list())
        return seq, sparse_logp.attach(logp, sink)

    def _forward(self, fc_feats, att_feats, seq, att_masks=None):
        """Teacher-forced log-probs [N,T,V1] (AttModel.py:126-164), scheduled sampling included."""
        feeds = self._feeds(fc_feats, att_feats, att_masks)
        B, dev = feeds[0].size(0), feeds[0].device
        seq, T_eff = self._labels(seq)
        N, T = seq.shape
        cfg = dict(n=N // B, T=T_eff, L=T, mode='forced', forced=seq, teacher=True)
        cfg.update(self._rollout_masks(B, N, T_eff, att_feats, att_masks, dev))
        cfg.update(self._scheduled_sampling(T_eff, N, dev))
        _, logp = self._run(cfg, *feeds)
        return logp

    def _rollout(self, fc_feats, att_feats, att_masks, opt, how, raw, **more):
        """Greedy / sampling rollout (AttModel.py:258-352).  more: what a family adds to the rollout's keywords."""
        feeds = self._feeds(fc_feats, att_feats, att_masks)
        B, n, L = feeds[0].size(0), int(opt.get('sample_n', 1)), self.seq_length
        cfg = dict(n=n, T=L, L=L, mode=how[0], temperature=how[1], seed=self._next_seed(), raw=raw)
        cfg.update(self._rollout_masks(B, B * n, L, att_feats, att_masks, feeds[0].device))
        cfg.update(more)
        if opt.get('_gumbel') is not None:         # test hook: injected noise [L, N, V1]
            cfg['gumbel'] = opt['_gumbel']
        return self._run(cfg, *feeds)

    # ------------------------------------------------------------------ single steps
    def _decode_stepper(self, fc_feats, att_feats, att_masks, L):
        """make(rows_per_image) -> the family's stepper (= _stepper); L is the caller's decode length (the stepper has none)"""
        feeds = self._feeds(fc_feats, att_feats, att_masks)
        self._device_check(feeds[0])
        return self._stepper(*feeds)


class StepAPI:
    """init_hidden / get_logprobs_state (AttModel.py:166-176) of UpDown, Att2in2 and AdaAtt, mixed in before RecurrentModel"""

    def init_hidden(self, bsz):
        w = self.logit.weight
        return (w.new_zeros(self.num_layers, bsz, self.rnn_size), w.new_zeros(self.num_layers, bsz, self.rnn_size))

    def get_logprobs_state(self, it, fc_feats, att_feats, p_att_feats, att_masks, state, output_logsoftmax=1):
        """One decoder step on prepared features (AttModel.py:166-176) for callers that drive the decoder themselves (ensembles,
        custom searches): features are per ROW (already repeated by the caller, as in the reference), state is the reference's
        (h [layers,N,R], c [layers,N,R]).  Eval numerics; returns (logprobs [N,V1], new state)."""
        self._device_check(att_feats)
        pr = Prepared.of_features(att_feats, p_att_feats, att_masks)
        N = pr.att.shape[0]
        st = self._row_stepper(self._params(), pr, fc_feats)
        st.load_state(state, N)
        logits = st.step(0, it.long().contiguous(), 1)
        new_state = st.export_state(N)
        if not output_logsoftmax:
            return logits.clone(), new_state
        logp = torch.empty_like(logits)
        _lib.check(_lib.lib.capmi_log_softmax_rows(_lib.ptr(logits), _lib.ptr(logp), N, st.V1, _lib.stream_ptr()),
                   'capmi_log_softmax_rows')
        return logp, new_state
