"""Att2in2Model (reference AttModel.py:854-859 over Att2in2Core 750-790) on the HIP backend -- configs/a2i2*.yml.

An AttModel whose fc_embed is the identity and whose core ignores fc_feats.  Same parameter names as the reference:
embed.0.weight, att_embed.0.{weight,bias}, ctx2att.{weight,bias}, core.{i2h,h2h,a2c}.{weight,bias},
core.attention.{h2att,alpha_net}.{weight,bias}, logit.{weight,bias}.  The modules only hold parameters; the rollouts run in
libcapmi (att2in2_engine), one native call each, BPTT by hand-written kernels behind one autograd.Function."""
import torch
import torch.nn as nn

from .CaptionModel import CaptionModel
from .AttModel import Attention
from .utils import parse_sample_method, clip_len
from imagecaptioning.pytorch_amd import att2in2_engine as engine
from imagecaptioning.pytorch_amd import ops
from imagecaptioning.pytorch_amd import sparse_logp
from imagecaptioning.pytorch_amd._lib import CapmiError


class Att2in2Core(nn.Module):
    """Parameter holder for Att2in2Core (AttModel.py:750-767): a2c, i2h, h2h, attention."""

    def __init__(self, opt):
        super().__init__()
        self.a2c = nn.Linear(opt.rnn_size, 2 * opt.rnn_size)
        self.i2h = nn.Linear(opt.input_encoding_size, 5 * opt.rnn_size)
        self.h2h = nn.Linear(opt.rnn_size, 5 * opt.rnn_size)
        self.dropout = nn.Dropout(opt.drop_prob_lm)
        self.attention = Attention(opt)


class _RolloutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, cfg, att_feats, att_masks, *params):
        P = dict(zip(model._param_names, [p.detach() for p in params]))
        ctx.sink = cfg.pop('_sink', None)
        ctx.set_materialize_grads(False)        # the dense log-prob gradient may be undefined (sparse route)
        pr = engine.prepare(P, att_feats, att_masks, cfg.pop('drop_att', None))
        ro = engine.Rollout(P, pr, **cfg)
        seq, logp = ro.run()
        ctx.model, ctx.ro, ctx.P = model, ro, P
        ctx.mark_non_differentiable(seq)
        # (an alias of the engine's tensor: returning the very tensor the saved engine holds would close a reference cycle)
        return seq, logp.detach()

    @staticmethod
    def backward(ctx, _g, g_logp):
        model, ro, P = ctx.model, ctx.ro, ctx.P
        flat = model._flat
        stash = flat.begin_backward() if flat is not None else None
        grads = flat.grad_views if flat is not None else {k: torch.empty_like(v) for k, v in P.items()}
        g_logp, sparse, keep = sparse_logp.split_grad(g_logp, ctx.sink, ro.seq_logp)
        ro._sparse_keep = keep
        ro.backward(g_logp, grads, sparse=sparse)
        if flat is not None:
            flat.end_backward(stash)
            return (None,) * (4 + len(model._param_names))
        return (None, None, None, None) + tuple(grads[k] for k in model._param_names)


class Att2in2Model(CaptionModel):
    def __init__(self, opt):
        super().__init__()
        self.vocab_size = opt.vocab_size
        self.input_encoding_size = opt.input_encoding_size
        self.rnn_size = opt.rnn_size
        self.num_layers = opt.num_layers
        self.drop_prob_lm = opt.drop_prob_lm
        self.seq_length = getattr(opt, 'max_length', 20) or opt.seq_length     # AttModel.py:60
        self.fc_feat_size = opt.fc_feat_size
        self.att_feat_size = opt.att_feat_size
        self.att_hid_size = opt.att_hid_size
        if (getattr(opt, 'bos_idx', 0), getattr(opt, 'eos_idx', 0), getattr(opt, 'pad_idx', 0)) != (0, 0, 0):
            raise NotImplementedError('capmi kernels assume bos=eos=pad=0 (the reference default, AttModel.py:65-67)')
        if getattr(opt, 'use_bn', 0):
            raise NotImplementedError('use_bn is outside the shipped configs')
        if getattr(opt, 'logit_layers', 1) != 1:
            raise NotImplementedError('logit_layers > 1 is broken in the reference itself (AttModel.py:92)')
        self.ss_prob = 0.0
        self.embed = nn.Sequential(nn.Embedding(self.vocab_size + 1, self.input_encoding_size), nn.ReLU(),
                                   nn.Dropout(self.drop_prob_lm))
        self.att_embed = nn.Sequential(nn.Linear(self.att_feat_size, self.rnn_size), nn.ReLU(), nn.Dropout(self.drop_prob_lm))
        self.logit = nn.Linear(self.rnn_size, self.vocab_size + 1)
        self.ctx2att = nn.Linear(self.rnn_size, self.att_hid_size)
        self.core = Att2in2Core(opt)
        self.vocab = opt.vocab
        self._flat = None
        self._rng_calls = 0

    @staticmethod
    def fc_embed(x):                  # AttModel.py:858: the identity
        return x

    @property
    def _param_names(self):
        return self._param_name_list()

    def flatten_parameters_(self):
        from imagecaptioning.pytorch_amd.flat import FlatParams
        self._flat = FlatParams(self)
        return self._flat

    def _device_check(self, t):
        if not t.is_cuda:
            raise CapmiError('the capmi backend runs on a HIP device only (got a %s tensor); there is no CPU path' % t.device.type)

    def init_hidden(self, bsz):
        w = self.logit.weight
        return (w.new_zeros(self.num_layers, bsz, self.rnn_size), w.new_zeros(self.num_layers, bsz, self.rnn_size))

    def _next_seed(self):
        self._rng_calls += 1
        return (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._rng_calls * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF

    def _dropout_masks(self, B, K, N, T, dev):
        """Philox keep-masks of the three dropout sites (att_embed, embed, core output) in one launch; {} in eval mode / p == 0.
        Test hook: `_drop_masks` (dict drop_att [B,K,R] / drop_xt [T,N,E] / drop_out [T,N,R]) replaces them."""
        p = self.drop_prob_lm
        if not self.training or p <= 0:
            return {}
        inj = getattr(self, '_drop_masks', None)
        if inj is not None:
            return {k: v.contiguous() for k, v in inj.items()}
        R, E = self.rnn_size, self.input_encoding_size
        att, xt, out = ops.dropout_masks([((B, K, R), 1 << 40, None, dev), ((T, N, E), 2 << 40, None, dev),
                                          ((T, N, R), 3 << 40, None, dev)], p, self._next_seed())
        return dict(drop_att=att, drop_xt=xt, drop_out=out)

    def _run(self, cfg, att_feats, att_masks):
        self._device_check(att_feats)
        att_feats = att_feats.float().contiguous()
        if att_masks is not None:
            att_masks = att_masks.float().contiguous()
        cfg['_sink'] = sink = sparse_logp.LogpSink()
        seq, logp = _RolloutFn.apply(self, cfg, att_feats, att_masks, *self._param_list())
        return seq, sparse_logp.attach(logp, sink)

    def _params(self):
        return {k: v.detach() for k, v in self._named_param_list()}

    def _prepare_feature(self, fc_feats, att_feats, att_masks):
        """AttModel.py:114-124 (eval numerics): (fc_feats unchanged, att', p_att, clipped masks)."""
        pr = engine.prepare(self._params(), att_feats.float().contiguous(), None if att_masks is None else att_masks.float())
        return fc_feats, pr.att, pr.p_att, pr.att_masks

    def _forward(self, fc_feats, att_feats, seq, att_masks=None):
        """Teacher-forced log-probs [N,T,V1] (AttModel.py:126-164), scheduled sampling included."""
        self._device_check(att_feats)
        B = att_feats.size(0)
        if seq.ndim == 3:
            seq = seq.reshape(-1, seq.shape[2])
        seq = seq.long().contiguous()
        N, T = seq.shape
        zero_cols = (seq[:, 1:].sum(0) == 0).nonzero()          # AttModel.py:158-159: stop at the first all-pad column
        T_eff = int(zero_cols[0]) + 1 if zero_cols.numel() else T
        K = clip_len(att_masks, att_feats.shape[1])
        cfg = dict(n=N // B, T=T_eff, L=T, mode='forced', forced=seq, teacher=True)
        cfg.update(self._dropout_masks(B, K, N, T_eff, att_feats.device))
        if self.training and self.ss_prob > 0.0:
            # AttModel.py:145-154: the coin flips of all steps here, the draws inside the rollout (_ss_coin / _ss_gumbel: test hooks)
            coin = self._ss_coin if getattr(self, '_ss_coin', None) is not None else \
                torch.rand(T_eff, N, device=att_feats.device) < self.ss_prob
            cfg['ss_mode'] = torch.where(coin, 1, 2).to(torch.uint8).contiguous()
            cfg['seed'] = self._next_seed()
            if getattr(self, '_ss_gumbel', None) is not None:
                cfg['gumbel'] = self._ss_gumbel
        _, logp = self._run(cfg, att_feats, att_masks)
        return logp

    def _stepper(self, att_feats, att_masks):
        from imagecaptioning.pytorch_amd.step import Att2in2Stepper
        P = self._params()
        pr = engine.prepare(P, att_feats.float().contiguous(), None if att_masks is None else att_masks.float())
        return lambda rows: Att2in2Stepper(P, pr, rows)

    def _decode_stepper(self, fc_feats, att_feats, att_masks, L):
        """make(rows_per_image) -> Att2in2Stepper (= _stepper).  Used by AttEnsemble; L is the caller's decode length (the stepper
        has none)."""
        self._device_check(att_feats)
        return self._stepper(att_feats, att_masks)

    def _sample(self, fc_feats, att_feats, att_masks=None, opt={}):
        """Greedy / sampling rollout (AttModel.py:258-352); beam search and the decode-time options on the stepper."""
        from imagecaptioning.pytorch_amd import decode, beam
        self._device_check(att_feats)
        beam.refuse_train_beam(self, opt)           # train_beam_size > 1: no log-probs without a graph
        method = opt.get('sample_method', 'greedy')
        raw = not opt.get('output_logsoftmax', 1)
        is_beam = opt.get('beam_size', 1) > 1 and method in ('greedy', 'beam_search')
        mode, temperature, top_k, top_p = (None, 1.0, 0, 0.0) if is_beam else parse_sample_method(method, opt.get('temperature', 1.0))
        if raw and (is_beam or decode.wants_options(opt) or top_k or top_p):
            raise NotImplementedError('output_logsoftmax=0 is implemented for the sampled / greedy rollout; beam search and the '
                                      'decode-time options of %s return log-probabilities' % type(self).__name__)
        B = att_feats.size(0)
        if is_beam:
            with torch.no_grad():
                return beam.beam_search_steps(self, self._stepper(att_feats, att_masks), B, self.vocab_size + 1, self.seq_length,
                                              opt, att_feats.device)
        if decode.wants_options(opt) or top_k or top_p:
            return self._sample_with_options(self._stepper(att_feats, att_masks), B, opt)
        n, L = int(opt.get('sample_n', 1)), self.seq_length
        K = clip_len(att_masks, att_feats.shape[1])
        cfg = dict(n=n, T=L, L=L, mode=mode, temperature=temperature, seed=self._next_seed(), raw=raw)
        cfg.update(self._dropout_masks(B, K, B * n, L, att_feats.device))
        if opt.get('_gumbel') is not None:         # test hook: injected noise [L, N, V1]
            cfg['gumbel'] = opt['_gumbel']
        return self._run(cfg, att_feats, att_masks)

    def get_logprobs_state(self, it, fc_feats, att_feats, p_att_feats, att_masks, state, output_logsoftmax=1):
        """One decoder step on prepared, per-row features (AttModel.py:166-176).  Eval numerics; returns (logprobs, state) with
        the state of one layer (Att2in2Core.forward, AttModel.py:789)."""
        from imagecaptioning.pytorch_amd import _lib
        from imagecaptioning.pytorch_amd.step import Att2in2Stepper
        from imagecaptioning.pytorch_amd.updown_engine import Prepared
        self._device_check(att_feats)
        pr = Prepared()
        pr.att, pr.p_att = att_feats.float().contiguous(), p_att_feats.float().contiguous()
        pr.att_masks = None if att_masks is None else att_masks.float().contiguous()
        N = pr.att.shape[0]
        st = Att2in2Stepper(self._params(), pr, 1)
        st.load_state(state, N)
        logits = st.step(0, it.long().contiguous(), 1)
        new_state = st.export_state(N)
        if not output_logsoftmax:
            return logits.clone(), new_state
        logp = torch.empty_like(logits)
        _lib.check(_lib.lib.capmi_log_softmax_rows(_lib.ptr(logits), _lib.ptr(logp), N, st.V1, _lib.stream_ptr()),
                   'capmi_log_softmax_rows')
        return logp, new_state
