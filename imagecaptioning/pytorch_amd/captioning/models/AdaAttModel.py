"""AdaAttModel / AdaAttMOModel (reference AttModel.py:843-852 over AdaAttCore 604-613: AdaAtt_lstm 451-537 + AdaAtt_attention
539-602, "Knowing when to look") on the HIP backend -- caption_model adaatt / adaattmo.

A plain AttModel (fc_embed is used) whose one-layer LSTM also emits a visual sentinel and whose attention runs over the K regions
plus that sentinel.  Same parameter names and shapes as the reference, so its checkpoints load unchanged: embed.0.weight,
fc_embed.0, att_embed.0, ctx2att, core.lstm.{w2h,v2h,h2h.0,r_w2h,r_v2h,r_h2h}, core.attention.{fr_linear.0,fr_embed,ho_linear.0,
ho_embed,alpha_net,att2h}, logit.  The modules only hold parameters; the rollouts run in libcapmi (adaatt_engine), one native call
each, BPTT by hand-written kernels behind one autograd.Function."""
import torch
import torch.nn as nn

from .CaptionModel import CaptionModel
from .utils import parse_sample_method, clip_len
from imagecaptioning.pytorch_amd import adaatt_engine as engine
from imagecaptioning.pytorch_amd import ops
from imagecaptioning.pytorch_amd import sparse_logp
from imagecaptioning.pytorch_amd._lib import CapmiError


class AdaAtt_lstm(nn.Module):
    """Parameter holder for AdaAtt_lstm (AttModel.py:451-478), one layer."""

    def __init__(self, opt, use_maxout):
        super().__init__()
        G = (4 + int(bool(use_maxout))) * opt.rnn_size
        self.use_maxout = use_maxout
        self.w2h = nn.Linear(opt.input_encoding_size, G)
        self.v2h = nn.Linear(opt.rnn_size, G)
        self.i2h = nn.ModuleList()                          # layers above the first: none (num_layers == 1)
        self.h2h = nn.ModuleList([nn.Linear(opt.rnn_size, G)])
        self.r_w2h = nn.Linear(opt.input_encoding_size, opt.rnn_size)
        self.r_v2h = nn.Linear(opt.rnn_size, opt.rnn_size)
        self.r_h2h = nn.Linear(opt.rnn_size, opt.rnn_size)


class AdaAtt_attention(nn.Module):
    """Parameter holder for AdaAtt_attention (AttModel.py:539-563)."""

    def __init__(self, opt):
        super().__init__()
        p = opt.drop_prob_lm
        self.fr_linear = nn.Sequential(nn.Linear(opt.rnn_size, opt.input_encoding_size), nn.ReLU(), nn.Dropout(p))
        self.fr_embed = nn.Linear(opt.input_encoding_size, opt.att_hid_size)
        self.ho_linear = nn.Sequential(nn.Linear(opt.rnn_size, opt.input_encoding_size), nn.Tanh(), nn.Dropout(p))
        self.ho_embed = nn.Linear(opt.input_encoding_size, opt.att_hid_size)
        self.alpha_net = nn.Linear(opt.att_hid_size, 1)
        self.att2h = nn.Linear(opt.rnn_size, opt.rnn_size)


class AdaAttCore(nn.Module):
    def __init__(self, opt, use_maxout=False):
        super().__init__()
        self.lstm = AdaAtt_lstm(opt, use_maxout)
        self.attention = AdaAtt_attention(opt)


class _RolloutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, cfg, fc_feats, att_feats, att_masks, *params):
        P = dict(zip(model._param_names, [p.detach() for p in params]))
        ctx.sink = cfg.pop('_sink', None)
        ctx.set_materialize_grads(False)        # the dense log-prob gradient may be undefined (sparse route)
        ap = engine.prepare(P, fc_feats, att_feats, att_masks, cfg.pop('drop_fc', None), cfg.pop('drop_att', None))
        ro = engine.Rollout(P, ap, **cfg)
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
            return (None,) * (5 + len(model._param_names))
        return (None,) * 5 + tuple(grads[k] for k in model._param_names)


class AdaAttModel(CaptionModel):
    use_maxout = False

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
        if not (self.input_encoding_size == self.rnn_size == self.att_hid_size):
            raise NotImplementedError('AdaAtt_attention views its operands across the three widths (AttModel.py:569-582): it needs '
                                      'input_encoding_size == rnn_size == att_hid_size, got %d, %d, %d' %
                                      (self.input_encoding_size, self.rnn_size, self.att_hid_size))
        if self.num_layers != 1:
            raise NotImplementedError('AdaAtt with num_layers = %d: one layer is implemented' % self.num_layers)
        if (getattr(opt, 'bos_idx', 0), getattr(opt, 'eos_idx', 0), getattr(opt, 'pad_idx', 0)) != (0, 0, 0):
            raise NotImplementedError('capmi kernels assume bos=eos=pad=0 (the reference default, AttModel.py:65-67)')
        if getattr(opt, 'use_bn', 0):
            raise NotImplementedError('use_bn is outside the shipped configs')
        if getattr(opt, 'logit_layers', 1) != 1:
            raise NotImplementedError('logit_layers > 1 is broken in the reference itself (AttModel.py:92)')
        self.ss_prob = 0.0
        p = self.drop_prob_lm
        self.embed = nn.Sequential(nn.Embedding(self.vocab_size + 1, self.input_encoding_size), nn.ReLU(), nn.Dropout(p))
        self.fc_embed = nn.Sequential(nn.Linear(self.fc_feat_size, self.rnn_size), nn.ReLU(), nn.Dropout(p))
        self.att_embed = nn.Sequential(nn.Linear(self.att_feat_size, self.rnn_size), nn.ReLU(), nn.Dropout(p))
        self.logit = nn.Linear(self.rnn_size, self.vocab_size + 1)
        self.ctx2att = nn.Linear(self.rnn_size, self.att_hid_size)
        self.core = AdaAttCore(opt, self.use_maxout)
        self.vocab = opt.vocab
        self._flat = None
        self._rng_calls = 0

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
        """The dropout sites of one rollout; {} in eval mode / p == 0.  fc_embed, att_embed and per step embed, h, sentinel, fr, ho and
        the core output get Philox keep-masks (two launches); the [N,K+1,A] tanh tile of every step is drawn inside the attention
        kernels (tile_p, tile_seed).  Test hook: `_drop_masks` (dict drop_fc [B,R] / drop_att [B,K,R] / drop_xt [T,N,E] / drop_h /
        drop_fake / drop_out [T,N,R] / drop_fr / drop_ho [T,N,E] / drop_tile [T,N,K+1,A]) replaces them."""
        p = self.drop_prob_lm
        if not self.training or p <= 0:
            return {}
        inj = getattr(self, '_drop_masks', None)
        if inj is not None:
            return {k: v.contiguous() for k, v in inj.items()}
        R, E = self.rnn_size, self.input_encoding_size
        seed = self._next_seed()
        names = ('drop_fc', 'drop_att', 'drop_xt', 'drop_h', 'drop_fake', 'drop_fr', 'drop_ho', 'drop_out')
        shapes = ((B, R), (B, K, R), (T, N, E), (T, N, R), (T, N, R), (T, N, E), (T, N, E), (T, N, R))
        specs = [(s, (i + 1) << 40, None, dev) for i, s in enumerate(shapes)]
        masks = list(ops.dropout_masks(specs[:4], p, seed)) + list(ops.dropout_masks(specs[4:], p, seed))
        out = dict(zip(names, masks))
        out.update(tile_p=p, tile_seed=self._next_seed())
        return out

    def _run(self, cfg, fc_feats, att_feats, att_masks):
        self._device_check(att_feats)
        fc_feats, att_feats = fc_feats.float().contiguous(), att_feats.float().contiguous()
        if att_masks is not None:
            att_masks = att_masks.float().contiguous()
        cfg['_sink'] = sink = sparse_logp.LogpSink()
        seq, logp = _RolloutFn.apply(self, cfg, fc_feats, att_feats, att_masks, *self._param_list())
        return seq, sparse_logp.attach(logp, sink)

    def _params(self):
        return {k: v.detach() for k, v in self._named_param_list()}

    def _prepare_feature(self, fc_feats, att_feats, att_masks):
        """AttModel.py:114-124 (eval numerics): (fc', att', p_att, clipped masks)."""
        ap = engine.prepare(self._params(), fc_feats.float().contiguous(), att_feats.float().contiguous(),
                            None if att_masks is None else att_masks.float())
        return ap.fc, ap.att, ap.p_att, ap.att_masks

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
        _, logp = self._run(cfg, fc_feats, att_feats, att_masks)
        return logp

    def _stepper(self, fc_feats, att_feats, att_masks):
        from imagecaptioning.pytorch_amd.step import AdaAttStepper
        P = self._params()
        ap = engine.prepare(P, fc_feats.float().contiguous(), att_feats.float().contiguous(),
                            None if att_masks is None else att_masks.float())
        return lambda rows: AdaAttStepper(P, ap, rows)

    def _decode_stepper(self, fc_feats, att_feats, att_masks, L):
        """make(rows_per_image) -> AdaAttStepper (= _stepper).  Used by AttEnsemble; L is the caller's decode length (the stepper
        has none)."""
        self._device_check(att_feats)
        return self._stepper(fc_feats, att_feats, att_masks)

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
                return beam.beam_search_steps(self, self._stepper(fc_feats, att_feats, att_masks), B, self.vocab_size + 1,
                                              self.seq_length, opt, att_feats.device)
        if decode.wants_options(opt) or top_k or top_p:
            return self._sample_with_options(self._stepper(fc_feats, att_feats, att_masks), B, opt)
        n, L = int(opt.get('sample_n', 1)), self.seq_length
        K = clip_len(att_masks, att_feats.shape[1])
        cfg = dict(n=n, T=L, L=L, mode=mode, temperature=temperature, seed=self._next_seed(), raw=raw)
        cfg.update(self._dropout_masks(B, K, B * n, L, att_feats.device))
        if opt.get('_gumbel') is not None:         # test hook: injected noise [L, N, V1]
            cfg['gumbel'] = opt['_gumbel']
        return self._run(cfg, fc_feats, att_feats, att_masks)

    def get_logprobs_state(self, it, fc_feats, att_feats, p_att_feats, att_masks, state, output_logsoftmax=1):
        """One decoder step on prepared, per-row features (AttModel.py:166-176).  Eval numerics; returns (logprobs, state) with
        the state of the one layer."""
        from imagecaptioning.pytorch_amd import _lib
        from imagecaptioning.pytorch_amd.step import AdaAttStepper
        from imagecaptioning.pytorch_amd.updown_engine import Prepared
        self._device_check(att_feats)
        pr = Prepared()
        pr.fc, pr.att, pr.p_att = fc_feats.float().contiguous(), att_feats.float().contiguous(), p_att_feats.float().contiguous()
        pr.att_masks = None if att_masks is None else att_masks.float().contiguous()
        pr.K = pr.att.shape[1]
        N = pr.att.shape[0]
        P = self._params()
        st = AdaAttStepper(P, engine.from_features(P, pr), 1)
        st.load_state(state, N)
        logits = st.step(0, it.long().contiguous(), 1)
        new_state = st.export_state(N)
        if not output_logsoftmax:
            return logits.clone(), new_state
        logp = torch.empty_like(logits)
        _lib.check(_lib.lib.capmi_log_softmax_rows(_lib.ptr(logits), _lib.ptr(logp), N, st.V1, _lib.stream_ptr()),
                   'capmi_log_softmax_rows')
        return logp, new_state


class AdaAttMOModel(AdaAttModel):
    use_maxout = True
