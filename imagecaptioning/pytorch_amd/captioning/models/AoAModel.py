"""AoAModel (reference captioning/models/AoAModel.py:188-226) on the HIP backend -- BASELINE configs[4]
(configs/aoa.yml switches: refine 1, refine_aoa 1, use_ff 0, decoder_type AoA, use_multi_head 2, mean_feats 1) and the ablation
switches of AoAModel.py:100-226: decoder_type AoA / LSTM / base, out_res, ctx_drop, mean_feats, refine, refine_aoa, use_ff.
Parameter tree = the reference's for every variant; arithmetic = aoa_engine.py + csrc kernels."""
import copy

import torch
import torch.nn as nn

from .CaptionModel import CaptionModel
from .TransformerModel import _FF, _LayerNorm, _Sublayer, _clones
from imagecaptioning.pytorch_amd import aoa_engine as engine
from imagecaptioning.pytorch_amd._lib import CapmiError


FF_HIDDEN = 2048         # PositionwiseFeedForward(rnn_size, 2048, 0.1): constants of the reference (AoAModel.py:119)


class _MHDot(nn.Module):
    """MultiHeadedDotAttention parameter holder (AoAModel.py:17-55)."""

    def __init__(self, d, project_k_v, do_aoa, norm_q, use_output_layer=1):
        super().__init__()
        if norm_q:
            self.norm = _LayerNorm(d)
        self.linears = _clones(nn.Linear(d, d), 1 + 2 * project_k_v)
        if use_output_layer and not do_aoa:         # (AoAModel.py:36,48-51: deleted again when the AoA block follows)
            self.output_layer = nn.Linear(d, d)
        if do_aoa:
            self.aoa_layer = nn.Sequential(nn.Linear(2 * d, 2 * d), nn.GLU())


class _RefLayer(nn.Module):
    def __init__(self, d, refine_aoa, use_ff):
        super().__init__()
        self.self_attn = _MHDot(d, 1, refine_aoa, 0)
        if use_ff:
            self.feed_forward = _FF(d, FF_HIDDEN)
        self.sublayer = _clones(_Sublayer(d), 1 + use_ff)


class _Refiner(nn.Module):
    def __init__(self, d, refine_aoa=1, use_ff=0):
        super().__init__()
        self.layers = _clones(_RefLayer(d, refine_aoa, use_ff), 6)
        self.norm = _LayerNorm(d)


class _Core(nn.Module):
    def __init__(self, opt):
        super().__init__()
        R = opt.rnn_size
        kind = getattr(opt, 'decoder_type', 'AoA')
        self.att_lstm = nn.LSTMCell(opt.input_encoding_size + R, R)
        if kind == 'AoA':
            self.att2ctx = nn.Sequential(nn.Linear(2 * R, 2 * R), nn.GLU())
        elif kind == 'LSTM':
            self.att2ctx = nn.LSTMCell(2 * R, R)
        else:
            self.att2ctx = nn.Sequential(nn.Linear(2 * R, R), nn.ReLU())
        self.attention = _MHDot(R, 0, 0, 1, use_output_layer=0)


class _Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, cfg, fc_feats, att_feats, att_masks, *params):
        P = model._params()
        ctx.sink = cfg.pop('_sink', None)
        ctx.set_materialize_grads(False)        # the dense log-prob gradient may be undefined (sparse route)
        grads = model._grad_targets(P)
        g = engine.AoAGraph(P, grads, model.num_heads, model.drop_prob_lm, model.dropout_aoa, model.training, model._next_seed(),
                            variant=model.variant)
        g.prepare(att_feats, att_masks, fc_feats)
        seq, logp = g.rollout(**cfg)
        ctx.g, ctx.model, ctx.grads = g, model, grads
        ctx.mark_non_differentiable(seq)
        # (an ALIAS of the engine's tensor is returned: autograd hangs this Function on the returned object, and returning the very
        #  tensor the saved engine holds would close a reference cycle ctx -> engine -> tensor -> grad_fn -> ctx -- every activation
        #  of the step then lives until the interpreter's cyclic collector happens to run, not until the step's graph is dropped)
        return seq, logp.detach()

    @staticmethod
    def backward(ctx, _gs, g_logp):
        flat = ctx.model._flat
        stash = flat.begin_backward() if flat is not None else None
        from imagecaptioning.pytorch_amd import sparse_logp
        g_logp, sparse, keep = sparse_logp.split_grad(g_logp, ctx.sink, ctx.g.seq_logp)
        ctx.g._sparse_keep = keep
        ctx.g.backward(g_logp, sparse=sparse)
        if flat is not None:
            flat.end_backward(stash)
            return (None,) * (5 + len(ctx.model._param_names))
        return (None, None, None, None, None) + tuple(ctx.grads[k] for k in ctx.model._param_names)


class AoAModel(CaptionModel):
    _sbs_refusal = None             # sample_method 'sbs': BeamDecoder is a stepper
    _cbs_refusal = None             # opt['constraints']: likewise
    _contrastive_refusal = None     # sample_method 'contrastive': the carried context is the logit operand (out_res 1: refused per model)
    graph_step = True      # graph_step.TrainStep captures this family's training iteration into a hipGraph (no host sync in it)

    def __init__(self, opt):
        super().__init__()
        for k, want in (('use_multi_head', 2), ('multi_head_scale', 1)):
            if getattr(opt, k, want) != want:
                raise NotImplementedError('AoA option %s=%r is outside configs/aoa.yml' % (k, getattr(opt, k)))
        kind = getattr(opt, 'decoder_type', 'AoA')
        # the ablation switches with the reference's own defaults (getattr sites of AoAModel.py:135-137,193; opt.refine, opt.refine_aoa
        # and opt.use_ff are read without one there: configs/aoa.yml's values stand in)
        self.variant = engine.Variant(decoder=kind if kind in ('AoA', 'LSTM') else 'base', out_res=int(bool(getattr(opt, 'out_res', 0))),
                                      ctx_drop=int(bool(getattr(opt, 'ctx_drop', 0))), mean_feats=int(bool(getattr(opt, 'mean_feats', 1))),
                                      refine=int(bool(getattr(opt, 'refine', 1))), refine_aoa=int(bool(getattr(opt, 'refine_aoa', 1))),
                                      use_ff=int(bool(getattr(opt, 'use_ff', 0))))
        v = self.variant
        if v.out_res:
            # logit(output + h_att): the BeamDecoder adds h_att as a second K segment of the logit GEMM, the sum is no kept row
            self._contrastive_refusal = 'out_res 1 forms the logit operand inside the GEMM, the decoder keeps no pre-logit row'
        self.vocab_size = opt.vocab_size
        self.rnn_size = opt.rnn_size
        self.input_encoding_size = opt.input_encoding_size
        self.num_layers = 2
        self.num_heads = opt.num_heads
        self.drop_prob_lm = opt.drop_prob_lm
        self.dropout_aoa = getattr(opt, 'dropout_aoa', 0.3)
        self.seq_length = getattr(opt, 'max_length', 20) or opt.seq_length
        self.vocab = opt.vocab
        R = self.rnn_size
        self.embed = nn.Sequential(nn.Embedding(self.vocab_size + 1, self.input_encoding_size), nn.ReLU(),
                                   nn.Dropout(self.drop_prob_lm))
        if not v.mean_feats:                 # (AoAModel.py:198-199: deleted when the mean of the regions stands in)
            self.fc_embed = nn.Sequential(nn.Linear(opt.fc_feat_size, R), nn.ReLU(), nn.Dropout(self.drop_prob_lm))
        self.att_embed = nn.Sequential(nn.Linear(opt.att_feat_size, R), nn.ReLU(), nn.Dropout(self.drop_prob_lm))
        self.logit = nn.Linear(R, self.vocab_size + 1)
        self.ctx2att = nn.Linear(R, 2 * R)
        if v.refine:
            self.refiner = _Refiner(R, v.refine_aoa, v.use_ff)
        self.core = _Core(opt)

    def _flat_groups(self):
        """Wq | Wk | Wv (and biases) of every refiner layer back to back in the flat buffers: one fused projection GEMM each"""
        names = [n for n, _ in self.named_parameters()]
        blocks = sorted({n[:n.index('.self_attn.') + len('.self_attn')] for n in names if n.startswith('refiner.') and '.self_attn.linears.' in n})
        return [['%s.linears.%d.%s' % (b, i, kind) for i in range(3)] for b in blocks for kind in ('weight', 'bias')]

    _rollout_filters = True         # top<k|p> run inside the rollout's select launch

    def _feeds(self, fc_feats, att_feats, att_masks):
        return att_feats, att_masks, fc_feats

    def _run(self, cfg, att_feats, att_masks, clipped=False, fc_feats=None):
        self._device_check(att_feats)
        if not clipped:
            att_feats, att_masks = self._clip_regions(att_feats, att_masks)
        from imagecaptioning.pytorch_amd import sparse_logp
        cfg = dict(cfg)
        cfg['_sink'] = sink = sparse_logp.LogpSink()
        seq, logp = _Fn.apply(self, cfg, self._fc(fc_feats), att_feats, att_masks, *self._param_list())
        return seq, sparse_logp.attach(logp, sink)

    def _fc(self, fc_feats):
        """the fc features the engine reads (mean_feats 0, AoAModel.py:221), or None"""
        if self.variant.mean_feats:
            return None
        if fc_feats is None:
            raise CapmiError('mean_feats 0 reads fc_feats (AoAModel.py:221): none were given')
        return fc_feats.float().contiguous()

    def _forward(self, fc_feats, att_feats, seq, att_masks=None):
        seq, T_eff = self._labels(seq)
        N, T = seq.shape
        cfg = dict(n=N // att_feats.size(0), T=T_eff, L=T, forced=seq, teacher=True)
        cfg.update(self._scheduled_sampling(T_eff, N, att_feats.device))
        _, logp = self._run(cfg, att_feats, att_masks, fc_feats=fc_feats)
        return logp

    def _decode_stepper(self, fc_feats, att_feats, att_masks, L):
        """make(rows_per_image) -> aoa_engine.BeamDecoder on features refined once, here: every decoder of the factory shares them
        (diverse groups).  Masks clipped to the longest row; L is the caller's decode length (the decoder has none)."""
        self._device_check(att_feats)
        g = engine.AoAGraph(self._params(), {}, self.num_heads, 0.0, 0.0, False, 0, variant=self.variant)
        with torch.no_grad():
            g.prepare(*self._clip_regions(att_feats, att_masks), self._fc(fc_feats))
        return lambda rows: engine.BeamDecoder(g, rows)

    def _rollout(self, fc_feats, att_feats, att_masks, opt, how, raw):
        mode, temperature, top_k, top_p = how
        L = self.seq_length
        cfg = dict(n=int(opt.get('sample_n', 1)), T=L, L=L, mode=mode, temperature=temperature,
                   seed=self._next_seed(), gumbel=opt.get('_gumbel'), top_k=top_k, top_p=top_p)
        if raw:
            cfg['raw'] = True
        if mode == 'greedy' and not self.training and not torch.is_grad_enabled() and opt.get('_graph', True):
            # deterministic, no gradient, launch-bound on the host: replay a captured hipGraph (graphs.py)
            if not hasattr(self, '_graphs'):
                from imagecaptioning.pytorch_amd.graphs import GraphedDecode
                self._graphs = GraphedDecode()
            gcfg = dict(cfg, seed=0)
            feeds = self._clip_regions(att_feats, att_masks)    # the data-dependent clip (a host sync) stays outside the graph
            if not self.variant.mean_feats:
                feeds += (self._fc(fc_feats),)
            return self._graphs(('greedy', cfg['n'], L, raw),
                                lambda a, m, f=None: self._run(gcfg, a, m, clipped=True, fc_feats=f), feeds)
        return self._run(cfg, att_feats, att_masks, fc_feats=fc_feats)
