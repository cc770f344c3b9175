"""Att2in2Model (reference AttModel.py:854-859 over Att2in2Core 750-790) on the HIP backend -- configs/a2i2*.yml.

An AttModel whose fc_embed is the identity and whose core ignores fc_feats.  Same parameter names as the reference:
embed.0.weight, att_embed.0.{weight,bias}, ctx2att.{weight,bias}, core.{i2h,h2h,a2c}.{weight,bias},
core.attention.{h2att,alpha_net}.{weight,bias}, logit.{weight,bias}.  The modules only hold parameters; the rollouts run in
libcapmi (att2in2_engine), one native call each, BPTT by hand-written kernels behind one autograd.Function."""
import torch
import torch.nn as nn

from .RecurrentModel import RecurrentModel, StepAPI
from .AttModel import Attention
from imagecaptioning.pytorch_amd import att2in2_engine as engine
from imagecaptioning.pytorch_amd import ops


class Att2in2Core(nn.Module):
    """Parameter holder for Att2in2Core (AttModel.py:750-767): a2c, i2h, h2h, attention."""

    def __init__(self, opt):
        super().__init__()
        self.a2c = nn.Linear(opt.rnn_size, 2 * opt.rnn_size)
        self.i2h = nn.Linear(opt.input_encoding_size, 5 * opt.rnn_size)
        self.h2h = nn.Linear(opt.rnn_size, 5 * opt.rnn_size)
        self.dropout = nn.Dropout(opt.drop_prob_lm)
        self.attention = Attention(opt)


class Att2in2Model(StepAPI, RecurrentModel):
    _trace_refusal = None           # return_attention: alpha of the rollouts / steppers
    _use_bn_refusal = None

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
        self._check_supported_opt(opt)
        self.embed = nn.Sequential(nn.Embedding(self.vocab_size + 1, self.input_encoding_size), nn.ReLU(),
                                   nn.Dropout(self.drop_prob_lm))
        self.att_embed = self._att_embed_modules(opt)
        self.logit = nn.Linear(self.rnn_size, self.vocab_size + 1)
        self.ctx2att = nn.Linear(self.rnn_size, self.att_hid_size)
        self.core = Att2in2Core(opt)
        self.vocab = opt.vocab

    @staticmethod
    def fc_embed(x):                  # AttModel.py:858: the identity
        return x

    def _feeds(self, fc_feats, att_feats, att_masks):
        return att_feats, att_masks

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

    def _make_rollout(self, P, cfg, att_feats, att_masks):
        pr = engine.prepare(P, att_feats, att_masks, cfg.pop('drop_att', None), bn=self._region_bn(self.training))
        return engine.Rollout(P, pr, **cfg), None

    def _prepare_feature(self, fc_feats, att_feats, att_masks):
        """AttModel.py:114-124 (eval numerics): (fc_feats unchanged, att', p_att, clipped masks)."""
        pr = engine.prepare(self._params(), att_feats.float().contiguous(), None if att_masks is None else att_masks.float(),
                            bn=self._region_bn(False))
        return fc_feats, pr.att, pr.p_att, pr.att_masks

    def _stepper(self, att_feats, att_masks):
        from imagecaptioning.pytorch_amd.step import Att2in2Stepper
        P = self._params()
        pr = engine.prepare(P, att_feats.float().contiguous(), None if att_masks is None else att_masks.float(),
                            bn=self._region_bn(False))
        return lambda rows: Att2in2Stepper(P, pr, rows)

    def _row_stepper(self, P, pr, fc_feats):
        from imagecaptioning.pytorch_amd.step import Att2in2Stepper
        return Att2in2Stepper(P, pr, 1)             # the state of one layer comes back (Att2in2Core.forward, AttModel.py:789)
