"""AdaAttModel / AdaAttMOModel (reference AttModel.py:843-852 over AdaAttCore 604-613: AdaAtt_lstm 451-537 + AdaAtt_attention
539-602, "Knowing when to look") on the HIP backend -- caption_model adaatt / adaattmo.

A plain AttModel (fc_embed is used) whose one-layer LSTM also emits a visual sentinel and whose attention runs over the K regions
plus that sentinel.  Same parameter names and shapes as the reference, so its checkpoints load unchanged: embed.0.weight,
fc_embed.0, att_embed.0, ctx2att, core.lstm.{w2h,v2h,h2h.0,r_w2h,r_v2h,r_h2h}, core.attention.{fr_linear.0,fr_embed,ho_linear.0,
ho_embed,alpha_net,att2h}, logit.  The modules only hold parameters; the rollouts run in libcapmi (adaatt_engine), one native call
each, BPTT by hand-written kernels behind one autograd.Function."""
import torch
import torch.nn as nn

from .RecurrentModel import RecurrentModel, StepAPI
from imagecaptioning.pytorch_amd import adaatt_engine as engine
from imagecaptioning.pytorch_amd import ops


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


class AdaAttModel(StepAPI, RecurrentModel):
    use_maxout = False
    # return_attention: pi [.., K + 1] of the rollouts / steppers, the visual sentinel in column 0 as AdaAtt_attention puts it
    # (AttModel.py:581-593: cat([fake_region, conv_feat]); with att_masks the sentinel takes the mask of region 0, then renormalised)
    _trace_refusal, _trace_col0 = None, 1

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
        self._check_supported_opt(opt)
        p = self.drop_prob_lm
        self.embed = nn.Sequential(nn.Embedding(self.vocab_size + 1, self.input_encoding_size), nn.ReLU(), nn.Dropout(p))
        self.fc_embed = nn.Sequential(nn.Linear(self.fc_feat_size, self.rnn_size), nn.ReLU(), nn.Dropout(p))
        self.att_embed = nn.Sequential(nn.Linear(self.att_feat_size, self.rnn_size), nn.ReLU(), nn.Dropout(p))
        self.logit = nn.Linear(self.rnn_size, self.vocab_size + 1)
        self.ctx2att = nn.Linear(self.rnn_size, self.att_hid_size)
        self.core = AdaAttCore(opt, self.use_maxout)
        self.vocab = opt.vocab

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

    def _make_rollout(self, P, cfg, fc_feats, att_feats, att_masks):
        ap = engine.prepare(P, fc_feats, att_feats, att_masks, cfg.pop('drop_fc', None), cfg.pop('drop_att', None))
        return engine.Rollout(P, ap, **cfg), None

    def _prepare_feature(self, fc_feats, att_feats, att_masks):
        """AttModel.py:114-124 (eval numerics): (fc', att', p_att, clipped masks)."""
        ap = engine.prepare(self._params(), fc_feats.float().contiguous(), att_feats.float().contiguous(),
                            None if att_masks is None else att_masks.float())
        return ap.fc, ap.att, ap.p_att, ap.att_masks

    def _stepper(self, fc_feats, att_feats, att_masks):
        from imagecaptioning.pytorch_amd.step import AdaAttStepper
        P = self._params()
        ap = engine.prepare(P, fc_feats.float().contiguous(), att_feats.float().contiguous(),
                            None if att_masks is None else att_masks.float())
        return lambda rows: AdaAttStepper(P, ap, rows)

    def _row_stepper(self, P, pr, fc_feats):
        from imagecaptioning.pytorch_amd.step import AdaAttStepper
        pr.fc = fc_feats.float().contiguous()
        return AdaAttStepper(P, engine.from_features(P, pr), 1)


class AdaAttMOModel(AdaAttModel):
    use_maxout = True
