"""NewFCModel (reference AttModel.py:904-945 over FCModel.LSTMCore 13-42) on the HIP backend -- BASELINE
configs[0] (configs/fc.yml).  Same parameter names as the reference: embed.weight, fc_embed.{weight,bias},
_core.i2h/h2h.{weight,bias}, logit.{weight,bias}."""
import torch.nn as nn

from .RecurrentModel import RecurrentModel
from imagecaptioning.pytorch_amd import newfc_engine as engine
from imagecaptioning.pytorch_amd import ops


class LSTMCore(nn.Module):
    """Parameter holder for FCModel.LSTMCore (FCModel.py:13-23)."""

    def __init__(self, opt):
        super().__init__()
        self.i2h = nn.Linear(opt.input_encoding_size, 5 * opt.rnn_size)
        self.h2h = nn.Linear(opt.rnn_size, 5 * opt.rnn_size)


class NewFCModel(RecurrentModel):
    def __init__(self, opt):
        super().__init__()
        self.vocab_size = opt.vocab_size
        self.input_encoding_size = opt.input_encoding_size
        self.rnn_size = opt.rnn_size
        self.num_layers = 1
        self.drop_prob_lm = opt.drop_prob_lm
        self.seq_length = getattr(opt, 'max_length', 20) or opt.seq_length
        self.fc_feat_size = opt.fc_feat_size
        self.vocab = opt.vocab
        self.fc_embed = nn.Linear(self.fc_feat_size, self.input_encoding_size)
        self.embed = nn.Embedding(self.vocab_size + 1, self.input_encoding_size)
        self._core = LSTMCore(opt)
        self.logit = nn.Linear(self.rnn_size, self.vocab_size + 1)

    def _feeds(self, fc_feats, att_feats, att_masks):
        return (fc_feats,)

    def _rollout_masks(self, B, N, T, att_feats, att_masks, dev):
        return {}                                 # the one dropout site is drawn in _run, behind the seeds of the caller

    def _make_rollout(self, P, cfg, fc_feats):
        return engine.Rollout(P, fc_feats, **cfg), None

    def _run(self, cfg, fc_feats):
        self._device_check(fc_feats)
        N, T = fc_feats.shape[0] * cfg['n'], cfg['T']
        if 'drop_out' in cfg:
            pass                                  # the training beam search replays with the masks of its search
        elif self.training and self.drop_prob_lm > 0:
            cfg['drop_out'] = ops.dropout_mask((T, N, self.rnn_size), self.drop_prob_lm, self._next_seed(), 0,
                                               fc_feats.device)
        return super()._run(cfg, fc_feats)

    def _stepper(self, fc_feats):
        """the image step is taken per stepper"""
        from imagecaptioning.pytorch_amd.step import NewFCStepper
        P = self._params()
        return lambda rows: NewFCStepper(P, fc_feats, rows)

    def _sample_beam(self, fc_feats, att_feats, att_masks=None, opt={}):
        from imagecaptioning.pytorch_amd import beam
        if beam.wants_train_beam(self, opt):
            # train mode with gradients (loss_wrapper.py, train_beam_size > 1): search, finalise on the device, forced replay
            return beam.newfc_beam_train(self, fc_feats, opt)
        # AttModel._sample_beam on the single-step decoder (the image step is taken once per image, AttModel.py:925-927)
        return super()._sample_beam(fc_feats, att_feats, att_masks, opt)
