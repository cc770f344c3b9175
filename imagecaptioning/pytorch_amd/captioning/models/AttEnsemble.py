"""AttEnsemble (reference captioning/models/AttEnsemble.py) on the HIP backend: test-time ensembles of any mix of the five
families (updown, newfc, att2in2, transformer, aoa) that share one vocabulary.

    AttEnsemble(models, weights=None)                                  same constructor, same state_dict keys (models.{i}.*, weights)
    model(fc, att, seq, att_masks)                 -> logprobs [N,T,V1]     teacher forced (AttModel.py:126-164)
    model(fc, att, att_masks, opt=..., mode='sample') -> (seq, seqLogprobs)  every decode option of AttModel._sample / _sample_beam
    model.get_logprobs_state(it, fc, att, p_att, masks, state)             AttEnsemble.py:45-53

Every path ends in capmi_ensemble_logprobs: log( sum_i w_i softmax(logit_i) / sum_i w_i ), one launch over all members' rows.
Teacher forcing runs each member's own one-call forward; decoding is host-stepped on an EnsembleStepper (step.py) over the
members' single-step decoders, through the same drivers the families use for their decode options (beam.beam_search_steps,
decode.sample_steps / diverse_sample_steps), so greedy, sampling, top-k/p, sample_n, beam and diverse beam search, decoding
constraints, suppress_UNK, temperature and length penalty all apply to the mixture as in the reference.

The ensemble is evaluation only (tools/eval_ensemble.py): a forward in train mode or with gradients enabled raises.
"""
import torch
import torch.nn as nn

from .CaptionModel import CaptionModel
from imagecaptioning.pytorch_amd import ops
from imagecaptioning.pytorch_amd._lib import CapmiError


class AttEnsemble(CaptionModel):
    _sbs_refusal = 'it is implemented for the single-model families; decode the members one by one'
    _cbs_refusal = _sbs_refusal
    _contrastive_refusal = 'a mixture has no single hidden state; decode the members one by one'

    def __init__(self, models, weights=None):
        super().__init__()
        models = list(models)
        if not models:
            raise ValueError('AttEnsemble needs at least one model')
        V1 = [m.vocab_size + 1 for m in models]
        if len(set(V1)) != 1:
            raise ValueError('ensemble members must share one vocabulary (vocab_size + 1 = %s)' % V1)
        weights = list(weights) if weights is not None else [1.0] * len(models)        # AttEnsemble.py:25
        ops.ensemble_weights(weights, len(models))                                       # >= 0, positive sum, 1..8 members
        self.models = nn.ModuleList(models)
        self.register_buffer('weights', torch.tensor([float(w) for w in weights]))
        m0 = models[0]
        self.vocab = getattr(m0, 'vocab', None)
        self.vocab_size = m0.vocab_size
        self.seq_length = m0.seq_length
        self.bad_endings_ix = m0.bad_endings_ix
        self.unk_idx = getattr(m0, 'unk_idx', None)
        self.bos_idx = self.eos_idx = self.pad_idx = 0
        self.ss_prob = 0
        self._rng_calls = 0

    # ------------------------------------------------------------------ helpers
    def _eval_only(self):
        if self.training or any(m.training for m in self.models):
            raise RuntimeError('AttEnsemble is evaluation only: call model.eval() first')
        if torch.is_grad_enabled():
            raise RuntimeError('AttEnsemble is evaluation only: run it under torch.no_grad()')

    def _w(self):
        return self.weights.tolist()

    def _stepper_factory(self, fc_feats, att_feats, att_masks):
        """make(rows_per_image) -> EnsembleStepper; every member prepares (and clips its masks) once, the decode length is the
        ensemble's seq_length (tools/eval_ensemble.py sets it to max_length)."""
        from imagecaptioning.pytorch_amd.step import EnsembleStepper
        L = self.seq_length
        makes = [m._decode_stepper(fc_feats, att_feats, att_masks, L) for m in self.models]
        w = self._w()
        return lambda rows: EnsembleStepper([mk(rows) for mk in makes], w)

    # ------------------------------------------------------------------ reference API
    def _forward(self, fc_feats, att_feats, seq, att_masks=None):
        """Teacher-forced mixture log-probs [N,T,V1] (AttModel._forward, AttModel.py:126-164, over get_logprobs_state :45-53):
        each member's own forward, then one launch; from the first all-pad column on (:158-159) the rows stay exactly 0."""
        self._eval_only()
        seq, T_eff = self._labels(seq)
        N, T = seq.shape
        V1 = self.vocab_size + 1
        members = [m._forward(fc_feats, att_feats, seq, att_masks).detach().contiguous() for m in self.models]
        for lp in members:
            if tuple(lp.shape) != (N, T, V1):
                raise CapmiError('ensemble member returned %s log-probs, expected %s' % (tuple(lp.shape), (N, T, V1)))
        out = torch.empty(N, T, V1, dtype=torch.float32, device=members[0].device)
        # one launch over all N*T rows (uniform row stride); the rows from T_eff on are the members' zeros and are zeroed again
        ops.ensemble_logprobs([lp.view(N * T, V1) for lp in members], self._w(), out=out.view(N * T, V1))
        if T_eff < T:
            out[:, T_eff:].zero_()
        return out

    def _sample(self, fc_feats, att_feats, att_masks=None, opt={}):
        """AttModel._sample / _sample_beam (AttModel.py:218-352) on the mixture, host-stepped on an EnsembleStepper."""
        from imagecaptioning.pytorch_amd import beam
        beam.refuse_train_beam(self, opt)           # train_beam_size > 1: named, before the general "evaluation only"
        self._eval_only()
        if not opt.get('output_logsoftmax', 1):
            raise NotImplementedError('output_logsoftmax=0 is only used by margin structure losses; AttEnsemble returns the '
                                      'mixture log-probabilities')
        make = self._stepper_factory(fc_feats, att_feats, att_masks)
        B = fc_feats.size(0) if fc_feats is not None else att_feats.size(0)
        if opt.get('beam_size', 1) > 1 and opt.get('sample_method', 'greedy') in ('greedy', 'beam_search'):
            return beam.beam_search_steps(self, make, B, self.vocab_size + 1, self.seq_length, opt, att_feats.device)
        return self._sample_with_options(make, B, opt)

    def init_hidden(self, batch_size):
        """AttEnsemble.py:28-30: the members' states, packed into one list"""
        return self.pack_state([m.init_hidden(batch_size) for m in self.models])

    def pack_state(self, state):
        self.state_lengths = [len(s) for s in state]
        return sum([list(s) for s in state], [])

    def unpack_state(self, state):
        out = []
        for n in self.state_lengths:
            out.append(state[:n])
            state = state[n:]
        return out

    def _members_with(self, name):
        for m in self.models:
            if not hasattr(m, name):
                raise NotImplementedError('%s of an ensemble needs %s on every member; %s has none (use model(..., mode=\'sample\'))'
                                          % (name, name, type(m).__name__))

    def _prepare_feature(self, *args):
        """AttEnsemble.py:55-56: per-member tuples (fc, att, p_att, masks)"""
        self._members_with('_prepare_feature')
        return tuple(zip(*[m._prepare_feature(*args) for m in self.models]))

    def get_logprobs_state(self, it, fc_feats, att_feats, p_att_feats, att_masks, state, output_logsoftmax=1):
        """AttEnsemble.py:45-53: every member's step (its logits), one capmi_ensemble_logprobs over them.  Features are the
        per-member lists of _prepare_feature (rows already repeated by the caller), state the packed list of init_hidden.
        output_logsoftmax is ignored, as in the reference: the result is always the mixture log-prob."""
        self._members_with('get_logprobs_state')
        states = self.unpack_state(state)
        logits, new_states = [], []
        for i, m in enumerate(self.models):
            lg, st = m.get_logprobs_state(it, fc_feats[i], att_feats[i], p_att_feats[i], att_masks[i], states[i], output_logsoftmax=0)
            logits.append(lg.contiguous())
            new_states.append(st)
        return ops.ensemble_logprobs(logits, self._w()), self.pack_state(new_states)
