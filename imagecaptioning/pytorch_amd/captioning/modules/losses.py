"""Criteria of the hot path (reference captioning/modules/losses.py).  They consume the dense
log-prob tensor the model API returns; the arithmetic is a gather + masked mean over [N,L] values
(K14/K15 of SURVEY.md 2.3) -- device tensor ops on the same HIP stream, no host sync.  The gather goes
through ``sparse_logp.select_logp``: when the tensor comes from a capmi rollout its gradient travels back
as [N,L] values + token ids (``capmi_logsoftmax_bwd_sparse``), never as a dense [N,L,V1] tensor."""
import logging
import math

import torch
import torch.nn as nn

from ..utils.rewards import get_scores, get_self_cider_scores
from imagecaptioning.pytorch_amd.ciderd import nsc_advantage
from imagecaptioning.pytorch_amd.sparse_logp import select_logp, sum_logp, fused_reward_criterion, fused_xe_criterion


def _shifted_mask(seq, like):
    """position 0 on, then (seq>0) shifted right: the EOS step still counts (losses.py:28-29)."""
    m = (seq > 0).to(like)
    return torch.cat([m.new_ones(m.size(0), 1), m[:, :-1]], 1)


class RewardCriterion(nn.Module):
    """losses.py:18-37."""

    def forward(self, input, seq, reward, reduction='mean'):
        # straight from the rollout's saved selected log-probs when `input` / `seq` are its untouched outputs: one launch
        fused = fused_reward_criterion(input, seq, reward, per_row=(reduction == 'none'))
        if fused is not None:
            return fused
        sel = select_logp(input, seq)
        mask = _shifted_mask(seq, sel)
        out = -sel * reward.to(sel) * mask
        if reduction == 'none':
            return out.sum(1) / mask.sum(1)
        return out.sum() / mask.sum()


class LanguageModelCriterion(nn.Module):
    """losses.py:204-224."""

    def forward(self, input, target, mask, reduction='mean'):
        if target.ndim == 3:
            target = target.reshape(-1, target.shape[2])
            mask = mask.reshape(-1, mask.shape[2])
        # device float32 log-probs: capmi_xe_loss_fwd / _bwd read the uncut labels and masks through their row pitch
        fused = fused_xe_criterion(input, target, mask, 0.0, per_row=(reduction == 'none'))
        if fused is not None:
            return fused
        T = input.size(1)
        target = target[:, :T]
        mask = mask[:, :T].to(input)
        out = -select_logp(input, target) * mask
        if reduction == 'none':
            return out.sum(1) / mask.sum(1)
        return out.sum() / mask.sum()


class LabelSmoothing(nn.Module):
    """losses.py:227-265: KL(true_dist || p), off-target mass smoothing/(V1-1)."""

    def __init__(self, size=0, padding_idx=0, smoothing=0.0):
        super().__init__()
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing

    def forward(self, input, target, mask, reduction='mean'):
        if target.ndim == 3:
            target = target.reshape(-1, target.shape[2])
            mask = mask.reshape(-1, mask.shape[2])
        if 0.0 < self.smoothing < 1.0:
            # device float32 log-probs: every dense row is read once by capmi_xe_loss_fwd, nothing dense goes through ATen
            fused = fused_xe_criterion(input, target, mask, self.smoothing, per_row=(reduction == 'none'))
            if fused is not None:
                return fused
        N, T, V1 = input.shape
        tgt2 = target[:, :T]
        target = tgt2.reshape(-1)
        mask = mask[:, :T].reshape(-1).to(input)
        off = self.smoothing / (V1 - 1)
        # sum_v q log q is a constant of (smoothing, V1); -sum_v q logp = -off*sum(lp) - (conf-off)*lp[target]
        ent = (V1 - 1) * (off * math.log(off) if off > 0 else 0.0) + \
              (self.confidence * math.log(self.confidence) if self.confidence > 0 else 0.0)
        cross = off * sum_logp(input).reshape(-1) + (self.confidence - off) * select_logp(input, tgt2.contiguous()).reshape(-1)
        out = (ent - cross) * mask
        if reduction == 'none':
            return out.view(N, T).sum(1) / mask.view(N, T).sum(1)
        return out.sum() / mask.sum()


class StructureLosses(nn.Module):
    """losses.py:40-202.  The ``structure_loss_type``s whose input is log-probabilities -- 'new_self_critical' (168-187, the one
    the *_nsc BASELINE configs use), 'seqnll' (81-88), 'risk' (89-103), 'softmax_margin' (147-155), 'best_of_n' (189-199) -- and, r4,
    the margin types that take RAW LOGITS -- 'max_margin' (105-114), 'multi_margin' (128-137), 'real_softmax_margin' (157-166):
    sampled with output_logsoftmax=0 (loss_wrapper.py:31-37), served by rollouts that store the logits (capmi.h CAPMI_SELECT_RAW).
    The optional ``entropy_reward_weight`` (66-69) is supported.  All of them only read the entries of the sampled tokens, so the
    gradient stays sparse (``select_logp``).  ``self_cider_reward_weight`` (175-182) is read by 'new_self_critical' alone, as in the
    reference: the self-CIDEr of the image's n samples times the weight joins each of its n rows after the leave-one-out baseline
    has been subtracted; with any other type it raises.  ``out['reward']`` is the mixed CIDEr-D / BLEU-4 score before either."""

    LOGPROB_TYPES = ('new_self_critical', 'seqnll', 'risk', 'softmax_margin', 'best_of_n')
    LOGIT_TYPES = ('max_margin', 'multi_margin', 'real_softmax_margin')

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.loss_type = opt.structure_loss_type

    def forward(self, input, seq, data_gts, reduction='mean'):
        if self.loss_type not in self.LOGPROB_TYPES + self.LOGIT_TYPES:
            raise NotImplementedError('structure_loss_type %r: implemented are %s'
                                      % (self.loss_type, ', '.join(self.LOGPROB_TYPES + self.LOGIT_TYPES)))
        sw = getattr(self.opt, 'self_cider_reward_weight', 0)
        if sw > 0 and self.loss_type != 'new_self_critical':
            raise NotImplementedError('self_cider_reward_weight is read by structure_loss_type new_self_critical alone '
                                      '(losses.py:175-182), not by %r' % self.loss_type)
        out = {}
        N = input.size(0)
        n = N // len(data_gts)
        assert n == self.opt.train_sample_n, n
        ew = getattr(self.opt, 'entropy_reward_weight', 0)
        ent = None
        if ew > 0:                      # mean per-token entropy of each sampled sequence, no gradient (:66-69); needs the dense rows
            with torch.no_grad():
                lp = torch.log_softmax(input.detach(), 2)
                ent = -(lp.exp() * lp).sum(2)
        sel = select_logp(input, seq)
        mask = _shifted_mask(seq, sel)
        scores = get_scores(data_gts, seq, self.opt, as_tensor=True)
        w_fused = None
        if sw > 0:
            selfc = get_self_cider_scores(data_gts, seq, self.opt, as_tensor=True)
            selfc = selfc if torch.is_tensor(selfc) else torch.as_tensor(selfc)
            if (ent is None and torch.is_tensor(scores) and scores.is_cuda and scores.dtype == torch.float64 and n >= 2
                    and sel.dtype == torch.float32 and selfc.is_cuda and selfc.dtype == torch.float64):
                # float32 scores, leave-one-out advantage and the self-CIDEr term in one launch
                scores, w_fused = nsc_advantage(scores.contiguous(), n, selfc.contiguous(), sw)
        if w_fused is None:
            scores = (scores if torch.is_tensor(scores) else torch.as_tensor(scores)).to(sel).view(-1, n)
        out['reward'] = scores
        if ent is not None:
            scores = scores + ew * ((ent * mask).sum(1) / mask.sum(1)).view(-1, n)
        lt = self.loss_type
        if lt in ('new_self_critical', 'best_of_n'):
            if w_fused is not None:
                w = w_fused
            elif lt == 'new_self_critical':         # leave-one-out baseline: the mean score of the image's other samples
                w = scores - (scores.sum(1, keepdim=True) - scores) / (scores.shape[1] - 1)
                if sw > 0:
                    w = w + sw * selfc.to(w).view(-1, 1)
            else:                                   # supervise only the best-scoring sample(s) of each image
                w = (scores == scores.max(1, keepdim=True)[0]).to(sel)
            output = -sel * mask * w.reshape(-1, 1)
            output = output.sum(1) / mask.sum(1) if reduction == 'none' else output.sum() / mask.sum()
        elif lt in ('max_margin', 'multi_margin'):
            # hinge between every sample and the cheapest one of its image, on the mean (masked) logit of the sampled tokens
            assert reduction == 'mean'
            costs = -scores
            avg = ((sel * mask).sum(1) / mask.sum(1)).view(-1, n)
            c_star, i_star = costs.min(1, keepdim=True)
            hinge = torch.relu(costs - c_star - avg.gather(1, i_star) + avg)
            output = (hinge.max(1)[0] / 2).mean() if lt == 'max_margin' else hinge.mean()
        else:
            costs = -scores
            if lt in ('risk', 'softmax_margin'):     # rescale the costs of each image to [0, 1]
                costs = costs - costs.min(1, keepdim=True)[0]
                costs = costs / costs.max(1, keepdim=True)[0]
            tot = (sel * mask).sum(1)
            if lt == 'risk':                         # expected cost under softmax(exp(sequence log-prob)) over the n samples
                assert reduction == 'mean'
                output = (torch.softmax(tot.view(-1, n).exp(), 1) * costs).sum(1).mean()
            else:                                    # cross-entropy towards the cheapest sample of each image
                avg = (tot / mask.sum(1)).view(-1, n)
                if lt in ('softmax_margin', 'real_softmax_margin'):
                    avg = avg + costs
                output = nn.functional.cross_entropy(avg, costs.min(1)[1], reduction=reduction)
        out['loss'] = output
        return out


class _FusedPPO(torch.autograd.Function):
    """PPOLoss's arithmetic on the device: forward = capmi_ppo_loss_fwd (two launches), backward = capmi_ppo_loss_bwd (one launch,
    the dense [N,L,V1] gradient written once; it reaches the rollout backward as its dense `g_dense` input, sparse_logp.split_grad).
    `stats` receives the [4] device tensor pg_loss, kl_loss, clipfrac, loss (no host sync)."""

    @staticmethod
    def forward(ctx, input, lo, seq, scores, n, eps, kl_coef, per_row, stats):
        from imagecaptioning.pytorch_amd import ops
        out, loss_rows, row_stats, msum = ops.ppo_loss_fwd(input.detach(), lo, seq, scores, n, eps, kl_coef, per_row)
        ctx.save_for_backward(lo, seq, row_stats, msum)
        ctx.cfg = (n, eps, kl_coef, per_row)
        stats['out'] = out
        return loss_rows if per_row else out[3]

    @staticmethod
    def backward(ctx, g):
        from imagecaptioning.pytorch_amd import ops
        lo, seq, row_stats, msum = ctx.saved_tensors
        n, eps, kl_coef, per_row = ctx.cfg
        # 'mean': the upstream gradient stays a device scalar (as in sparse_logp._FusedReward)
        grad = ops.ppo_loss_bwd(lo, seq, row_stats, msum, g.reshape(-1).float(), n, eps, kl_coef, per_row)
        return grad, None, None, None, None, None, None, None, None


class PPOLoss(nn.Module):
    """losses.py:267-357: the clipped policy ratio of the sampled tokens against a frozen old policy plus kl_coef times
    KL(old || new) over the whole vocabulary, with new_self_critical's leave-one-out advantage.

    The old model is the live model's family built anew (models.setup) with the weights of ``ppo_old_model_path``, on the live
    model's device, frozen and in eval mode.  It is not deep-copied from the live model (whose native caches are keyed to its own
    buffers), and it is not part of the live model's parameters, state_dict, flat Adam buffer or checkpoint.

    Two routes compute the same numbers: device float32 inputs go through _FusedPPO (capmi_ppo_loss_fwd / _bwd: every dense
    [N,L,V1] row is read once per pass, nothing dense goes through ATen); anything else (CPU tensors, float64) through
    ``generic``, the reference's formula in plain torch."""

    def __init__(self, opt, model):
        super().__init__()
        self.opt = opt
        self.cliprange = getattr(opt, 'ppo_cliprange', 0.2)
        self.kl_coef = getattr(opt, 'ppo_kl_coef', 0.02)
        self.old_model = None
        if getattr(opt, 'use_ppo', 0) == 1:
            path = getattr(opt, 'ppo_old_model_path', None)
            assert path is not None, 'Must provide old model path for PPO'
            from .. import models
            logging.warning('Make sure you are using the same model for PPO loss and the vocab must be the same.')
            dev = next(model.parameters()).device
            state_dict = torch.load(path, map_location=dev)
            if 'pytorch-lightning_version' in state_dict:        # a Lightning checkpoint
                state_dict = state_dict['state_dict']
                del state_dict['_vocab']
                del state_dict['_opt']
            old = models.setup(opt).to(dev)
            old.load_state_dict(state_dict)
            old.eval()
            for p in old.parameters():
                p.requires_grad = False
            self.old_model = old

    def old_logprobs(self, fc_feats, att_feats, seq, att_masks):
        """the old policy's teacher-forced log-probs [N, L, V1] of the sampled tokens (BOS prepended, the last token dropped)"""
        model_input_seq = torch.cat([seq.new_zeros(seq.size(0), 1), seq[:, :-1]], 1)
        with torch.no_grad():
            self.old_model.eval()
            return self.old_model(fc_feats, att_feats, model_input_seq, att_masks)

    def forward(self, input, seq, data_gts, fc_feats, att_feats, att_masks, reduction='mean'):
        """input: what the rollout returned, [N, L, V1] (log-probs; raw logits are read as they are, as the reference does)"""
        N = input.size(0)
        n = N // len(data_gts)
        assert n == self.opt.train_sample_n, n
        scores = get_scores(data_gts, seq, self.opt, as_tensor=True)
        scores = (scores if torch.is_tensor(scores) else torch.as_tensor(scores)).to(device=input.device, dtype=input.dtype)
        lo = self.old_logprobs(fc_feats, att_feats, seq, att_masks)
        return self.loss(input, seq, scores.reshape(-1), lo, reduction)

    def loss(self, input, seq, scores, lo, reduction='mean'):
        """the loss dict of `input` [N, L, V1] against the old log-probs `lo` [N, L, V1] with rewards `scores` [N]"""
        n = self.opt.train_sample_n
        fused = (input.is_cuda and input.dtype == torch.float32 and lo.dtype == torch.float32 and lo.shape == input.shape
                 and input.is_contiguous() and seq.dtype == torch.int64 and n >= 2 and input.size(0) % n == 0 and input.size(1) > 0)
        if not fused:
            return self.generic(input, seq, scores, lo, reduction)
        stats = {}
        loss = _FusedPPO.apply(input, lo.contiguous(), seq.contiguous(), scores.float().contiguous(), n, float(self.cliprange),
                               float(self.kl_coef), reduction == 'none', stats)
        st = stats['out']
        return {'reward': scores.view(-1, n), 'loss': loss, 'pg_loss': st[0], 'kl_loss': st[1], 'clipfrac': st[2]}

    def generic(self, input, seq, scores, lo, reduction='mean'):
        """losses.py:306-357 in plain torch (the route of CPU and float64 tensors)"""
        out = {}
        n = self.opt.train_sample_n
        mask = _shifted_mask(seq, input)
        scores = scores.to(input).view(-1, n)
        out['reward'] = scores
        adv = (scores - (scores.sum(1, keepdim=True) - scores) / (scores.shape[1] - 1)).view(-1, 1)
        ratio = torch.exp(input.gather(2, seq.unsqueeze(2)).squeeze(2) - lo.gather(2, seq.unsqueeze(2)).squeeze(2))
        pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - self.cliprange, 1.0 + self.cliprange))
        kl = nn.functional.kl_div(input, lo, reduction='none', log_target=True).sum(-1)
        msum = mask.sum()
        out['pg_loss'] = (pg * mask).sum() / msum
        out['kl_loss'] = (kl * mask).sum() / msum
        out['clipfrac'] = (((ratio - 1.0).abs() > self.cliprange).to(mask) * mask).sum() / msum
        if reduction == 'none':
            out['loss'] = ((pg + self.kl_coef * kl) * mask).sum(1) / mask.sum(1)
        else:
            out['loss'] = out['pg_loss'] + self.kl_coef * out['kl_loss']
        return out


def check_distill_opt(opt):
    """the start-up refusals of distill_weight > 0 (each with its reason); returns (names, normalised weights)"""
    from imagecaptioning.pytorch_amd import _lib
    names = list(getattr(opt, 'distill_from', None) or [])
    if getattr(opt, 'label_smoothing', 0) > 0:
        raise NotImplementedError('distill_weight > 0 with label_smoothing > 0: the teacher\'s soft targets replace the smoothed '
                                  'hard targets; set label_smoothing 0')
    if getattr(opt, 'scheduled_sampling_start', -1) >= 0 or getattr(opt, 'ss_prob', 0.0) > 0:
        raise NotImplementedError('distill_weight > 0 with scheduled sampling: the student would condition on its own sampled '
                                  'prefix and the teacher on the ground truth; set scheduled_sampling_start -1')
    if not names:
        raise NotImplementedError('distill_weight > 0 needs at least one teacher: distill_from is empty')
    if len(names) > _lib.ENSEMBLE_MAX:
        raise NotImplementedError('distill_from names %d teachers; the mixture kernel takes at most %d (CAPMI_ENSEMBLE_MAX)'
                                  % (len(names), _lib.ENSEMBLE_MAX))
    lam, tau = float(opt.distill_weight), float(getattr(opt, 'distill_temperature', 1.0))
    if not (0.0 < lam <= 1.0) or not (0.0 < tau < float('inf')):
        raise ValueError('distill_weight must lie in (0, 1] and distill_temperature be positive and finite (got %r, %r)' % (lam, tau))
    w = list(getattr(opt, 'distill_weights', None) or [1.0] * len(names))
    if len(w) != len(names) or any(not (x >= 0.0) or x == float('inf') for x in w) or not sum(w) > 0.0:
        raise ValueError('distill_weights: %d finite weights >= 0 with a positive sum expected (got %r)' % (len(names), w))
    tot = float(sum(w))
    return names, [float(x) / tot for x in w]


class DistillTeacher:
    """The frozen teacher of DistillCriterion: the members named by ``distill_from`` (id[-suffix], as tools/eval_ensemble.py --ids
    names them, under ``distill_log_root``), each built as its own family from its saved infos (models.setup) with its weights, on
    the student's device, in eval mode.  Members may be of different families; their vocabulary must be the student's.

    Deliberately not an nn.Module: the members are not part of the student's parameters, state_dict, flat optimizer buffer, EMA or
    checkpoints.  ``members``: already built models instead of saved runs (then nothing is loaded)."""

    def __init__(self, opt, model, members=None):
        self.names, self.weights = check_distill_opt(opt)
        if members is None:
            members = self._load(opt, model)
        if len(members) != len(self.names):
            raise ValueError('%d members for the %d names of distill_from' % (len(members), len(self.names)))
        V = getattr(model, 'vocab_size', None)
        for name, m in zip(self.names, members):
            if getattr(m, 'vocab_size', None) != V:
                raise ValueError('distill_from member %r has another vocabulary than the student (vocab_size %s vs %s)'
                                 % (name, getattr(m, 'vocab_size', None), V))
            m.eval()
            for p in m.parameters():
                p.requires_grad = False
        self.members = list(members)

    def _load(self, opt, model):
        import argparse
        from .. import models
        from ..utils import misc
        from imagecaptioning.pytorch_amd.tools.eval_ensemble import member_paths
        dev = next(model.parameters()).device
        out = []
        for name, (d, id_, suffix, _, model_path) in zip(self.names, member_paths(self.names, getattr(opt, 'distill_log_root', '.'))):
            inf = misc.load_infos_suffixed(d, id_, suffix)
            if getattr(opt, 'vocab', None) is not None and inf.get('vocab') is not None and inf['vocab'] != opt.vocab:
                raise ValueError('distill_from member %r has another vocabulary than the student' % name)
            mopt = argparse.Namespace(**vars(inf['opt']))
            mopt.start_from, mopt.vocab = None, inf.get('vocab', getattr(opt, 'vocab', None))
            m = models.setup(mopt).to(dev)
            m.load_state_dict(torch.load(model_path, map_location=dev))
            out.append(m)
        return out

    def __call__(self, fc_feats, att_feats, seq, att_masks, T):
        """the teacher's log-probs of one batch, [N, >= T, V1] (only the first T steps are meaningful to the caller): every member's
        teacher-forced forward on the student's input tokens; M >= 2 members are mixed by capmi_ensemble_logprobs"""
        lps = []
        with torch.no_grad():
            for m in self.members:
                m.eval()
                lp = m(fc_feats, att_feats, seq, att_masks)
                if lp.size(1) < T:
                    raise RuntimeError('a distillation teacher returned %d steps, the student %d' % (lp.size(1), T))
                lps.append(lp)
            if len(lps) == 1:
                return lps[0]
            if lps[0].is_cuda and all(lp.dtype == torch.float32 for lp in lps):
                from imagecaptioning.pytorch_amd import ops
                cut = [lp if lp.size(1) == T else lp[:, :T].contiguous() for lp in lps]
                N, _, V1 = cut[0].shape
                return ops.ensemble_logprobs([lp.contiguous().view(N * T, V1) for lp in cut], self.weights).view(N, T, V1)
            w = torch.tensor(self.weights, dtype=lps[0].dtype, device=lps[0].device).log().view(-1, 1, 1, 1)
            return torch.logsumexp(torch.stack([torch.log_softmax(lp[:, :T], 2) for lp in lps]) + w, 0)


class _FusedDistill(torch.autograd.Function):
    """DistillCriterion's arithmetic on the device: forward = capmi_distill_loss_fwd (two launches), backward = capmi_distill_loss_bwd
    (one launch, the dense [N,T,V1] gradient written once; it reaches the teacher-forced backward as its dense gradient,
    sparse_logp.split_grad).  `stats` receives the [3] device tensor lm_loss, kd_loss, loss (no host sync)."""

    @staticmethod
    def forward(ctx, input, lt, tok, mask, lam, tau, per_row, stats):
        from imagecaptioning.pytorch_amd import ops
        x = input.detach()
        out, loss_rows, row_stats, msum = ops.distill_loss_fwd(x, lt, tok, mask, lam, tau, per_row)
        ctx.save_for_backward(x, lt, tok, mask, row_stats, msum)
        ctx.cfg = (lam, tau, per_row)
        stats['out'] = out
        return loss_rows if per_row else out[2]

    @staticmethod
    def backward(ctx, g):
        from imagecaptioning.pytorch_amd import ops
        x, lt, tok, mask, row_stats, msum = ctx.saved_tensors
        lam, tau, per_row = ctx.cfg
        # 'mean': the upstream gradient stays a device scalar
        grad = ops.distill_loss_bwd(x, lt, tok, mask, row_stats, msum, g.reshape(-1).float(), lam, tau, per_row)
        return grad, None, None, None, None, None, None, None


class DistillCriterion(nn.Module):
    """Knowledge distillation on the teacher-forced pass: (1 - lambda) NLL(target) + lambda tau^2 KL(softmax(teacher / tau) ||
    softmax(student / tau)), masked means as LanguageModelCriterion's (the normative formula: include/capmi.h, capmi_distill).
    Returns {'loss', 'lm_loss' (masked mean NLL), 'kd_loss' (masked mean KL before lambda and tau^2)}.

    Two routes compute the same numbers: device float32 contiguous inputs go through _FusedDistill (every dense row is read once
    per pass, nothing dense goes through ATen); anything else (CPU tensors, float64) through ``generic``, plain torch."""

    def __init__(self, weight, temperature=1.0):
        super().__init__()
        self.weight, self.temperature = float(weight), float(temperature)

    @staticmethod
    def _dense2d(t, N, T):
        return t.ndim == 2 and t.shape[0] == N and t.shape[1] >= T and (t.shape[1] == 1 or t.stride(1) == 1) and (N == 1 or t.stride(0) >= T)

    def forward(self, input, teacher, target, mask, reduction='mean'):
        if target.ndim == 3:
            target = target.reshape(-1, target.shape[2])
            mask = mask.reshape(-1, mask.shape[2])
        N, T, V1 = input.shape
        fused = (input.is_cuda and input.dtype == torch.float32 and input.is_contiguous() and N > 0 and T > 0
                 and teacher.is_cuda and teacher.dtype == torch.float32 and teacher.ndim == 3 and teacher.shape[0] == N
                 and teacher.shape[1] >= T and teacher.shape[2] == V1 and (V1 == 1 or teacher.stride(2) == 1)
                 and (N == 1 or (teacher.stride(1) > 0 and teacher.stride(0) % teacher.stride(1) == 0
                                 and teacher.stride(0) // teacher.stride(1) >= teacher.shape[1]))
                 and not teacher.requires_grad and target.dtype == torch.int64 and target.is_cuda and mask.is_cuda
                 and not mask.requires_grad and self._dense2d(target, N, T) and mask.ndim == 2 and mask.shape[0] == N
                 and mask.shape[1] >= T)
        if not fused:
            return self.generic(input, teacher, target, mask, reduction)
        if mask.dtype != torch.float32 or not self._dense2d(mask, N, T):
            mask = mask[:, :T].float().contiguous()
        stats = {}
        loss = _FusedDistill.apply(input, teacher, target, mask, self.weight, self.temperature, reduction == 'none', stats)
        st = stats['out']
        return {'loss': loss, 'lm_loss': st[0], 'kd_loss': st[1]}

    def generic(self, input, teacher, target, mask, reduction='mean'):
        """the formula in plain torch (the route of CPU and float64 tensors)"""
        if target.ndim == 3:
            target = target.reshape(-1, target.shape[2])
            mask = mask.reshape(-1, mask.shape[2])
        N, T, V1 = input.shape
        lam, tau = self.weight, self.temperature
        target = target[:, :T]
        mask = mask[:, :T].to(input)
        on = mask != 0
        zero = torch.zeros((), dtype=input.dtype, device=input.device)
        ok = (target >= 0) & (target < V1)
        nll = -input.gather(2, target.clamp(0, V1 - 1).unsqueeze(2)).squeeze(2)
        nll = torch.where(ok, nll, torch.full_like(nll, float('nan')))
        lp_s = torch.log_softmax(input / tau, 2)
        lp_t = torch.log_softmax(teacher[:, :T].detach().to(input) / tau, 2)
        p_t = lp_t.exp()
        kl = torch.where(p_t > 0, p_t * (lp_t - lp_s), zero).sum(2)
        # a masked position is not read: an exact 0, also where it holds an infinity or a NaN
        nll_m, kl_m = torch.where(on, mask * nll, zero), torch.where(on, mask * kl, zero)
        c = torch.where(on, mask * ((1.0 - lam) * nll + lam * tau * tau * kl), zero)
        msum = mask.sum()
        out = {'lm_loss': nll_m.sum() / msum, 'kd_loss': kl_m.sum() / msum}
        out['loss'] = c.sum(1) / mask.sum(1) if reduction == 'none' else c.sum() / msum
        return out
