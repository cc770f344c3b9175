"""LossWrapper (reference captioning/modules/loss_wrapper.py:18-75): picks XE / SCST / structure
loss per step.  Same constructor, call signature and output dict.  Differences are all on the
device side: the SCST reward never leaves HBM (no .cpu().numpy() round trip, rewards.py:48-49)."""
import torch

from . import losses
from ..utils.rewards import self_critical_reward_device, select_gts


class LossWrapper(torch.nn.Module):
    def __init__(self, model, opt):
        super().__init__()
        self.opt = opt
        self.model = model
        from ..models.utils import parse_truncation
        if parse_truncation(getattr(opt, 'train_sample_method', 'sample')) is not None:
            raise NotImplementedError('train_sample_method %r: min-p, epsilon, eta and typical sampling are test-time options '
                                      '(sample_method / sample_n_method); training rollouts have no truncation hook and no '
                                      'gradient through one' % opt.train_sample_method)
        if getattr(opt, 'train_sample_method', 'sample') == 'contrastive':
            raise NotImplementedError("train_sample_method 'contrastive': contrastive search is a test-time option (sample_method); it "
                                      'is deterministic and carries no gradient, a training rollout needs samples')
        if getattr(opt, 'label_smoothing', 0) > 0:
            self.crit = losses.LabelSmoothing(smoothing=opt.label_smoothing)
        else:
            self.crit = losses.LanguageModelCriterion()
        self.rl_crit = losses.RewardCriterion()
        self.struc_crit = losses.StructureLosses(opt) if getattr(opt, 'structure_loss_type', None) else None
        self.ppo_crit = losses.PPOLoss(opt, model) if getattr(opt, 'use_ppo', 0) else None
        # distill_weight > 0: the plain XE branch trains against the frozen teacher of distill_from as well (SCST / structure
        # branches and their lm_loss term keep self.crit).  0, the default: nothing is built, nothing is launched
        self.distill_crit = self.distill_teacher = None
        if getattr(opt, 'distill_weight', 0.0) > 0:
            self.distill_teacher = losses.DistillTeacher(opt, model)          # (not an nn.Module: no parameters of ours)
            self.distill_crit = losses.DistillCriterion(opt.distill_weight, getattr(opt, 'distill_temperature', 1.0))

    def forward(self, fc_feats, att_feats, labels, masks, att_masks, gts, gt_indices, sc_flag, struc_flag,
                drop_worst_flag):
        opt = self.opt
        out = {}
        reduction = 'none' if drop_worst_flag else 'mean'
        if struc_flag:
            use_ppo = bool(getattr(opt, 'use_ppo', 0))
            if use_ppo and opt.structure_loss_type in losses.StructureLosses.LOGIT_TYPES \
                    and not getattr(opt, 'struc_use_logsoftmax', False):
                raise NotImplementedError('use_ppo reads the rollout output; with structure_loss_type %r (max_margin, multi_margin, '
                                          'real_softmax_margin) and no struc_use_logsoftmax that is raw logits, which is not '
                                          'supported' % opt.structure_loss_type)
            if use_ppo and opt.train_beam_size > 1 and opt.train_sample_method in ('greedy', 'beam_search'):
                raise NotImplementedError('use_ppo with train_beam_size > 1: the PPO reference pass re-runs a sampled rollout, not a '
                                          'beam search')
            w = opt.structure_loss_weight
            if w < 1:
                lm_loss = self.crit(self.model(fc_feats, att_feats, labels[..., :-1], att_masks), labels[..., 1:],
                                    masks[..., 1:], reduction=reduction)
            else:
                # (a device fill: the reference's torch.tensor(0).type_as(fc_feats) is a blocking host -> device copy)
                lm_loss = (att_feats if att_feats is not None else fc_feats).new_zeros(())
            if w > 0:
                gen_result, sample_logprobs = self.model(
                    fc_feats, att_feats, att_masks,
                    opt={'sample_method': opt.train_sample_method, 'beam_size': opt.train_beam_size,
                         # loss_wrapper.py:34-35: the margin losses (softmax_margin excepted) read raw logits
                         'output_logsoftmax': int(bool(getattr(opt, 'struc_use_logsoftmax', False))
                                                  or opt.structure_loss_type == 'softmax_margin'
                                                  or 'margin' not in opt.structure_loss_type),
                         'sample_n': opt.train_sample_n}, mode='sample')
                gts = select_gts(gts, gt_indices)
                if use_ppo:
                    struc_loss = self.ppo_crit(sample_logprobs, gen_result, gts, fc_feats, att_feats, att_masks, reduction=reduction)
                else:
                    struc_loss = self.struc_crit(sample_logprobs, gen_result, gts, reduction=reduction)
            else:
                z = (att_feats if att_feats is not None else fc_feats).new_zeros(())
                struc_loss = {'loss': z, 'reward': z, 'pg_loss': z, 'kl_loss': z, 'clipfrac': z}
            loss = (1 - w) * lm_loss + w * struc_loss['loss']
            out['lm_loss'] = lm_loss
            out['struc_loss'] = struc_loss['loss']
            out['reward'] = struc_loss['reward']
            if use_ppo:
                out['pg_loss'] = struc_loss['pg_loss']
                out['kl_loss'] = struc_loss['kl_loss']
                out['clipfrac'] = struc_loss['clipfrac']
        elif not sc_flag and self.distill_crit is not None:
            if getattr(self.model, 'ss_prob', 0.0) > 0:
                raise NotImplementedError('distill_weight > 0 with scheduled sampling: teacher and student would condition on '
                                          'different prefixes')
            logp = self.model(fc_feats, att_feats, labels[..., :-1], att_masks)
            teacher = self.distill_teacher(fc_feats, att_feats, labels[..., :-1], att_masks, logp.size(1))
            d = self.distill_crit(logp, teacher, labels[..., 1:], masks[..., 1:], reduction=reduction)
            loss = d['loss']
            out['lm_loss'] = d['lm_loss']
            out['kd_loss'] = d['kd_loss']
        elif not sc_flag:
            loss = self.crit(self.model(fc_feats, att_feats, labels[..., :-1], att_masks), labels[..., 1:], masks[..., 1:],
                             reduction=reduction)
        else:
            fused = (getattr(self, 'fuse_scst_rollouts', True) and hasattr(self.model, 'scst_rollouts')
                     and opt.sc_sample_method == 'greedy' and opt.sc_beam_size == 1
                     and opt.train_sample_method == 'sample' and opt.train_beam_size == 1)
            if fused:
                # greedy baseline + sampled rollouts in one pass over the weights (see AttModel.scst_rollouts)
                self.model.train()
                greedy_res, gen_result, sample_logprobs = self.model.scst_rollouts(
                    fc_feats, att_feats, att_masks, sample_n=opt.train_sample_n)
            else:
                self.model.eval()
                with torch.no_grad():
                    greedy_res, _ = self.model(fc_feats, att_feats, att_masks, mode='sample',
                                               opt={'sample_method': opt.sc_sample_method, 'beam_size': opt.sc_beam_size})
                self.model.train()
                gen_result, sample_logprobs = self.model(
                    fc_feats, att_feats, att_masks,
                    opt={'sample_method': opt.train_sample_method, 'beam_size': opt.train_beam_size,
                         'sample_n': opt.train_sample_n}, mode='sample')
            gts = select_gts(gts, gt_indices)
            adv, _scores = self_critical_reward_device(greedy_res, gts, gen_result, opt)      # [N] on device
            reward = adv.unsqueeze(1).expand(-1, gen_result.shape[1])
            loss = self.rl_crit(sample_logprobs, gen_result.data, reward, reduction=reduction)
            out['reward'] = getattr(adv, '_capmi_mean', None) if getattr(adv, '_capmi_mean', None) is not None else adv.mean()
        out['loss'] = loss
        return out
