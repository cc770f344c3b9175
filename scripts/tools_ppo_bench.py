"""The PPO structure loss on one MI355X (V1 = 9488).

1. capmi_ppo_loss_fwd + _bwd against PPOLoss's generic ATen route (forward + autograd gradient to the input) on the same inputs at
   R = 1000 rows (bs 10 x 5, L = 20) and R = 6720 rows, results compared; achieved bytes/s with 2 R V1 4 bytes moved by the
   forward (new + old rows) and 2 R V1 4 by the backward (old rows in, gradient out).
2. One UpDown nsc iteration (sampled rollout of bs 10 x 5, L = 20, structure loss, backward into the parameters; no optimizer, fixed
   scores) with use_ppo 1 against one with new_self_critical: the old model's teacher-forced forward plus the PPO kernels.

Device events after warm-up, median of --runs runs.

    python scripts/tools_ppo_bench.py [--runs 50] [--warmup 10]
"""
import argparse
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = 'cuda:0'
V1 = 9488


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def opt_ns(**kw):
    V = V1 - 1
    o = argparse.Namespace(caption_model='updown', vocab_size=V, input_encoding_size=512, rnn_size=512, num_layers=1,
                           drop_prob_lm=0.5, seq_length=20, max_length=20, fc_feat_size=2048, att_feat_size=2048, att_hid_size=512,
                           use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)}, train_sample_n=5,
                           structure_loss_type='new_self_critical', use_ppo=0, ppo_old_model_path=None, ppo_cliprange=0.2,
                           ppo_kl_coef=0.02, entropy_reward_weight=0, self_cider_reward_weight=0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def kernels(runs, warmup):
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd.captioning.modules.losses import PPOLoss
    crit = PPOLoss(opt_ns(), None)
    for N, L in ((50, 20), (320, 21)):
        R = N * L
        g = torch.Generator(device=DEV).manual_seed(0)
        lo = torch.log_softmax(2 * torch.randn(N, L, V1, device=DEV, generator=g), 2)
        ln = torch.log_softmax(lo + 0.3 * torch.randn(N, L, V1, device=DEV, generator=g), 2)
        seq = torch.randint(1, V1, (N, L), device=DEV, generator=g)
        lens = torch.randint(8, L + 1, (N,), device=DEV, generator=g)
        seq[torch.arange(L, device=DEV).unsqueeze(0) >= lens.unsqueeze(1)] = 0
        scores = torch.rand(N, device=DEV, generator=g)
        u = torch.ones(1, device=DEV)
        st = {}

        def fwd():
            st['f'] = ops.ppo_loss_fwd(ln, lo, seq, scores, 5)

        fwd()

        def bwd():
            out, _, rs, msum = st['f']
            st['g'] = ops.ppo_loss_bwd(lo, seq, rs, msum, u, 5)

        x = ln.clone().requires_grad_(True)

        def aten():
            o = crit.generic(x, seq, scores, lo)
            st['a'] = (o['loss'].detach(), torch.autograd.grad(o['loss'], x)[0])

        t_f, t_b, t_a = timed(fwd, runs, warmup), timed(bwd, runs, warmup), timed(aten, runs, warmup)
        loss_f, loss_a = float(st['f'][0][3]), float(st['a'][0])
        gerr = float((st['g'] - st['a'][1]).abs().max()) / float(st['a'][1].abs().max())
        mb = 2 * R * V1 * 4
        print('R = %5d rows: fused fwd %.1f us (%.2f TB/s) + bwd %.1f us (%.2f TB/s) = %.1f us;  ATen generic fwd+bwd %.1f us '
              '(%.1fx);  loss %.6f vs %.6f, max |d grad| / max |grad| %.1e'
              % (R, t_f * 1e3, mb / t_f / 1e9, t_b * 1e3, mb / t_b / 1e9, (t_f + t_b) * 1e3, t_a * 1e3, t_a / (t_f + t_b),
                 loss_f, loss_a, gerr), flush=True)


def iteration(runs, warmup):
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules import losses
    torch.manual_seed(0)
    model = models.setup(opt_ns()).to(DEV)
    model.flatten_parameters_()
    model.train()
    B, n, K = 10, 5, 36
    fc = torch.zeros(B, 2048, device=DEV)
    att = torch.randn(B, K, 2048, device=DEV).clamp_min(0)
    am = torch.ones(B, K, device=DEV)
    scores = torch.rand(B * n, device=DEV)
    losses.get_scores = lambda gts, s, opt, as_tensor=False: scores
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'old.pth')
        torch.save(model.state_dict(), path)
        ppo = losses.PPOLoss(opt_ns(use_ppo=1, ppo_old_model_path=path), model)
    nsc = losses.StructureLosses(opt_ns())

    def step(use_ppo):
        seq, slp = model(fc, att, am, opt={'sample_method': 'sample', 'beam_size': 1, 'output_logsoftmax': 1, 'sample_n': n},
                         mode='sample')
        if use_ppo:
            o = ppo(slp, seq, [None] * B, fc, att, am)
        else:
            o = nsc(slp, seq, [None] * B)
        o['loss'].backward()

    t0 = timed(lambda: step(False), runs, warmup)
    t1 = timed(lambda: step(True), runs, warmup)
    print('UpDown nsc iteration bs 10 x 5, L 20: new_self_critical %.3f ms, PPO %.3f ms (+%.3f ms, %.0f%%)'
          % (t0, t1, t1 - t0, 100 * (t1 - t0) / t0), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    kernels(a.runs, a.warmup)
    iteration(a.runs, a.warmup)


if __name__ == '__main__':
    main()
