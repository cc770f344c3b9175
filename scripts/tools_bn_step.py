"""use_bn on one MI355X: whole training steps for a kernel trace, and the trace's BatchNorm rows.

run:      K UpDown steps at the configs size (R = E = 1000, A = 512, 36 x 2048 features, vocabulary 9487) with --use_bn 0 | 1 | 2:
          --mode scst (bs 10 x 5 samples, fused rollout, RewardCriterion on fixed rewards, BPTT, Adam) or --mode xe (bs 64 x 5
          captions).  Meant to run under `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/tools_bn_step.py run ...`.
summary:  the bn_* kernels of such a trace's .db, per step, against the step's whole kernel time.

    python scripts/tools_bn_step.py run --mode scst --use_bn 1 --steps 20
    python scripts/tools_bn_step.py summary trace.db 20
"""
import argparse
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(args):
    import torch
    from imagecaptioning.pytorch_amd import synthetic
    from imagecaptioning.pytorch_amd.captioning import models
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion, RewardCriterion
    dev = 'cuda:0'
    torch.manual_seed(0)
    opt = synthetic.updown_opt(use_bn=args.use_bn)
    model = models.setup(opt).to(dev)
    flat = model.flatten_parameters_()
    model.train()
    B, n, K, L = (10, 5, 36, 20) if args.mode == 'scst' else (64, 5, 36, 20)
    fc = torch.randn(B, 2048, device=dev).clamp_min(0)
    att = torch.randn(B, K, 2048, device=dev).clamp_min(0)
    am = torch.ones(B, K, device=dev)
    for b in range(B):
        am[b, 10 + (b * 7) % 27:] = 0
    am[3] = 1
    labels = torch.randint(1, opt.vocab_size + 1, (B, n, L + 2), device=dev)
    labels[..., 0] = 0
    labels[..., L:] = 0
    masks = (labels > 0).float()
    masks[..., :2] = 1
    reward = torch.randn(B * n, 1, device=dev).repeat(1, L)
    for _ in range(args.steps):
        flat.zero_grad()
        if args.mode == 'scst':
            _, gen, logp = model.scst_rollouts(fc, att, am, sample_n=n)
            loss = RewardCriterion()(logp, gen, reward)
        else:
            loss = LanguageModelCriterion()(model(fc, att, labels[..., :-1], am), labels[..., 1:], masks[..., 1:])
        loss.backward()
        flat.adam_step(5e-4, clip_value=0.1)
    torch.cuda.synchronize()
    print('%s use_bn %d: %d steps, last loss %.4f' % (args.mode, args.use_bn, args.steps, float(loss)))


def summary(args):
    db = sqlite3.connect(args.db)
    rows = db.execute("select name, count(*), sum(end-start)/1e3 from kernels group by name order by 3 desc").fetchall()
    tot = sum(r[2] for r in rows)
    print('kernel time %.3f ms/step over %d steps, %.0f launches/step' % (tot / args.steps / 1e3, args.steps,
                                                                           sum(r[1] for r in rows) / args.steps))
    bn = [r for r in rows if 'bn_' in r[0]]
    print('| kernel | calls/step | us/step |\n|---|---|---|')
    for r in bn:
        print('| `%s` | %.1f | %.1f |' % (r[0].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:80], r[1] / args.steps, r[2] / args.steps))
    print('| all bn_* | %.1f | %.1f |' % (sum(r[1] for r in bn) / args.steps, sum(r[2] for r in bn) / args.steps))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    a = sub.add_parser('run')
    a.add_argument('--mode', choices=('scst', 'xe'), default='scst')
    a.add_argument('--use_bn', type=int, default=1)
    a.add_argument('--steps', type=int, default=20)
    b = sub.add_parser('summary')
    b.add_argument('db')
    b.add_argument('steps', type=int)
    args = ap.parse_args()
    (run if args.cmd == 'run' else summary)(args)
