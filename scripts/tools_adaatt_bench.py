"""ms per AdaAtt training step (caption_model adaatt and adaattmo) at the a2i2-like shapes (R = E = A = 512, att_feat 2048,
V1 9488, K 36), with the Att2in2 step of the same tree at the same size beside it for scale: the three models alternate inside one
process, every step is synchronised and timed on its own, and the median with the 10th / 90th percentile is printed.
XE at bs 10 x 5 with T = 16; SCST = 5 sampled rows per image with L = 20 + RewardCriterion backward (train mode, dropout 0.5).
Forward + backward of the model only (no optimizer, no reward computation).

    python scripts/tools_adaatt_bench.py [--steps 30] [--warmup 5] [--once xe|scst --model adaatt]

--once runs one step of one model and nothing else: the process to put behind a kernel trace to count launches.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(name, dev):
    from imagecaptioning.pytorch_amd.captioning import models
    V = 9487
    o = argparse.Namespace(caption_model=name, vocab_size=V, input_encoding_size=512, rnn_size=512, num_layers=1,
                           drop_prob_lm=0.5, seq_length=16, max_length=20, fc_feat_size=2048, att_feat_size=2048,
                           att_hid_size=512, use_bn=0, logit_layers=1, vocab={str(i): 'w%d' % i for i in range(1, V + 1)})
    model = models.setup(o).to(dev)
    model.flatten_parameters_()
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--once', choices=('xe', 'scst'), default=None)
    ap.add_argument('--model', default='adaatt')
    a = ap.parse_args()
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion, RewardCriterion
    torch.manual_seed(0)
    dev = 'cuda:0'
    V, B, n, K = 9487, 10, 5, 36
    fc = torch.randn(B, 2048, device=dev).clamp_min(0)
    att = torch.randn(B, K, 2048, device=dev).clamp_min(0)
    am = torch.ones(B, K, device=dev)
    am[:, 30:] = 0
    am[0] = 1
    labels = torch.randint(1, V + 1, (B, n, 18), device=dev)
    labels[..., 0] = 0
    labels[..., 17:] = 0
    masks = torch.ones(B, n, 18, device=dev)
    reward = torch.randn(B * n, 20, device=dev)

    def xe(model):
        model.train()
        logp = model(fc, att, labels[..., :-1], am)
        LanguageModelCriterion()(logp, labels[..., 1:], masks[..., 1:]).backward()

    def scst(model):
        model.train()
        seq, slp = model(fc, att, am, opt={'sample_method': 'sample', 'sample_n': n}, mode='sample')
        RewardCriterion()(slp, seq, reward).backward()

    steps = {'xe': xe, 'scst': scst}
    if a.once:
        model = build(a.model, dev)
        for _ in range(2):                 # the first call allocates; the trace's last step is the one to read
            steps[a.once](model)
        torch.cuda.synchronize()
        return
    names = ('att2in2', 'adaatt', 'adaattmo')
    built = {k: build(k, dev) for k in names}
    for tag, fn in (('xe bs10x5 T16', xe), ('scst bs10x5 L20', scst)):
        times = {k: [] for k in names}
        for i in range(a.warmup + a.steps):
            for k in names:                # alternating: the models see the same clocks and the same neighbours
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(built[k])
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        for k in names:
            t = sorted(times[k])
            print('%-8s %s: median %.3f ms  (p10 %.3f, p90 %.3f, %d steps)' %
                  (k, tag, t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10], len(t)), flush=True)


if __name__ == '__main__':
    main()
