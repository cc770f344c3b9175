"""Writes tests/golden/reward_mix.npz: the call site of the BLEU-4 and self-CIDEr rewards, recorded from the reference itself.

    CAPMI_REFERENCE=/path/to/ImageCaptioning.pytorch python tests/golden/make_reward_mix.py

The reference's ``captioning/utils/rewards.py`` and ``captioning/modules/losses.py`` are imported from its checkout and run
unmodified.  Only the three external scorer objects are supplied (coco-caption and the cider submodule are empty directories
there): stubs with the upstream interfaces that hand back recorded pseudo-random scores, BLEU lists and self-CIDEr matrices.
What this pins is therefore the arithmetic AROUND the scorers: which scorer is called for which weights, the mix
cider_reward_weight * cider + bleu_reward_weight * bleu over sampled and greedy rows, the advantage and its repeat along L,
get_scores, get_self_cider_scores' eigenvalue formula, and new_self_critical's leave-one-out baseline with the self-CIDEr term.
The fixture holds arrays only."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

REF = os.environ.get('CAPMI_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = ((1.0, 0.5), (0.0, 1.0), (0.5, 0.5))


def main():
    sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):           # 'cider or coco-caption missing'
        import captioning.utils.rewards as R
        import captioning.modules.losses as RL
    B, n, L, V1 = 4, 3, 6, 11
    N = B * n
    rng = np.random.default_rng(20241017)
    cider = rng.random(N + B) * 2.0
    bleu = rng.random(N + B)
    X = rng.standard_normal((B, n, 5))
    K = np.einsum('bik,bjk->bij', X, X)
    K = K / np.sqrt(np.einsum('bii->bi', K))[:, :, None] / np.sqrt(np.einsum('bii->bi', K))[:, None, :] * 10.0
    K = (K + K.transpose(0, 2, 1)) / 2
    K[1] = 10.0                                                # identical captions: rank 1
    calls = {'ciderd': 0, 'bleu': 0, 'cider': 0}

    class CiderDStub:
        def compute_score(self, gts, res):
            calls['ciderd'] += 1
            assert len(gts) == len(res)
            return float(cider[:len(res)].mean()), cider[:len(res)].copy()

    class BleuStub:
        def compute_score(self, gts, res):
            calls['bleu'] += 1
            assert len(gts) == len(res)
            return [0.0] * 4, [list(bleu[:len(res)] * (k + 1) / 4) for k in range(4)]

    class CiderStub:
        def __init__(self):
            self.i = 0

        def my_self_cider(self, groups):
            calls['cider'] += 1
            assert len(groups) == 1 and len(groups[0]) == n
            out = K[self.i % B].copy()
            self.i += 1
            return [out]

    R.CiderD_scorer, R.Bleu_scorer, R.Cider_scorer = CiderDStub(), BleuStub(), CiderStub()

    g = torch.Generator().manual_seed(271)
    seq = torch.randint(1, V1, (N, L), generator=g)
    for r, ln in enumerate([6, 3, 1, 0, 5, 2, 6, 4, 1, 3, 2, 5]):      # ragged: EOS at step 0, no EOS at all, ...
        seq[r, ln:] = 0
    greedy = torch.randint(1, V1, (B, L), generator=g)
    greedy[0, 2:] = 0
    gts = [np.ones((2, L), dtype=np.int64) for _ in range(B)]
    logits = torch.randn(N, L, V1, generator=g, dtype=torch.float32)
    out = dict(B=np.array(B), n=np.array(n), seq=seq.numpy(), greedy=greedy.numpy(), cider=cider, bleu=bleu, K=K,
               logits=logits.numpy(), pairs=np.array(PAIRS))
    with contextlib.redirect_stdout(io.StringIO()):
        for i, (cw, bw) in enumerate(PAIRS):
            opt = argparse.Namespace(cider_reward_weight=cw, bleu_reward_weight=bw)
            before = dict(calls)
            out['reward_%d' % i] = R.get_self_critical_reward(greedy, gts, seq, opt)
            out['scores_%d' % i] = np.asarray(R.get_scores(gts, seq, opt), dtype=np.float64)
            out['calls_%d' % i] = np.array([calls['ciderd'] - before['ciderd'], calls['bleu'] - before['bleu']])
        opt = argparse.Namespace(structure_loss_type='new_self_critical', train_sample_n=n, entropy_reward_weight=0,
                                 self_cider_reward_weight=0.3, cider_reward_weight=0.5, bleu_reward_weight=0.5)
        out['struct_weights'] = np.array([0.5, 0.5, 0.3])
        R.Cider_scorer.i = 0
        out['self_cider'] = np.asarray(R.get_self_cider_scores(gts, seq, opt), dtype=np.float64)
        for red in ('mean', 'none'):
            R.Cider_scorer.i = 0
            x = torch.log_softmax(logits.clone(), 2).requires_grad_(True)
            o = RL.StructureLosses(opt)(x, seq, gts, reduction=red)
            loss = o['loss']
            w = torch.linspace(0.5, 1.5, loss.numel()).view_as(loss) if red == 'none' else None
            (loss if w is None else (loss * w).sum()).backward()
            out['struct_%s_loss' % red] = loss.detach().numpy()
            out['struct_%s_grad' % red] = x.grad.numpy()
            out['struct_%s_reward' % red] = o['reward'].numpy()
    assert np.isfinite(out['self_cider']).all()
    np.savez_compressed(os.path.join(HERE, 'reward_mix.npz'), **out)
    print('reward_mix.npz: %d arrays, %d bytes; self_cider %s' % (len(out), os.path.getsize(os.path.join(HERE, 'reward_mix.npz')),
                                                                 out['self_cider']))


if __name__ == '__main__':
    main()
