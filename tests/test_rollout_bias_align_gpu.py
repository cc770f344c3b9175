"""Bias gradients whose target is not 16-byte aligned, on a real MI355X.

The BPTT drivers fold each bias gradient into the grouped weight-gradient launch where its target is 16-byte aligned and give it a
capmi_colsum launch of its own otherwise (rollout_common.h grouped_dw_with_bias for Att2in2 and AdaAtt; NewFC's logit bias has
the same branch in newfc.hip).  capmi_colsum writes its output one float at a time, so any 4-byte aligned target is legal.  Torch's
allocator hands out aligned tensors, so here the teacher-forced forward + backward of each family's tiny golden fixture runs
twice through the engine's Rollout: with the gradient targets as allocated, and with every bias gradient that this branch looks at
(MOVED, by capmi_*_grads field) one float into a larger buffer.  Weights, weight gradients and the other bias gradients stay where
they were: the prefill's biases go through a host-side choice of their own (engine_common.prepare_backward), which also picks
another GEMM route for their weight gradients.

Both runs meet the comparison of the family's golden XE test (check_grads in tests/test_att2in2_gpu.py / test_adaatt_gpu.py,
test_newfc_golden_xe_grads_and_greedy in tests/test_model_api_gpu.py: rtol 5e-4, atol 1e-6 + 2e-5 of the largest element)
against the family's float64 restatement, and every gradient that is not a bias is bit-identical between the two.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import adaatt_ref64
import att2in2_ref64
import ss_ref64
from test_adaatt_host import Fixture

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _npz(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _att2in2():
    from imagecaptioning.pytorch_amd import att2in2_engine as E
    z = _npz('att2in2_tiny.npz')
    att, am = z['att'], z['att_masks']
    make = lambda P, cfg: E.Rollout(P, E.prepare(P, att.float().to(DEV), am.float().to(DEV)), **cfg)      # noqa: E731
    return z, E.Rollout, make, lambda P, seq: att2in2_ref64.xe(P, att, am, seq)


def _adaatt(name):
    from imagecaptioning.pytorch_amd import adaatt_engine as E
    fx = Fixture(name)
    z = {k: fx.t(k) for k in fx.files}
    fc, att, am = z['fc'], z['att'], z['att_masks']
    make = lambda P, cfg: E.Rollout(P, E.prepare(P, fc.float().to(DEV), att.float().to(DEV), am.float().to(DEV)), **cfg)   # noqa: E731
    return z, E.Rollout, make, lambda P, seq: adaatt_ref64.xe(P, fc, att, am, seq)


def _newfc():
    from imagecaptioning.pytorch_amd import newfc_engine as E
    z = _npz('newfc_tiny.npz')
    fc = z['fc']
    make = lambda P, cfg: E.Rollout(P, fc.float().to(DEV).contiguous(), **cfg)      # noqa: E731
    return z, E.Rollout, make, lambda P, seq: ss_ref64.newfc_xe(P, fc, seq)[0]


_ADAATT_MOVED = ('logit_b', 'att2h_b', 'fre_b', 'hoe_b', 'fr_b', 'ho_b')
MOVED = {'att2in2': ('logit_b', 'i2h_b', 'h2h_b', 'a2c_b', 'h2att_b'), 'adaatt': _ADAATT_MOVED, 'adaattmo': _ADAATT_MOVED,
         'newfc': ('logit_b',)}
CASES = {'att2in2': _att2in2, 'adaatt': lambda: _adaatt('adaatt'), 'adaattmo': lambda: _adaatt('adaattmo'), 'newfc': _newfc}


def _off_by_one_float(t):
    """a contiguous tensor of t's shape that starts one float into a larger buffer"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize('family', sorted(CASES))
def test_unaligned_bias_gradient_targets(family):
    z, rollout_cls, make, ref_xe = CASES[family]()
    P = {k[2:]: v for k, v in z.items() if k.startswith('P.')}
    labels, masks = z['labels'], z['masks']
    seq = labels[..., :-1].reshape(-1, labels.shape[-1] - 1).long().contiguous()
    N, T = seq.shape
    zero_cols = (seq[:, 1:].sum(0) == 0).nonzero()              # AttModel.py:158-159: stop at the first all-pad column
    T_eff = int(zero_cols[0]) + 1 if zero_cols.numel() else T
    B = z['fc'].shape[0]

    # the float64 restatement, once
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    ss_ref64.lm_loss(ref_xe(P64, seq), labels, masks).backward()
    want = {k: v.grad.numpy() for k, v in P64.items()}

    Pd = {k: v.to(DEV).contiguous() for k, v in P.items()}
    tgt = labels[..., 1:].reshape(N, -1)[:, :T].to(DEV)
    m = masks[..., 1:].reshape(N, -1)[:, :T].float().to(DEV)
    g_logp = torch.zeros(N, T, Pd['logit.weight'].shape[0], device=DEV)
    g_logp.scatter_(2, tgt.unsqueeze(2), (-m / m.sum()).unsqueeze(2))           # d(LanguageModelCriterion) / d(logp)
    biases = [name for field, name in rollout_cls.G_FIELDS if field in MOVED[family]]
    assert len(biases) == len(MOVED[family]) and all(k.endswith('.bias') and k in P for k in biases)

    def run(shift):
        grads = {k: torch.empty_like(v) for k, v in Pd.items()}
        for k in biases if shift else ():
            grads[k] = _off_by_one_float(grads[k])
        ro = make(Pd, dict(n=N // B, T=T_eff, L=T, mode='forced', forced=seq.to(DEV), teacher=True))
        ro.run()
        ro.backward(g_logp, grads)
        torch.cuda.synchronize()
        assert all(v.data_ptr() % 16 == 0 for k, v in grads.items() if not (shift and k in biases))
        return {k: v.cpu() for k, v in grads.items()}

    runs = [run(False), run(True)]
    for got in runs:
        for k, r in want.items():
            np.testing.assert_allclose(got[k].numpy(), r, rtol=5e-4, atol=1e-6 + 2e-5 * np.abs(r).max(), err_msg=k)
    for k in P:
        if k not in biases:
            assert torch.equal(runs[0][k], runs[1][k]), k
