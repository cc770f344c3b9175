"""capmi_xe_loss_fwd / _bwd (LanguageModelCriterion and LabelSmoothing as kernels) against the formulas of
captioning/modules/losses.py:39-79 evaluated in float64 with plain torch on the same inputs.

The bound is measured, not fixed: for every case the float32 ATen route (CAPMI_FUSED_XE=0) runs on the same inputs, and the
kernel route may err against the float64 value by at most 4 x what the ATen route errs (both sum the same number of float32 terms,
in another order), with a floor of 4 float32 ulps of the largest reference magnitude (so that an exactly-rounded ATen result does
not make the bound zero: the kernel's last steps -- one product, one quotient, the cast of a double sum -- round three times).
Worst errors seen over all parity cases (units of 1 float32 ulp of the largest reference magnitude) are printed by
test_parity; the figures of the MI355X run are recorded in DESIGN.md."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -23
WORST = {'kernel': 0.0, 'aten': 0.0}


def ref64(x, tgt, mask, smoothing, red):
    """losses.py:39-79 on float64 `x` (the 3-D reshape and the cut to T columns included)"""
    if tgt.ndim == 3:
        tgt, mask = tgt.reshape(-1, tgt.shape[2]), mask.reshape(-1, mask.shape[2])
    N, T, V1 = x.shape
    tgt, mask = tgt[:, :T], mask[:, :T].to(x)
    sel = x.gather(2, tgt.unsqueeze(2)).squeeze(2)
    if smoothing == 0:
        out = -sel * mask
    else:
        conf, off = 1.0 - smoothing, smoothing / (V1 - 1)
        ent = (V1 - 1) * (off * math.log(off) if off > 0 else 0.0) + (conf * math.log(conf) if conf > 0 else 0.0)
        out = (ent - (off * x.sum(2) + (conf - off) * sel)) * mask
    return out.sum(1) / mask.sum(1) if red == 'none' else out.sum() / mask.sum()


def crit_of(smoothing):
    from imagecaptioning.pytorch_amd.captioning.modules.losses import LanguageModelCriterion, LabelSmoothing
    return LanguageModelCriterion() if smoothing == 0 else LabelSmoothing(smoothing=smoothing)


def make_case(N, T, V1, layout, seed=0):
    """log-probs [N, T, V1]; targets / masks 'tight' [N, T], 'wide' [N, T + 2] (the columns past T hold ones and valid tokens: a
    wrong pitch changes the result) or '3d' [B, n, T + 2].  Masks with trailing zeros, the last row on at position 0 only; token 0
    and token V1 - 1 both occur under the mask."""
    g = torch.Generator().manual_seed(seed + 1000 * N + 10 * T + V1)
    x = torch.log_softmax(3.0 * torch.randn(N, T, V1, generator=g), 2)
    W = T if layout == 'tight' else T + 2
    tok = torch.randint(0, V1, (N, W), generator=g)
    lens = torch.randint(1, T + 1, (N,), generator=g)
    if T > 1:
        lens[0] = max(2, T - 2)
    if N > 1:
        lens[N - 1] = 1
    mask = (torch.arange(W)[None, :] < lens[:, None]).float()
    mask[:, T:] = 1.0
    tok[0, 0] = 0
    if N > 1:
        tok[N - 1, 0] = V1 - 1
    elif T > 1:
        tok[0, 1] = V1 - 1
    if layout == '3d':
        n = 5 if N % 5 == 0 else 1
        tok, mask = tok.view(N // n, n, W), mask.view(N // n, n, W)
    return x.to(DEV), tok.to(DEV), mask.to(DEV)


def weights(loss):
    return torch.linspace(0.5, 1.5, loss.numel(), dtype=loss.dtype, device=loss.device).view_as(loss)


def scalar(loss, red):
    return (loss * weights(loss)).sum() if red == 'none' else loss


def run_ref(x, tok, mask, smoothing, red):
    x64 = x.double().requires_grad_(True)
    loss = ref64(x64, tok, mask, smoothing, red)
    scalar(loss, red).backward()
    return loss.detach(), x64.grad


def run_aten(x, tok, mask, smoothing, red, monkeypatch):
    monkeypatch.setenv('CAPMI_FUSED_XE', '0')
    xa = x.clone().requires_grad_(True)
    loss = crit_of(smoothing)(xa, tok, mask, reduction=red)
    scalar(loss, red).backward()
    monkeypatch.delenv('CAPMI_FUSED_XE')
    return loss.detach(), xa.grad


def run_kernel(x, tok, mask, smoothing, red):
    """the criterion on a leaf with a LogpSink: (loss, the sink's (tok, g_sel, g_sum, scale), the leaf)"""
    from imagecaptioning.pytorch_amd import sparse_logp as S
    xk = x.clone().requires_grad_(True)
    sink = S.LogpSink()
    S.attach(xk, sink)
    loss = crit_of(smoothing)(xk, tok, mask, reduction=red)
    assert sink.sel_taken and sink.sum_taken == (smoothing > 0)
    scalar(loss, red).backward()
    return loss.detach(), sink.take(), xk


def dense_of(taken, V1):
    tok, g_sel, g_sum, scale = taken
    s = 1.0 if scale is None else scale.double()
    d = torch.zeros(tok.shape + (V1,), dtype=torch.float64, device=tok.device)
    if g_sum is not None:
        d += g_sum.double().unsqueeze(2)
    d.scatter_add_(2, tok.unsqueeze(2), g_sel.double().unsqueeze(2))
    return d * s


def within_rule(got, aten, ref, what):
    """max |got - ref| <= max(4 max |aten - ref|, 4 ulps of max |ref|); NaNs sit where the reference has them"""
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got.double()), nan), what
    ok = ~nan
    if not bool(ok.any()):
        return
    mag = float(ref[ok].abs().max())
    e_k = float((got.double()[ok] - ref[ok]).abs().max())
    e_a = float((aten.double()[ok] - ref[ok]).abs().max())
    ulp = EPS * mag if mag > 0 else EPS
    WORST['kernel'], WORST['aten'] = max(WORST['kernel'], e_k / ulp), max(WORST['aten'], e_a / ulp)
    print('%s: kernel %.3g  aten %.3g  (ulps of %.3g)' % (what, e_k / ulp, e_a / ulp, mag))
    assert e_k <= max(4.0 * e_a, 4.0 * ulp), (what, e_k, e_a, ulp)


SHAPES = [(1, 1), (3, 7), (40, 7), (50, 22)]       # N * T = 280 > one 256-thread workgroup of the fold; 1100 > 1024


@pytest.mark.parametrize('smoothing', [0.0, 0.1])
@pytest.mark.parametrize('NT', SHAPES)
@pytest.mark.parametrize('V1', [3, 9, 67, 257, 1027, 128])
def test_parity(V1, NT, smoothing, monkeypatch):
    N, T = NT
    for layout in ('tight', 'wide', '3d'):
        x, tok, mask = make_case(N, T, V1, layout)
        for red in ('mean', 'none'):
            what = 'V1=%d N=%d T=%d s=%g %s %s' % (V1, N, T, smoothing, layout, red)
            l_ref, g_ref = run_ref(x, tok, mask, smoothing, red)
            l_at, g_at = run_aten(x, tok, mask, smoothing, red, monkeypatch)
            l_k, taken, xk = run_kernel(x, tok, mask, smoothing, red)
            assert l_k.dtype == torch.float32 and l_k.shape == l_ref.shape
            within_rule(l_k, l_at, l_ref, what + ' loss')
            assert xk.grad is None                              # no dense gradient for the input
            assert taken is not None and (taken[2] is None) == (smoothing == 0)
            assert (taken[3] is None) == (red == 'none')       # 'mean': the upstream scalar travels as `scale`
            assert taken[0].is_contiguous() and tuple(taken[0].shape) == (N, T)
            within_rule(dense_of(taken, V1), g_at, g_ref, what + ' grad')
    print('worst so far: kernel %.3g ulps, aten %.3g ulps' % (WORST['kernel'], WORST['aten']))


@pytest.mark.parametrize('smoothing', [0.0, 0.1])
def test_forward_only_route_needs_no_sink(smoothing, monkeypatch):
    """validation loss: no gradient asked for, the kernel runs without a graph"""
    from imagecaptioning.pytorch_amd import ops
    x, tok, mask = make_case(3, 7, 67, 'wide')
    seen = []
    orig = ops.xe_loss_fwd
    monkeypatch.setattr(ops, 'xe_loss_fwd', lambda *a, **k: (seen.append(1), orig(*a, **k))[1])
    for red in ('mean', 'none'):
        l_ref, _ = run_ref(x, tok, mask, smoothing, red)
        loss = crit_of(smoothing)(x, tok, mask, reduction=red)
        l_at, _ = run_aten(x, tok, mask, smoothing, red, monkeypatch)
        assert not loss.requires_grad
        within_rule(loss, l_at, l_ref, 'forward-only s=%g %s' % (smoothing, red))
    assert len(seen) == 2


@pytest.mark.parametrize('smoothing', [0.0, 0.1])
def test_zero_mask_sums_give_nan_as_the_checker(smoothing, monkeypatch):
    x, tok, mask = make_case(3, 7, 67, 'tight')
    mask[1] = 0
    l_ref, g_ref = run_ref(x, tok, mask, smoothing, 'none')
    l_at, _ = run_aten(x, tok, mask, smoothing, 'none', monkeypatch)
    l_k, taken, _ = run_kernel(x, tok, mask, smoothing, 'none')
    assert torch.isnan(l_ref).tolist() == [False, True, False]
    within_rule(l_k, l_at, l_ref, 'row with an all-zero mask')
    mask.zero_()
    l_k, _, _ = run_kernel(x, tok, mask, smoothing, 'mean')
    assert bool(torch.isnan(l_k)) and bool(torch.isnan(run_ref(x, tok, mask, smoothing, 'mean')[0]))


@pytest.mark.parametrize('red', ['mean', 'none'])
@pytest.mark.parametrize('smoothing', [0.0, 0.1])
def test_two_runs_are_bit_equal(smoothing, red):
    x, tok, mask = make_case(40, 7, 1027, 'wide')
    a = run_kernel(x, tok, mask, smoothing, red)
    b = run_kernel(x, tok, mask, smoothing, red)
    assert torch.equal(a[0], b[0])
    for u, v in zip(a[1], b[1]):
        assert (u is None and v is None) or torch.equal(u, v)


@pytest.mark.parametrize('red', ['mean', 'none'])
@pytest.mark.parametrize('smoothing', [0.0, 0.1])
def test_captured_replay_is_bit_equal_to_the_eager_launch(smoothing, red):
    from imagecaptioning.pytorch_amd.graphs import GraphedDecode
    N, T, V1 = 40, 7, 257
    x0, tok0, mask0 = make_case(N, T, V1, 'wide', seed=0)
    x1, tok1, mask1 = make_case(N, T, V1, 'wide', seed=5)
    mask1[3, 2:] = 0
    w = torch.linspace(0.5, 1.5, N, device=DEV)

    def step(x, tok, mask):
        loss, taken, _ = run_kernel(x, tok, mask, smoothing, red) if red == 'mean' else run_w(x, tok, mask)
        return tuple(t for t in (loss,) + tuple(taken) if t is not None)

    def run_w(x, tok, mask):
        from imagecaptioning.pytorch_amd import sparse_logp as S
        xk = x.detach().requires_grad_(True)
        sink = S.LogpSink()
        S.attach(xk, sink)
        loss = crit_of(smoothing)(xk, tok, mask, reduction='none')
        (loss * w).sum().backward()
        return loss.detach(), sink.take(), xk

    graphed = GraphedDecode()
    graphed('xe', step, (x0, tok0, mask0))
    got = graphed('xe', step, (x1, tok1, mask1))          # the same graph, new contents in the same buffers
    assert len(graphed.cache) == 1
    want = step(x1, tok1, mask1)
    first = step(x0, tok0, mask0)
    assert len(got) == len(want) == 3 + int(smoothing > 0) + int(red == 'mean')      # loss, tok, g_sel (, g_sum) (, scale)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert not torch.equal(first[0], want[0])


def test_invalid_arguments_raise():
    from imagecaptioning.pytorch_amd import ops
    from imagecaptioning.pytorch_amd._lib import CapmiError
    x, tok, mask = make_case(3, 7, 67, 'tight')
    with pytest.raises(CapmiError, match='capmi_xe_loss_fwd'):
        ops.xe_loss_fwd(x, tok[:, :6].contiguous(), mask)                  # tok_ld < T
    with pytest.raises(CapmiError, match='capmi_xe_loss_fwd'):
        ops.xe_loss_fwd(x, tok, mask, smoothing=1.0)
    with pytest.raises(CapmiError, match='capmi_xe_loss_fwd'):
        ops.xe_loss_fwd(torch.empty(3, 7, 0, device=DEV), tok, mask)       # V1 = 0
    _, msum, _ = ops.xe_loss_fwd(x, tok, mask)
    with pytest.raises(CapmiError, match='capmi_xe_loss_bwd'):
        ops.xe_loss_bwd(mask[:, :6].contiguous(), msum, 7, 67)             # mask_ld < T
    with pytest.raises(CapmiError, match='capmi_xe_loss_bwd'):
        ops.xe_loss_bwd(mask, msum, 7, 67, smoothing=1.0)
    with pytest.raises(CapmiError, match='capmi_xe_loss_bwd'):
        ops.xe_loss_bwd(mask, msum, 7, 0)


@pytest.mark.parametrize('family', ['updown', 'newfc', 'transformer'])
def test_one_xe_step_agrees_with_the_old_route(family, tmp_path):
    """One XE step (LanguageModelCriterion, then LabelSmoothing) of a tiny model in two fresh child processes, the route on and
    CAPMI_FUSED_XE=0.  No float64 run of the model exists, so the rule above is applied to what it bounds: the criterion's
    coefficients g_sel / g_sum differ between the routes by at most 4 ulps each (two roundings per route), a parameter gradient
    is a sum of N * T per-position contributions that are linear in them, so it may move by 4 ulps of its largest entry per
    position; the loss by 4 ulps."""
    outs = {}
    for flag in ('1', '0'):
        out = str(tmp_path / ('xe_%s.npz' % flag))
        env = dict(os.environ, CAPMI_FUSED_XE=flag)
        subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'xe_step_child.py'), family, out], env=env, check=True, timeout=300)
        outs[flag] = np.load(out)
    on, off = outs['1'], outs['0']
    assert int(on['select_calls']) == 0 and int(on['sum_calls']) == 0          # no aten::gather, no dense row sum in ATen
    assert int(off['select_calls']) == 2 and int(off['sum_calls']) == 1
    assert set(on.files) == set(off.files) and sum(k.startswith('lm.g.') for k in on.files) > 3
    for k in on.files:
        if k.endswith('.loss'):
            print(k, float(on[k]), float(off[k]))
            assert abs(float(on[k]) - float(off[k])) <= 4 * EPS * abs(float(off[k])), k
        elif '.g.' in k:
            pos = int(on[k.split('.')[0] + '.positions'])
            mag = float(np.abs(off[k]).max())
            err = float(np.abs(on[k] - off[k]).max())
            print('%s: %.3g ulps of its largest entry (%d positions)' % (k, err / (EPS * mag) if mag else 0.0, pos))
            assert err <= 4 * EPS * pos * mag, k
