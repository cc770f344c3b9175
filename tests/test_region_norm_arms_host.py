"""region_norm_ref64.py, the float64 truth of test_region_norm_arms_gpu.py, pinned on the CPU: against F.batch_norm in float64, against
float64 autograd of F.batch_norm, and (bn_linear_bwd) against autograd through linear(batch_norm(x)).  1e-12 of each quantity's
largest element.  Two small shapes with the hand-made columns and NaN on the padded rows, one masked and one not."""
import pytest
import torch
import torch.nn.functional as F

import region_norm_ref64 as ref

SHAPES = [(23, 9, True), (6, 5, False)]       # (rows, D, masked)
TOL = 1e-12


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def case(rows, D, masked):
    mask = None
    if masked:
        mask = torch.ones(rows)
        mask[:2] = 0            # a leading padded stretch, one in the middle, the tail
        mask[7:10] = 0
        mask[-4:] = 0
    x, dy = ref.inputs(rows, D, mask, seed=3)
    gamma, beta = ref.affine(D)
    g = torch.Generator().manual_seed(17)
    rm, rv = 0.3 * torch.rand(D, generator=g), 0.5 + torch.rand(D, generator=g)
    return x, dy, mask, gamma, beta, rm, rv


@pytest.mark.parametrize('rows,D,masked', SHAPES)
def test_forward_is_f_batch_norm_in_float64(rows, D, masked):
    x, _, mask, gamma, beta, _, _ = case(rows, D, masked)
    v = ref.valid_rows(mask, rows)
    assert int(v.sum()) == (rows - 9 if masked else rows)
    t = ref.forward(x, mask, gamma, beta, steps=3)
    rm, rv = torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
    for _ in range(3):
        y = F.batch_norm(x[v].double(), rm, rv, gamma.double(), beta.double(), True, ref.MOM, ref.EPS)
    assert t['count'] == int(v.sum())
    assert rel(t['y'][v], y) < TOL and rel(t['running_mean'], rm) < TOL and rel(t['running_var'], rv) < TOL
    assert not t['y'][~v].any() and torch.isfinite(t['y']).all()
    x64 = x[v].double()
    assert rel(t['mean'], x64.mean(0)) < TOL and rel(t['var'], x64.var(0, unbiased=False)) < TOL
    assert rel(t['rstd'], 1 / torch.sqrt(x64.var(0, unbiased=False) + ref.EPS)) < TOL
    if D >= 5:                  # the hand-made columns are there
        assert float(t['var'][1]) == 0.0 and float(t['mean'][2]) == 7.0 and abs(float(t['mean'][4]) - 100) < 0.02


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('rows,D,masked', SHAPES)
def test_backward_is_float64_autograd_of_f_batch_norm(rows, D, masked, train):
    x, dy, mask, gamma, beta, rm, rv = case(rows, D, masked)
    v = ref.valid_rows(mask, rows)
    t = ref.backward(dy, x, mask, gamma, beta, train, rm, rv)
    a = ref.aten_backward(dy, x, mask, gamma, beta, train, rm, rv, dtype=torch.float64)
    for k in ('dgamma', 'dbeta', 'dx'):
        assert torch.isfinite(t[k]).all() and rel(t[k], a[k]) < TOL, (k, rel(t[k], a[k]))
    assert not t['dx'][~v].any()
    # the bound the device test uses is finite, positive and above its floor
    b = ref.backward_bound(t, dy, x, mask, gamma, beta, train, rm, rv)
    for k in b:
        assert b[k] >= 1e-6 * float(t[k].abs().max()) > 0


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('rows,D,masked', SHAPES)
def test_linear_bwd_is_autograd_through_linear_of_batch_norm(rows, D, masked, train):
    x, _, mask, gamma, beta, rm, rv = case(rows, D, masked)
    v = ref.valid_rows(mask, rows)
    R = 7
    g = torch.Generator().manual_seed(29)
    W = (torch.randn(R, D, generator=g) / D ** 0.5).double().requires_grad_()
    d_pre = torch.randn(int(v.sum()), R, generator=g).double()
    x64, ga, be = x[v].double(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    bias = torch.zeros(R, dtype=torch.float64, requires_grad=True)
    y = F.batch_norm(x64, None if train else rm.double(), None if train else rv.double(), ga, be, train, 0.0, ref.EPS)
    (F.linear(y, W, bias) * d_pre).sum().backward()
    if train:
        f = ref.forward(x, mask, gamma, beta)
        mean, rstd = f['mean'], f['rstd']
    else:
        mean, rstd = rm.double(), 1 / torch.sqrt(rv.double() + ref.EPS)
    G0, db = d_pre.t() @ x64, d_pre.sum(0)        # the weight gradient on the RAW rows
    assert rel(db, bias.grad) < TOL
    t = ref.linear_bwd(G0, db, W, mean, rstd, gamma, beta)
    want = dict(dW=W.grad, dgamma=ga.grad, dbeta=be.grad)
    # Column 4 (mean 100, std 0.01) is the one place where the formula on the RAW rows is ill-conditioned even in float64: G0 and
    # db mean^T are both near 100 |db| and known to 2^-53 of that, their difference is multiplied by rstd = 100.  Every element is
    # therefore held to 1e-12 of the magnitude its roundings act on (mag_*, the scale of the device bounds), and every column but
    # that one also to 1e-12 of the quantity's largest element.
    keep = torch.ones(D, dtype=torch.bool)
    if train:
        keep[4] = False
    for k in ('dW', 'dgamma', 'dbeta'):
        assert ((t[k] - want[k]).abs() <= TOL * t['mag_' + k]).all(), k
        assert float((t[k] - want[k]).abs()[..., keep].max()) < TOL * float(want[k].abs().max()), k
        assert (t['mag_' + k] >= t[k].abs() * (1 - 1e-12)).all()          # a magnitude bounds its quantity
        assert (ref.linear_bwd_bound(t, R)[k] >= 0).all()
