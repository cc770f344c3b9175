"""float64 truth for the kernels of region_norm.hip (BatchNorm1d over the valid region rows), plain torch on the CPU.

x / dy are [rows, D]; `mask` holds one value per row (0 = padded row), None = every row is valid.  Padded rows are never read: they
may hold NaN.  Pinned against F.batch_norm and its autograd in float64 by test_region_norm_arms_host.py.
"""
import torch
import torch.nn.functional as F

EPS, MOM = 1e-5, 0.1
U = 2.0 ** -24                  # unit roundoff of float32


def valid_rows(mask, rows):
    """bool [rows]: the rows that count"""
    if mask is None:
        return torch.ones(rows, dtype=torch.bool)
    return mask.reshape(-1).cpu() != 0


def inputs(rows, D, mask=None, seed=0):
    """(x, dy) [rows, D] float32.  x: clamp_min(0) of a normal plus, where D >= 5, three hand-made columns -- 1: constant 0,
    2: constant 7, 4: mean 100 with std 0.01 (kernel_inputs of test_use_bn_gpu.py).  dy: a plain normal, NOT multiplied by the mask.
    Padded rows of both hold NaN: a padded row read into any sum shows in every output."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g).clamp_min(0)
    if D >= 5:
        x[:, 1] = 0.0
        x[:, 2] = 7.0
        x[:, 4] = 100.0 + 0.01 * torch.randn(rows, generator=g)
    dy = torch.randn(rows, D, generator=g)
    pad = ~valid_rows(mask, rows)
    x[pad] = float('nan')
    dy[pad] = float('nan')
    return x, dy


def affine(D, seed=5):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)


def forward(x, mask, gamma, beta, steps=1, eps=EPS, momentum=MOM, running_mean=None, running_var=None):
    """train-mode forward: mean, biased var, rstd, y ([rows, D], zero on padded rows), count, and the running buffers after `steps`
    updates with the unbiased variance (from zeros / ones unless given)"""
    rows, D = x.shape
    v = valid_rows(mask, rows)
    x64 = x[v].double()
    M = x64.shape[0]
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    rstd = 1 / torch.sqrt(var + eps)
    y = torch.zeros(rows, D, dtype=torch.float64)
    y[v] = (x64 - mean) * rstd * gamma.double() + beta.double()
    rm = torch.zeros(D, dtype=torch.float64) if running_mean is None else running_mean.double().clone()
    rv = torch.ones(D, dtype=torch.float64) if running_var is None else running_var.double().clone()
    for _ in range(steps):
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * M / (M - 1)
    return dict(mean=mean, var=var, rstd=rstd, y=y, running_mean=rm, running_var=rv, count=M)


def _grads(dy, x, mask, gamma, beta, train, running_mean, running_var, eps, dtype, aten):
    rows, D = x.shape
    v = valid_rows(mask, rows)
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()         # noqa: E731  (never the caller's tensor)
    xin, ga, be = leaf(x[v]), leaf(gamma), leaf(beta)
    if aten:
        rm = None if train else running_mean.to(dtype)
        rv = None if train else running_var.to(dtype)
        y = F.batch_norm(xin, rm, rv, ga, be, train, 0.0, eps)
    else:
        if train:
            mu = xin.mean(0)
            var = ((xin - mu) ** 2).mean(0)
        else:
            mu, var = running_mean.to(dtype), running_var.to(dtype)
        y = (xin - mu) / torch.sqrt(var + eps) * ga + be
    (y * dy[v].to(dtype)).sum().backward()
    dx = torch.zeros(rows, D, dtype=dtype)
    dx[v] = xin.grad
    return dict(dgamma=ga.grad, dbeta=be.grad, dx=dx)


def backward(dy, x, mask, gamma, beta, train, running_mean=None, running_var=None, eps=EPS):
    """dgamma, dbeta, dx ([rows, D], zero on padded rows) by float64 autograd over the valid rows; eval: the running statistics are
    constants"""
    return _grads(dy, x, mask, gamma, beta, train, running_mean, running_var, eps, torch.float64, False)


def aten_backward(dy, x, mask, gamma, beta, train, running_mean=None, running_var=None, eps=EPS, dtype=torch.float32):
    """the same three by ATen's CPU autograd of F.batch_norm over the valid rows in `dtype`"""
    return _grads(dy, x, mask, gamma, beta, train, running_mean, running_var, eps, dtype, True)


def backward_bound(truth, dy, x, mask, gamma, beta, train, running_mean=None, running_var=None, eps=EPS):
    """per quantity 4 x the error of ATen's CPU float32 autograd against `truth` on the same inputs, floor 1e-6 of the largest element
    (the margin and the floor of truth_and_bound in test_use_bn_gpu.py)"""
    a = aten_backward(dy, x, mask, gamma, beta, train, running_mean, running_var, eps)
    return {k: max(4 * float((a[k].double() - truth[k]).abs().max()), 1e-6 * float(truth[k].abs().max())) for k in truth}


def linear_bwd(G0, db, W, mean, rstd, gamma, beta):
    """BatchNorm in front of a Linear (region_norm.hip's header): G = (G0 - db mean^T) diag(rstd), dW = G diag(gamma) + db beta^T,
    dgamma_j = sum_r W_rj G_rj, dbeta_j = sum_r W_rj db_r -- in float64 on the float32 inputs the kernel is given.  With them the
    magnitudes its float32 roundings act on:
      mag_dW     = (|G0| + |db||mean|^T) rstd |gamma| + |db||beta|^T
      mag_dgamma = sum_r |W| (|G0| + |db||mean|^T) rstd
      mag_dbeta  = sum_r |W||db|"""
    G0, db, W, mean, rstd, gamma, beta = (t.detach().double().cpu() for t in (G0, db, W, mean, rstd, gamma, beta))
    G = (G0 - db[:, None] * mean[None, :]) * rstd
    absG = (G0.abs() + db.abs()[:, None] * mean.abs()[None, :]) * rstd
    return dict(dW=G * gamma + db[:, None] * beta[None, :], dgamma=(W * G).sum(0), dbeta=(W * db[:, None]).sum(0),
                mag_dW=absG * gamma.abs() + db.abs()[:, None] * beta.abs()[None, :], mag_dgamma=(W.abs() * absG).sum(0),
                mag_dbeta=(W.abs() * db.abs()[:, None]).sum(0))


def linear_bwd_bound(t, R):
    """elementwise bounds with u = 2^-24: dW 8u mag (at most six roundings per element), dgamma (R + 8)u mag, dbeta (R + 2)u mag"""
    return dict(dW=8 * U * t['mag_dW'], dgamma=(R + 8) * U * t['mag_dgamma'], dbeta=(R + 2) * U * t['mag_dbeta'])
