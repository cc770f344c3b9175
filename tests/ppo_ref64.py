"""An fp64 restatement of the PPO structure loss (reference captioning/modules/losses.py:267-357) with its analytic gradient, the
yardstick of the capmi_ppo_loss_fwd / _bwd kernels (tests/test_ppo_gpu.py).  Checked against the reference's own recorded numbers
on the CPU (tests/test_ppo_host.py).  Works on any device; every input is promoted to float64."""
import torch


def shifted_mask(seq):
    m = (seq > 0).double()
    return torch.cat([m.new_ones(m.size(0), 1), m[:, :-1]], 1)


def advantage(scores, n):
    s = scores.double().view(-1, n)
    return (s - (s.sum(1, keepdim=True) - s) / (n - 1)).reshape(-1)


def ppo64(ln, lo, seq, scores, n, eps=0.2, kl_coef=0.02, per_row=False, u=None):
    """-> dict: kl, r, pg, g_pg, mask [N, L]; pg_loss, kl_loss, clipfrac, loss (mean: scalar; per_row: [N]); kl_bound [N, L] =
    sum_v p_old |lo - ln| (the scale of the KL's rounding); grad [N, L, V1] = d (u . loss) / d ln (u: 1 or [N], default ones)."""
    ln, lo = ln.double(), lo.double()
    N, L, V1 = ln.shape
    m = shifted_mask(seq)
    A = advantage(scores, n).view(-1, 1)
    s = seq.unsqueeze(2)
    r = torch.exp(ln.gather(2, s).squeeze(2) - lo.gather(2, s).squeeze(2))
    p1, p2 = -A * r, -A * r.clamp(1 - eps, 1 + eps)
    pg = torch.maximum(p1, p2)
    inside = ((r >= 1 - eps) & (r <= 1 + eps)).double()
    g_pg = torch.where(p1 > p2, -A * r, torch.where(p2 > p1, torch.where(inside > 0, -A * r, torch.zeros_like(r)),
                                                     torch.where(inside > 0, -A * r, 0.5 * (-A * r))))
    po = lo.exp()
    kl = (po * (lo - ln)).sum(2)
    M = m.sum()
    out = {'kl': kl, 'r': r, 'pg': pg, 'g_pg': g_pg, 'mask': m, 'kl_bound': (po * (lo - ln).abs()).sum(2)}
    out['pg_loss'] = (pg * m).sum() / M
    out['kl_loss'] = (kl * m).sum() / M
    out['clipfrac'] = (((r - 1).abs() > eps).double() * m).sum() / M
    if per_row:
        out['loss'] = ((pg + kl_coef * kl) * m).sum(1) / m.sum(1)
        uu = torch.ones(N, dtype=torch.float64, device=ln.device) if u is None else u.double().reshape(N)
        c = uu.view(-1, 1) * m / m.sum(1, keepdim=True)
    else:
        out['loss'] = out['pg_loss'] + kl_coef * out['kl_loss']
        c = (1.0 if u is None else float(u)) * m / M
    grad = -kl_coef * c.unsqueeze(2) * po
    grad.scatter_add_(2, s, (c * g_pg).unsqueeze(2))
    out['grad'] = grad
    return out
