"""The distillation loss of include/capmi.h (capmi_distill) in float64 plain torch with autograd.  There is no reference counterpart:
this restatement of the normative formula is the yardstick of tests/test_distill_host.py and tests/test_distill_gpu.py.

    a = ls / tau, b = lt / tau, pS = softmax(a), pT = softmax(b)
    kl   = sum_v pT_v (log pT_v - log pS_v)            (a term with pT_v == 0 is exactly 0)
    c    = m ((1 - lambda) (-ls_s) + lambda tau^2 kl)
    loss = sum c / sum m ('mean');  loss[i] = sum_t c / sum_t m ('none')
"""
import torch

D = torch.float64


def distill64(ls, lt, tok, mask, lam, tau, per_row=False, u=1.0):
    """ls [N, T, V1] student log-probs, lt [N, >= T, V1] teacher log-probs, tok / mask [N, >= T]; u: the upstream gradient (a number
    for 'mean', [N] for 'none').  Returns float64 CPU tensors: loss, lm_loss, kd_loss, the per-position kl / nll [N, T], kl_bound
    (sum_v |pT_v (log pT_v - log pS_v)|, the scale of kl's rounding error) and grad = d (u . loss) / d ls."""
    x = ls.detach().cpu().to(D).requires_grad_(True)
    N, T, V1 = x.shape
    y = lt.detach().cpu().to(D)[:, :T]
    s = tok.detach().cpu()[:, :T]
    m = mask.detach().cpu().to(D)[:, :T]
    on = m != 0
    zero = torch.zeros((), dtype=D)
    ok = (s >= 0) & (s < V1)
    nll = -x.gather(2, s.clamp(0, V1 - 1).unsqueeze(2)).squeeze(2)
    nll = torch.where(ok, nll, torch.full_like(nll, float('nan')))
    lp_s = torch.log_softmax(x / tau, 2)
    lp_t = torch.log_softmax(y / tau, 2)
    p_t = lp_t.exp()
    terms = torch.where(p_t > 0, p_t * (lp_t - lp_s), zero)
    kl = terms.sum(2)
    c = torch.where(on, m * ((1.0 - lam) * nll + lam * tau * tau * kl), zero)
    msum = m.sum()
    out = {'lm_loss': (torch.where(on, m * nll, zero).sum() / msum).detach(),
           'kd_loss': (torch.where(on, m * kl, zero).sum() / msum).detach(),
           'kl': kl.detach(), 'nll': nll.detach(), 'kl_bound': terms.detach().abs().sum(2), 'mask': m}
    loss = c.sum(1) / m.sum(1) if per_row else c.sum() / msum
    if per_row:
        uu = torch.as_tensor(u, dtype=D).detach().cpu().reshape(-1)
        live = m.sum(1) > 0                                # (a fully masked sample is NaN: it gets no gradient here)
        (loss[live] * uu[live]).sum().backward()
    else:
        (loss * float(u)).backward()
    out['loss'] = loss.detach()
    out['grad'] = x.grad
    return out
