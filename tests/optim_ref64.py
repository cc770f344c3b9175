"""float64 replay of the fused flat-buffer optimizer rules (capmi_optim_step and, for comparison, capmi_adam_step), written from
the update formulas -- not a test: test_optim_host.py pins it to the torch.optim classes, test_optim_gpu.py holds the kernels to it.

Pre-processing of every rule: g * grad_scale, then clamp to +-clip when clip > 0 (clip_grad_value_).
  rmsprop  g += wd p; sq = alpha sq + (1 - alpha) g^2; p -= lr g / (sqrt(sq) + eps)
  adagrad  g += wd p; sum += g^2; p -= lr g / (sqrt(sum) + eps)
  sgdm     g += wd p; buf = g on the first step, else alpha buf + g; p -= lr buf
  sgdmom   the same buffer; p -= lr (g + alpha buf)                                   (nesterov)
  adamw    p *= 1 - lr wd; m = alpha m + (1 - alpha) g; v = beta v + (1 - beta) g^2;
           p -= lr / (1 - alpha^t) * m / (sqrt(v) / sqrt(1 - beta^t) + eps)
  adam     the same with g += wd p in place of the decoupled decay
"""
import numpy as np
import torch

STATE_KEYS = {'adam': ('exp_avg', 'exp_avg_sq'), 'adamw': ('exp_avg', 'exp_avg_sq'), 'rmsprop': ('square_avg',), 'adagrad': ('sum',),
              'sgdm': ('momentum_buffer',), 'sgdmom': ('momentum_buffer',)}
RULES = ('rmsprop', 'adagrad', 'sgdm', 'sgdmom', 'adamw')


def f32(x):
    """a hyper-parameter as the C ABI receives it (float), as a Python float"""
    return float(np.float32(x))


def new_state(rule, p):
    return {k: torch.zeros_like(p, dtype=torch.float64) for k in STATE_KEYS[rule]}


def step(rule, p, g, state, lr, t, alpha=0.9, beta=0.999, eps=1e-8, weight_decay=0.0, clip=0.0, grad_scale=1.0):
    """one update in place: p float64, g any float dtype, state from new_state(), t the 1-based step number"""
    assert p.dtype == torch.float64
    g = g.double() * grad_scale
    if clip > 0:
        g = g.clamp(-clip, clip)
    if rule in ('adam', 'adamw'):
        m, v = state['exp_avg'], state['exp_avg_sq']
        if rule == 'adamw':
            p.mul_(1.0 - lr * weight_decay)
        elif weight_decay:
            g = g + weight_decay * p
        m.copy_(alpha * m + (1.0 - alpha) * g)
        v.copy_(beta * v + (1.0 - beta) * g * g)
        p.sub_(lr / (1.0 - alpha ** t) * m / (v.sqrt() / (1.0 - beta ** t) ** 0.5 + eps))
        return
    if weight_decay:
        g = g + weight_decay * p
    if rule == 'rmsprop':
        sq = state['square_avg']
        sq.copy_(alpha * sq + (1.0 - alpha) * g * g)
        p.sub_(lr * g / (sq.sqrt() + eps))
    elif rule == 'adagrad':
        s = state['sum']
        s.add_(g * g)
        p.sub_(lr * g / (s.sqrt() + eps))
    elif rule in ('sgdm', 'sgdmom'):
        buf = state['momentum_buffer']
        buf.copy_(g if t == 1 else alpha * buf + g)
        p.sub_(lr * (g + alpha * buf if rule == 'sgdmom' else buf))
    else:
        raise ValueError(rule)
