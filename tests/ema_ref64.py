"""Float64 restatement of the exponential moving average of the parameters (capmi_ema_step / capmi_ema_step_dyn, capmi.h):

    d   = warmup ? min(decay, (1 + step) / (10 + step)) : decay
    ema = d * ema + (1 - d) * p

`d` is the kernel's: decay and the warm-up quotient are float32 numbers (IEEE single-precision add and divide, which numpy's
float32 scalars reproduce), widened exactly.  Everything after it is float64, on whatever device the tensors live on.

Bound the tests hold the kernel to (derived, not tuned): a step of the kernel rounds twice in float32 -- the product (1 - d) * p
and the fused multiply-add -- each by at most 2^-24 of a value no larger than m = max(|ema|, |p|) (a convex combination never
leaves that range), and the error carried in from the step before is scaled by d <= 1.  After S steps: |error| <= 2 * S * 2^-24 * m.
"""
import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of float32


def decay_at(decay, warmup, step):
    """the decay of 1-based step `step` as the kernel computes it, as a Python float (the float32 value, exactly)"""
    d = np.float32(decay)
    if warmup:
        s = np.float32(step)
        d = min(d, (np.float32(1.0) + s) / (np.float32(10.0) + s))
    return float(np.float32(d))


def step(ema64, p, decay, warmup, step_no):
    """one update in place on the float64 tensor `ema64`; p: the parameters of this step (any float dtype)"""
    d = decay_at(decay, warmup, step_no)
    ema64.mul_(d).add_(p.to(torch.float64) * (1.0 - d))
    return ema64


def replay(ema0, ps, decay, warmup, first_step=1):
    """the average after the recorded sequence `ps` of parameter buffers, starting from `ema0`, steps first_step, first_step + 1, ..."""
    e = ema0.to(torch.float64).clone()
    for i, p in enumerate(ps):
        step(e, p, decay, warmup, first_step + i)
    return e


def atol(steps, *tensors):
    """2 * S * 2^-24 * m, m the largest magnitude among the inputs (the initial average and every parameter buffer)"""
    m = max(float(t.abs().max()) for t in tensors)
    return 2.0 * steps * U * m
