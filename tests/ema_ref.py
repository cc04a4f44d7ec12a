"""Float64 reference of the weight EMA, shared by test_ema_cpu.py and test_ema_gpu.py.

t counts EMA updates from 1.  The decay at update t is min(decay, (1 + t) / (warmup + t)) for warmup >= 1 and the constant `decay`
for warmup == 0; the weight of the new value is w_t = 1 - that, and the average moves by ema += w_t (p - ema)."""
import torch


def ema_weight(t, decay, warmup):
    if warmup == 0:
        return 1.0 - decay
    return max(1.0 - decay, (warmup - 1.0) / (warmup + float(t)))


def ema_update(ema64, p, t, decay, warmup, active=None):
    """One update of a float64 average with the (float32) weights p; `active` (bool mask) restricts it to some elements."""
    new = ema64 + ema_weight(t, decay, warmup) * (p.double() - ema64)
    return new if active is None else torch.where(active, new, ema64)
