"""Float64 reference of FlatAdamW's gradient-norm clipping, shared by test_grad_clip_cpu.py and test_grad_clip_gpu.py.

norm = |scale| sqrt(sum g^2) is the global L2 norm of the gradient the optimizer applies (grad_scale included); the coefficient is
torch.nn.utils.clip_grad_norm_'s min(1, max_norm / (norm + 1e-6))."""
import math

import torch


def grad_norm(g, scale=1.0):
    return abs(float(scale)) * math.sqrt(float((g.detach().double().cpu() ** 2).sum()))


def clip_coef(norm, max_norm):
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def assert_margin(norms, max_norm, lo=0.5, hi=2.0):
    """Every norm / max_norm lies outside [lo, hi]: an fp32 rounding of the norm cannot move a step across the clipping threshold."""
    for x in norms:
        r = x / max_norm
        assert not (lo <= r <= hi), "norm / max_norm = %.3f lies inside [%g, %g]" % (r, lo, hi)


def torch_clip(g, max_norm):
    """What torch.nn.utils.clip_grad_norm_ makes of a clone of g (one tensor); returns (clipped gradient, total norm)."""
    p = torch.nn.Parameter(torch.zeros_like(g))
    p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([p], max_norm)
    return p.grad, float(total)
