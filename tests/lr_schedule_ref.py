"""The learning-rate schedule of the fused AdamW, restated once in float64 (numpy only).

`t` is the number of scheduled optimizer steps applied so far, i.e. the 0-based index of the step about to be taken; W = warmup,
N = total, r = min_ratio:

    t <  W                f(t) = t / W
    t >= W, constant      f(t) = 1
    t >= W, linear        f(t) = 1 - (1 - r) u           u = min(1, (t - W) / (N - W))
    t >= W, cosine        f(t) = r + (1 - r) (1 + cos(pi u)) / 2
    lr_t = fp32(lr f(t))                                 everything before the final rounding in double

With r = 0 and t <= N these are the constant / linear / cosine-with-warm-up lambdas of the published diffusion-policy recipes as
torch's LambdaLR applies them (restated, unpinned: `diffusers` is not a dependency).  Past N the rate stays at r lr: u is clamped;
the published cosine lambda rises again there, which is deliberately not copied.

The base rate `lr` of a device schedule is an fp32 (lr_state[3], as `lr` is a float argument of the unscheduled entries): callers
that compare against the device pass the value the device holds, `float(np.float32(lr))`."""
import math

import numpy as np

KINDS = ("constant", "linear", "cosine")


def factor(t, decay, warmup=0, total=None, min_ratio=0.0):
    """f(t) as a float64."""
    if decay not in KINDS:
        raise ValueError("decay = %r" % (decay,))
    t, W, r = np.float64(t), np.float64(warmup), np.float64(min_ratio)
    if t < W:
        return np.float64(t / W)
    if decay == "constant":
        return np.float64(1.0)
    if total is None or not total > warmup:
        raise ValueError("decay = %r needs total > warmup" % (decay,))
    u = min(np.float64(1.0), (t - W) / (np.float64(total) - W))
    if decay == "linear":
        return np.float64(1.0 - (1.0 - r) * u)
    return np.float64(r + (1.0 - r) * (1.0 + math.cos(math.pi * u)) / 2.0)


def rate(t, lr, decay, warmup=0, total=None, min_ratio=0.0):
    """lr_t = fp32(lr f(t)) as a numpy float32."""
    return np.float32(np.float64(lr) * factor(t, decay, warmup, total, min_ratio))


def ulps(got, want):
    """Distance of two float32 values of one sign in units in the last place (0: the same bits, or +0 against -0)."""
    a, b = np.float32(got), np.float32(want)
    if not (np.isfinite(a) and np.isfinite(b)) or (a < 0) != (b < 0):
        return float("inf") if a != b else 0
    return abs(int(np.abs(a).view(np.int32)) - int(np.abs(b).view(np.int32)))
