"""Times the optimizer step with and without global gradient-norm clipping on the flat buffer of the keypose model:

  (a) a3d_adamw_step                                   -- the plain step, two launches
  (b) torch.nn.utils.clip_grad_norm_(flat.grad) + (a)  -- what can be done from outside: the gradient as ONE tensor, clipped in place
  (c) a3d_adamw_clip_step                              -- norm, decision and update in three launches, the gradient left as it is

n and the parameter offsets are FlatAdamW's for bench.py's model (every trainable parameter), the gradients are random and re-filled
from a pristine copy before every window (variant (b) scales them in place).  max_norm is half the gradient's norm, so (b) and (c)
clip in every call.  The protocol is profiles/optim_ema_time.py's: each variant is warmed up, then timed with device events over
windows of back-to-back calls; the windows of the three variants alternate so that a drift of the machine hits them alike.
Reported: the median window, per call, with the range of the windows.

    python profiles/optim_clip_time.py [--out profiles/optim_clip_time.txt]

Exits non-zero when the windows of (c) are not all below the windows of (b)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_clip_time.txt"))
    ap.add_argument("--launches", type=int, default=500, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_clip_time.py measures on the GPU; there is none here")
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    import bench
    dev = torch.device("cuda:0")
    L, E = a3d.lib, a3d.engine
    model = bench.build_model(a3d, dev, torch.bfloat16)
    flat, opt = E.get_optimizer(model, lr=1e-4, max_grad_norm=1.0)
    n, nseg = flat.n, len(flat.order)
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(0)).to(dev)
    opt.max_grad_norm = 0.5 * float(g0.double().norm())
    grad_param = torch.nn.Parameter(flat.flat.detach(), requires_grad=False)     # clip_grad_norm_ wants parameters: one, whose .grad
    grad_param.grad = flat.grad                                                   # is the whole flat gradient

    def plain():
        L.call("a3d_adamw_step", flat.flat.data_ptr(), flat.grad.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(),
               opt.step_count.data_ptr(), opt.seg_off.data_ptr(), opt.seg_state.data_ptr(), nseg, n, flat.n_nodecay, 1e-4, 0.9, 0.999,
               1e-8, 0.0, 5e-4, 1.0, L.stream())

    def torch_clip():
        torch.nn.utils.clip_grad_norm_([grad_param], opt.max_grad_norm)
        plain()

    variants = [("a3d_adamw_step", plain), ("clip_grad_norm_ + a3d_adamw_step", torch_clip), ("a3d_adamw_clip_step", opt.step)]
    for _, fn in variants:
        flat.grad.copy_(g0)
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(args.windows):
        for k, (_, fn) in enumerate(variants):
            flat.grad.copy_(g0)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1e3 / args.launches)              # us per call
    assert torch.isfinite(flat.flat).all() and opt.skipped_steps.item() == 0.0
    assert opt.clipped_steps.item() == 50 + args.windows * args.launches, "variant (c) must have clipped in every call"
    lines = ["optimizer step on the keypose model's flat buffer: n = %d floats in %d parameters (%s)" % (n, nseg, torch.cuda.get_device_name(0)),
             "device events over %d windows of %d back-to-back calls per variant, windows alternating; us per call" % (args.windows, args.launches)]
    med = []
    for (name, _), ts in zip(variants, times):
        m = statistics.median(ts)
        med.append(m)
        lines.append("  %-34s median %7.2f us  (min %7.2f, max %7.2f)" % (name, m, min(ts), max(ts)))
    lines.append("  fused / clip_grad_norm_ = %.3f, fused / plain = %.3f, windows of (c) below windows of (b): %s"
                 % (med[2] / med[1], med[2] / med[0], "yes" if max(times[2]) < min(times[1]) else "NO"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if not max(times[2]) < min(times[1]):
        raise SystemExit("a3d_adamw_clip_step (max %.2f us) is not below clip_grad_norm_ + a3d_adamw_step (min %.2f us)"
                         % (max(times[2]), min(times[1])))


if __name__ == "__main__":
    main()
