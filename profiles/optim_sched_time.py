"""Times the optimizer step with and without the device-resident learning-rate schedule on the flat buffer of the
keypose model:

  (a) a3d_adamw_step                          -- the plain step, two launches, the rate a kernel argument
  (b) a3d_adamw_sched_step, cosine schedule   -- the same two launches; the prepare launch derives the rate (double cos, one thread
                                                 per workgroup), the update launch reads it from lr_state and counts the step

n and the parameter offsets are FlatAdamW's for bench.py's model (every trainable parameter), the gradients are random.  The
schedule is long (warm-up 1000, total 10^6 steps) so that every timed call of (b) is in the warm-up or on the cosine, never on the
clamp.  The protocol is profiles/optim_ema_time.py's: each variant is warmed up, then timed with device events over windows of
back-to-back calls; the windows of the two variants alternate so that a drift of the machine hits them alike.  Reported: the median
window, per call, with the range of the windows, the difference of the medians and whether the windows overlap.

    python profiles/optim_sched_time.py [--out profiles/optim_sched_time.txt]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_sched_time.txt"))
    ap.add_argument("--launches", type=int, default=500, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_sched_time.py measures on the GPU; there is none here")
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    import bench
    dev = torch.device("cuda:0")
    L, E = a3d.lib, a3d.engine
    model = bench.build_model(a3d, dev, torch.bfloat16)
    flat, opt = E.get_optimizer(model, lr=1e-4, lr_schedule=dict(decay="cosine", warmup=1000, total=10 ** 6, min_ratio=0.1))
    n, nseg = flat.n, len(flat.order)
    flat.grad.copy_(torch.randn(n, generator=torch.Generator().manual_seed(0)).to(dev))

    def plain():
        L.call("a3d_adamw_step", flat.flat.data_ptr(), flat.grad.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(),
               opt.step_count.data_ptr(), opt.seg_off.data_ptr(), opt.seg_state.data_ptr(), nseg, n, flat.n_nodecay, 1e-4, 0.9, 0.999,
               1e-8, 0.0, 5e-4, 1.0, L.stream())

    variants = [("a3d_adamw_step", plain), ("a3d_adamw_sched_step (cosine)", opt.step)]
    for _, fn in variants:
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(args.windows):
        for k, (_, fn) in enumerate(variants):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1e3 / args.launches)              # us per call
    assert torch.isfinite(flat.flat).all()
    assert opt.schedule_step.item() == 50 + args.windows * args.launches, "variant (b) must have counted every one of its calls"
    assert 0.0 < opt.current_lr.item() <= 1e-4
    lines = ["optimizer step on the keypose model's flat buffer: n = %d floats in %d parameters (%s)" % (n, nseg, torch.cuda.get_device_name(0)),
             "device events over %d windows of %d back-to-back calls per variant, windows alternating; us per call" % (args.windows, args.launches)]
    med = []
    for (name, _), ts in zip(variants, times):
        m = statistics.median(ts)
        med.append(m)
        lines.append("  %-34s median %7.2f us  (min %7.2f, max %7.2f)" % (name, m, min(ts), max(ts)))
    overlap = max(times[0]) >= min(times[1]) and max(times[1]) >= min(times[0])
    lines.append("  scheduled - plain = %+.2f us (%.3f x), windows overlap: %s" % (med[1] - med[0], med[1] / med[0], "yes" if overlap else "no"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
