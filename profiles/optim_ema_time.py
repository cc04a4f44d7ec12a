"""Times the optimizer launch with and without the fused weight EMA on the flat buffer of the keypose model:

  (a) a3d_adamw_step                      -- the plain step, 7 floats moved per element
  (b) (a) followed by ema.lerp_(p, w)     -- the unfused alternative, 10 floats per element and one more launch
  (c) a3d_adamw_ema_step                  -- the fused step, 9 floats per element

n and the parameter offsets are FlatAdamW's for bench.py's model (every trainable parameter), the gradients are random.  Each
variant is warmed up, then timed with device events over windows of back-to-back launches; the windows of the three variants
alternate so that a drift of the machine hits them alike.  Reported: the median window, per call, with the spread of the windows.

    python profiles/optim_ema_time.py [--out profiles/optim_ema_time.txt]

Exits non-zero when (c) is slower than (b): a fused path that loses to the unfused one is not to be shipped."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_ema_time.txt"))
    ap.add_argument("--launches", type=int, default=500, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_ema_time.py measures on the GPU; there is none here")
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    import bench
    dev = torch.device("cuda:0")
    L, E = a3d.lib, a3d.engine
    model = bench.build_model(a3d, dev, torch.bfloat16)
    flat, opt = E.get_optimizer(model, lr=1e-4, ema_decay=0.999, ema_warmup=10)
    n, nseg = flat.n, len(flat.order)
    flat.grad.copy_(torch.randn(n, generator=torch.Generator().manual_seed(0)).to(dev))
    w = 1e-3

    def plain():
        L.call("a3d_adamw_step", flat.flat.data_ptr(), flat.grad.data_ptr(), opt.exp_avg.data_ptr(), opt.exp_avg_sq.data_ptr(),
               opt.step_count.data_ptr(), opt.seg_off.data_ptr(), opt.seg_state.data_ptr(), nseg, n, flat.n_nodecay, 1e-4, 0.9, 0.999,
               1e-8, 0.0, 5e-4, 1.0, L.stream())

    def unfused():
        plain()
        opt.ema.lerp_(flat.flat, w)

    variants = [("a3d_adamw_step", 7, plain), ("a3d_adamw_step + ema.lerp_", 10, unfused), ("a3d_adamw_ema_step", 9, opt.step)]
    for _, _, fn in variants:
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(args.windows):
        for k, (_, _, fn) in enumerate(variants):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.launches):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1e3 / args.launches)              # us per call
    assert torch.isfinite(flat.flat).all() and torch.isfinite(opt.ema).all()
    lines = ["optimizer step on the keypose model's flat buffer: n = %d floats in %d parameters (%s)" % (n, nseg, torch.cuda.get_device_name(0)),
             "device events over %d windows of %d back-to-back calls per variant, windows alternating; us per call" % (args.windows, args.launches)]
    med = []
    for (name, floats, _), ts in zip(variants, times):
        m = statistics.median(ts)
        med.append(m)
        lines.append("  %-28s median %7.2f us  (min %7.2f, max %7.2f)  %2d floats/element -> %6.1f GB/s at the median"
                     % (name, m, min(ts), max(ts), floats, floats * 4.0 * n / (m * 1e-6) / 1e9))
    lines.append("  fused / unfused = %.3f, fused / plain = %.3f" % (med[2] / med[1], med[2] / med[0]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if med[2] > med[1]:
        raise SystemExit("a3d_adamw_ema_step (%.2f us) is slower than a3d_adamw_step + lerp_ (%.2f us)" % (med[2], med[1]))


if __name__ == "__main__":
    main()
