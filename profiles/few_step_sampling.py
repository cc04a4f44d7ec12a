"""Few-step sampling: time of the hipGraph-replayed DiffusionPlanner.compute_trajectory for K in {10, 20, 50, 100} scheduled steps
next to the default 100-step call, at cfg-3 (B = 64, L = 16, 3 cameras: S = 3074) and at the deployed horizon (B = 24, L = 50).

  python profiles/few_step_sampling.py [--reps 20] [--rounds 5] [--default-only] [--out profiles/few_step_sampling.json]

Workload as bench_denoise.py --mode sample: synthetic inputs, visual tokens encoded once outside the timed region, context encoding
+ K / V cache + AdaLN tables built inside every call, the denoise loop replayed from the captured graph.  Timing: every variant is
captured and warmed first, then `rounds` rounds ALTERNATE over the variants (so drift of the shared machine hits all alike), each
round timing `reps` back-to-back calls between two device events; per variant the median over rounds and the spread (min .. max).
A least-squares line time(K) = setup + K * step over the scheduled variants gives the per-step time and the step-invariant setup.
--default-only times only the default call (this also runs on a tree that predates the schedules: the parent's figure).
No GPU: the script fails (there is no CPU timing)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_denoise as BD  # noqa: E402

SHAPES = [("cfg-3", 64, 16), ("horizon-50", 24, 50)]
KS = [10, 20, 50, 100]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=3)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("few_step_sampling.py needs the GPU")
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    result = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for tag, B, Ln in SHAPES:
        s = BD.synthetic_inputs(B, Ln, a.cams, dev)
        g = torch.Generator(device=dev).manual_seed(5)
        n0, n1 = torch.randn(B, Ln, 9, device=dev, generator=g), torch.randn(100, B, Ln, 9, device=dev, generator=g)
        variants = [("default-100", {})]
        if not a.default_only:
            variants += [(f"ddpm-K{K}", dict(num_inference_steps=K)) for K in KS]
            variants += [("ddim0-K10", dict(num_inference_steps=10, scheduler="ddim")),
                         ("ddim0.5-K20", dict(num_inference_steps=20, scheduler="ddim", eta=0.5))]
        # one planner per variant: each keeps its own captured graph, so alternating between them replays instead of recapturing
        runs = {}
        tokens = None
        for name, kw in variants:
            m = BD.build_planner(a3d, dev, train=False)
            if tokens is None:
                with torch.no_grad():
                    tokens = m.prediction_head.encode_images(s["rgbs"], None).contiguous()
            K = kw.get("num_inference_steps", 100)
            noise = None if (kw.get("scheduler") == "ddim" and kw.get("eta", 0.0) == 0.0) else n1[:K].contiguous()
            args = (s["trajectory_mask"], None, s["pcds"], s["instr"], s["curr_gripper"], s["action"])

            def run(m=m, kw=kw, noise=noise, args=args, graph=True):
                return m.compute_trajectory(*args, init_noise=n0, step_noise=noise, visual_tokens=tokens, use_graph=graph, **kw)
            eager = run(graph=False)
            for _ in range(3):
                out = run()
            torch.cuda.synchronize()
            assert torch.isfinite(out).all() and (out - eager).abs().max().item() <= 1e-4, name
            runs[name] = (run, m.last_sampler_path, K)
        times = {name: [] for name in runs}
        for _ in range(a.rounds):
            for name, (run, _, _) in runs.items():
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                st.record()
                for _ in range(a.reps):
                    run()
                en.record()
                torch.cuda.synchronize()
                times[name].append(st.elapsed_time(en) / a.reps)
        rec = {"B": B, "L": Ln, "S": a.cams * 1024 + 2, "variants": {}}
        for name, (_, path, K) in runs.items():
            t = times[name]
            rec["variants"][name] = {"steps": K, "sampler": path, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t),
                                     "trajectories_per_s": B / statistics.median(t) * 1e3}
        if not a.default_only:
            xs = [float(K) for K in KS]
            ys = [rec["variants"][f"ddpm-K{K}"]["ms_median"] for K in KS]
            mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
            slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
            setup = my - slope * mx
            d, k100, k10 = rec["variants"]["default-100"], rec["variants"]["ddpm-K100"], rec["variants"]["ddpm-K10"]
            rec["fit"] = {"ms_per_step": slope, "setup_ms": setup, "setup_share_at_K10": setup / k10["ms_median"],
                          "K10_over_default": k10["ms_median"] / d["ms_median"],
                          "K100_minus_default_ms": k100["ms_median"] - d["ms_median"],
                          "default_spread_ms": d["ms_max"] - d["ms_min"]}
        result["shapes"][tag] = rec
        for name, v in rec["variants"].items():
            print(f"{tag:11s} {name:12s} {v['steps']:3d} steps  median {v['ms_median']:8.3f} ms  [{v['ms_min']:.3f} .. {v['ms_max']:.3f}]  "
                  f"{v['trajectories_per_s']:8.1f} traj/s  {v['sampler']}", flush=True)
        if "fit" in rec:
            f = rec["fit"]
            print(f"{tag:11s} fit: {f['ms_per_step']:.4f} ms per step + {f['setup_ms']:.3f} ms setup ({100 * f['setup_share_at_K10']:.1f} % of the "
                  f"K = 10 call); K = 10 / default = {f['K10_over_default']:.3f}; K = 100 - default = {f['K100_minus_default_ms']:+.3f} ms "
                  f"(default spread {f['default_spread_ms']:.3f} ms)", flush=True)
        del runs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
