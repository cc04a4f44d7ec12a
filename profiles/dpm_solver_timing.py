"""scheduler="dpm++" next to "ddim" with eta = 0: time of the hipGraph-replayed DiffusionPlanner.compute_trajectory at K = 10, at
cfg-3 (B = 64, L = 16, 3 cameras: S = 3074) and at the deployed horizon (B = 24, L = 50).

  python profiles/dpm_solver_timing.py [--reps 20] [--rounds 5] [--only-ddim] [--root OTHER_CHECKOUT] [--out FILE.json]

Workload and timing as profiles/few_step_sampling.py: synthetic inputs, visual tokens encoded once outside the timed region, context
encoding + K / V cache + AdaLN tables inside every call, the denoise loop replayed from the captured graph; every variant is captured
and warmed first, then `rounds` rounds ALTERNATE over the variants, each timing `reps` back-to-back calls between two device events;
per variant the median over rounds and the spread (min .. max).
--root: import the package and bench_denoise from another checkout of this project (with --only-ddim: one that predates "dpm++",
the parent commit's figure); the caller alternates processes on the two trees.  No GPU: the script fails (there is no CPU timing)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

SHAPES = [("cfg-3", 64, 16), ("horizon-50", 24, 50)]
K = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=3)
    ap.add_argument("--only-ddim", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpm_solver_timing.py needs the GPU")
    sys.path.insert(0, os.path.abspath(a.root))
    BD = importlib.import_module("bench_denoise")
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    result = {"root": os.path.basename(os.path.abspath(a.root)), "K": K, "reps": a.reps, "rounds": a.rounds,
              "device": torch.cuda.get_device_name(0), "shapes": {}}
    variants = [("ddim0", dict(scheduler="ddim"))]
    if not a.only_ddim:
        variants += [("dpm++2M", dict(scheduler="dpm++")), ("dpm++order1", dict(scheduler="dpm++", solver_order=1))]
    for tag, B, Ln in SHAPES:
        s = BD.synthetic_inputs(B, Ln, a.cams, dev)
        n0 = torch.randn(B, Ln, 9, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        args = (s["trajectory_mask"], None, s["pcds"], s["instr"], s["curr_gripper"], s["action"])
        runs, tokens = {}, None
        for name, kw in variants:                      # one planner per variant: each keeps its own captured graph
            m = BD.build_planner(a3d, dev, train=False)
            if tokens is None:
                with torch.no_grad():
                    tokens = m.prediction_head.encode_images(s["rgbs"], None).contiguous()

            def run(m=m, kw=kw, graph=True):
                return m.compute_trajectory(*args, init_noise=n0, visual_tokens=tokens, use_graph=graph, num_inference_steps=K, **kw)
            eager = run(graph=False)
            for _ in range(3):
                out = run()
            torch.cuda.synchronize()
            assert torch.isfinite(out).all() and (out - eager).abs().max().item() <= 1e-4, name
            runs[name] = (run, m.last_sampler_path, out.clone())
        if "dpm++order1" in runs:
            assert torch.equal(runs["dpm++order1"][2], runs["ddim0"][2]) and not torch.equal(runs["dpm++2M"][2], runs["ddim0"][2])
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
        for name, (_, path, _) in runs.items():
            t = times[name]
            rec["variants"][name] = {"sampler": path, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
            print(f"{result['root']:10s} {tag:11s} {name:12s} K={K}  median {statistics.median(t):8.3f} ms  [{min(t):.3f} .. {max(t):.3f}]  {path}",
                  flush=True)
        result["shapes"][tag] = rec
        del runs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
