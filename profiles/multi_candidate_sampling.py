"""Multi-candidate sampling: time of the hipGraph-replayed DiffusionPlanner.compute_trajectory(num_samples=G) for G in {1, 2, 4} at a
fixed trajectory count B G, next to the replicated call (today's route to G candidates: every input G times along the batch axis =
the default call on B G samples), at the cfg-3 shape (B G = 64, L = 16, 3 cameras: S = 3074) and at the script horizon (B G = 24,
L = 50).

  python profiles/multi_candidate_sampling.py [--reps 10] [--rounds 5] [--default-only] [--out profiles/multi_candidate_sampling.json]

Workload as bench_denoise.py --mode sample: synthetic inputs, visual tokens encoded once outside the timed region, context encoding
+ K / V cache + AdaLN tables built inside every call, the denoise loop replayed from the captured graph.  Every variant runs the
K = 10 and the K = 50 "ddpm" schedule: time(K) = setup + K step gives the per-step time and the step-invariant setup.  Timing: every
variant is captured and warmed first, then `rounds` rounds ALTERNATE over the variants (drift of the shared machine hits all alike),
each round timing `reps` back-to-back calls between two device events; per variant the median over rounds and min .. max.  Peak
allocated bytes: torch.cuda.max_memory_allocated over one replayed call, minus what was allocated before it.
--default-only times the default call alone (G = None on B G scenes; this also runs on a tree that predates num_samples: the
parent's figure, with A3D_LIB pointing at the parent's library and this script started from the parent's checkout).
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
GS = [1, 2, 4]
KS = [10, 50]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=3)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_candidate_sampling.py needs the GPU")
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    result = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "tree": os.path.dirname(os.path.abspath(a3d.__file__)),
              "shapes": {}}
    for tag, BT, Ln in SHAPES:
        g = torch.Generator(device=dev).manual_seed(5)
        n0, n1 = torch.randn(BT, Ln, 9, device=dev, generator=g), torch.randn(max(KS), BT, Ln, 9, device=dev, generator=g)
        variants = [("default", None)] + ([] if a.default_only else [(f"num_samples-G{G}", G) for G in GS])
        runs = {}
        for name, G in variants:
            B = BT // (G or 1)
            s = BD.synthetic_inputs(B, Ln, a.cams, dev)
            args = (s["trajectory_mask"], None, s["pcds"], s["instr"], s["curr_gripper"], s["action"])
            tokens = None
            for K in KS:
                # one planner per (variant, K): each keeps its own captured graph, so alternating replays instead of recapturing
                m = BD.build_planner(a3d, dev, train=False)
                if tokens is None:
                    with torch.no_grad():
                        tokens = m.prediction_head.encode_images(s["rgbs"], None).contiguous()
                kw = dict(num_inference_steps=K)
                init, step = n0, n1[:K].contiguous()
                if G is not None:
                    kw["num_samples"] = G
                    init, step = n0.reshape(B, G, Ln, 9), step.reshape(K, B, G, Ln, 9)

                def run(m=m, kw=kw, init=init, step=step, args=args, tokens=tokens, graph=True):
                    return m.compute_trajectory(*args, init_noise=init, step_noise=step, visual_tokens=tokens, use_graph=graph, **kw)
                eager = run(graph=False)
                for _ in range(3):
                    out = run()
                torch.cuda.synchronize()
                assert torch.isfinite(out).all() and (out - eager).abs().max().item() <= 1e-4, (name, K)
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                run()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                st_ = getattr(m, "_graph", None) and m._graph.get("state")
                cache = sum(t.numel() * t.element_size() for rec in st_["layers"] for t in (rec["Kf"], rec["Vt"])) if isinstance(st_, dict) and "layers" in st_ else None
                runs[(name, K)] = (run, m.last_sampler_path, peak, cache)
            del s
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, (run, _, _, _) in runs.items():
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                st.record()
                for _ in range(a.reps):
                    run()
                en.record()
                torch.cuda.synchronize()
                times[k].append(st.elapsed_time(en) / a.reps)
        rec = {"trajectories": BT, "L": Ln, "S": a.cams * 1024 + 2, "variants": {}}
        for name, G in variants:
            v = {"G": G, "scenes": BT // (G or 1), "sampler": runs[(name, KS[0])][1], "peak_allocated_bytes": runs[(name, KS[-1])][2],
                 "kv_cache_bytes": runs[(name, KS[-1])][3]}
            for K in KS:
                t = times[(name, K)]
                v[f"K{K}"] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
            lo, hi = v[f"K{KS[0]}"]["ms_median"], v[f"K{KS[-1]}"]["ms_median"]
            v["ms_per_step"] = (hi - lo) / (KS[-1] - KS[0])
            v["setup_ms"] = lo - KS[0] * v["ms_per_step"]
            v["trajectories_per_s_K%d" % KS[-1]] = BT / hi * 1e3
            rec["variants"][name] = v
            print(f"{tag:11s} {name:16s} {v['scenes']:3d} scenes  {v['ms_per_step']:.4f} ms/step  setup {v['setup_ms']:7.3f} ms  "
                  + "  ".join(f"K={K}: {v[f'K{K}']['ms_median']:.3f} [{v[f'K{K}']['ms_min']:.3f} .. {v[f'K{K}']['ms_max']:.3f}] ms" for K in KS)
                  + f"  {v['trajectories_per_s_K%d' % KS[-1]]:8.1f} traj/s  peak {v['peak_allocated_bytes'] / 2**20:.1f} MiB  {v['sampler']}", flush=True)
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
