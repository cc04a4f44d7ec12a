"""Chained keypose-to-trajectory inference: time of one Actioner.predict (keypose forward + trajectory sampling on the predicted
goal) at (B, cameras) = (1, 3) and (8, 3), 256 x 256 images, L = 50, with the K = 10 "ddim" schedule and with the full chain, in four
variants that add one stage each:

  separate   share_backbone=False, fused_conditioning=False: the two calls written out by hand (the parent commit's behaviour)
  +share     one pass of the frozen backbone for both models
  +fused     ... and the conditioning seam in one launch (a3d_traj_condition)
  +graph     ... and predict(use_graph=True): one graph for the keypose half, the sampler's captured loop after it

  python profiles/chained_predict.py [--reps 5] [--rounds 5] [--shapes 1,8] [--out profiles/chained_predict.json]

Models: Act3D (3 levels, 10 000 evaluation ghost points, bf16 backbone + FPN) and the script-shape DiffusionPlanner of
bench_denoise.py (bf16 backbone + FPN), both in eval mode and holding the same frozen backbone.  Every variant is warmed first
(the graph variants captured), then `rounds` rounds ALTERNATE over the variants (drift of a shared machine hits all alike), each
round timing `reps` back-to-back calls between two device events; per variant the median over rounds and min .. max.  The frozen
backbone alone (backbone_maps on the same images) is timed in the same rounds: the saving of the shared pass is read against it.
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
import bench as BK  # noqa: E402
import bench_denoise as BD  # noqa: E402

LN = 50
SCHEDULES = [("ddim-K10", dict(num_inference_steps=10, scheduler="ddim")), ("full-chain", dict())]
VARIANTS = [("separate", False, False, False), ("+share", True, False, False), ("+fused", True, True, False),
            ("+graph", True, True, True)]


def build_keypose(a3d, dev):
    torch.manual_seed(0)
    m = a3d.Act3D(backbone="clip", image_size=(256, 256), embedding_dim=60, num_attn_heads=4, gripper_loc_bounds=BK.PERACT_BOUNDS,
                  num_ghost_points=1000, num_ghost_points_val=10000, num_sampling_level=3, weight_tying=True, gp_emb_tying=True,
                  use_instruction=False).to(dev)
    m.backbone_dtype = m.fpn_dtype = torch.bfloat16
    return m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cams", type=int, default=3)
    ap.add_argument("--shapes", default="1,8", help="batch sizes, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chained_predict.py needs the GPU")
    BK.prepare_convolution_search()
    torch.backends.cudnn.benchmark = True
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    kp = build_keypose(a3d, dev)
    backbone = {k: v.clone() for k, v in kp.backbone.state_dict().items()}       # before the first pass converts the weights

    def planner():
        m = BD.build_planner(a3d, dev, train=False)
        m.prediction_head.backbone.load_state_dict(backbone)
        return m

    shared_planner = planner()
    result = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "L": LN, "cameras": a.cams, "shapes": {}}
    for B in [int(x) for x in a.shapes.split(",")]:
        s = BD.synthetic_inputs(B, LN, a.cams, dev, seed=7)
        rgbs = (s["rgbs"] * 2 - 1)[:, None].contiguous()                          # (B, history 1, cameras, 3, H, W) in [-1, 1]
        pcds = s["pcds"][:, None].contiguous()
        gripper = torch.cat([s["curr_gripper"], torch.ones(B, 1, device=dev)], -1)[:, None].contiguous()
        g = torch.Generator(device=dev).manual_seed(5)
        init, step = torch.randn(B, LN, 9, device=dev, generator=g), torch.randn(100, B, LN, 9, device=dev, generator=g)
        runs = {}
        for sname, skw in SCHEDULES:
            kw = dict(skw, init_noise=init)
            if "scheduler" not in skw:
                kw["step_noise"] = step
            for vname, share, fused, graph in VARIANTS:
                # a graph variant keeps the sampler's captured loop in its planner: one planner per (schedule, graph variant)
                pl = planner() if graph else shared_planner
                act = a3d.Actioner(kp, pl, predict_keypose=True, predict_trajectory=True, share_backbone=share, fused_conditioning=fused)
                act.set_instruction(s["instr"][:1])

                def run(act=act, kw=kw, graph=graph):
                    return act.predict(rgbs, pcds, gripper, None, s["trajectory_mask"], use_graph=graph, **kw)
                for _ in range(3):
                    out = run()
                torch.cuda.synchronize()
                assert torch.isfinite(out["trajectory"]).all() and act.last_backbone_passes == (1 if share else 2), (sname, vname)
                runs[(sname, vname)] = (run, pl.last_sampler_path)
        rgb = rgbs[:, -1] / 2 + 0.5
        runs[("backbone", "alone")] = (lambda: kp.backbone_maps(rgb), None)
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, (run, _) in runs.items():
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                st.record()
                for _ in range(a.reps):
                    run()
                en.record()
                torch.cuda.synchronize()
                times[k].append(st.elapsed_time(en) / a.reps)
        rec = {"B": B, "schedules": {}}
        t = times[("backbone", "alone")]
        rec["backbone_alone"] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        print(f"B={B} backbone alone: {rec['backbone_alone']['ms_median']:.3f} [{min(t):.3f} .. {max(t):.3f}] ms", flush=True)
        for sname, _ in SCHEDULES:
            rec["schedules"][sname] = {}
            for vname, _, _, _ in VARIANTS:
                t = times[(sname, vname)]
                v = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "sampler": runs[(sname, vname)][1]}
                rec["schedules"][sname][vname] = v
                print(f"B={B} {sname:10s} {vname:9s} {v['ms_median']:8.3f} [{v['ms_min']:.3f} .. {v['ms_max']:.3f}] ms  {v['sampler']}", flush=True)
        result["shapes"]["B%d" % B] = rec
        del runs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
