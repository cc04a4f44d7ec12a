"""Scene clearance: the two-launch kernel (diffusion.trajectory_clearance, a3d_traj_clearance) next to the same term written with torch
ops on the device -- what a user of compute_trajectory(num_samples=G) writes by hand without it: torch.cdist of the waypoints
against the cloud, a mask, amin, the hinge and the mean over the scored rows, kept free of host copies.

  python profiles/trajectory_clearance.py [--reps 50] [--rounds 7] [--out profiles/trajectory_clearance.json]

Shapes (B, G, L, C, H, W) = (24, 2, 50, 3, 128, 128), (8, 16, 50, 3, 128, 128), (1, 16, 50, 4, 256, 256); 8-channel poses, suffix
padding of up to L / 4 rows, a cloud of uniform points in the workspace with 10 % of them masked and 2 % broken (a NaN coordinate),
margin 0.05, skip (1, 1).  Both variants are warmed first, then `rounds` rounds ALTERNATE over them (drift of a shared machine hits
both alike), each round timing `reps` back-to-back calls between two device events; per variant the median over rounds and
min .. max.  Also reported: launches (the kernel: 2; the torch sequence: ATen operators dispatched in one call, each at least one
launch) and the peak of temporary device bytes of one call beyond its outputs (the kernel: its workspace of partial minima; torch:
the (B, G L, N) distance matrix and what is made on the way to it).  The torch sequence is run whole; it would be chunked over the
scenes only if the matrix did not fit.  The yardstick is the torch variant of the same run; there is no absolute target.
`clearance` of the two variants is compared on every shape (cdist's default mode expands the norm, so the agreement is loose).
No GPU: the script fails (there is no CPU timing)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(24, 2, 50, 3, 128, 128), (8, 16, 50, 3, 128, 128), (1, 16, 50, 4, 256, 256)]
BOUNDS = [[-0.3, -0.5, 0.6], [0.7, 0.5, 1.6]]
MARGIN, SKIP = 0.05, (1, 1)


def torch_clearance(P, mask, scene, scene_mask, margin, skip):
    """the term in torch ops, stream-ordered (no .item(), no host copy) -> (nearest (B, G, L), clearance (B, G))"""
    B, G, L, _ = P.shape
    C = scene.shape[1]
    pts = scene.reshape(B, C, 3, -1).permute(0, 1, 3, 2).reshape(B, -1, 3)          # (B, N, 3): one copy of the cloud
    counted = torch.isfinite(pts).all(-1) & ~scene_mask.reshape(B, -1)
    pts = torch.where(counted[..., None], pts, torch.zeros_like(pts))               # cdist must not see the NaNs
    d = torch.cdist(P[..., :3].reshape(B, G * L, 3), pts)                            # (B, G L, N)
    d = d.masked_fill(~counted[:, None, :], float("inf"))
    nearest = d.amin(-1).reshape(B, G, L)
    valid = ~mask
    j = torch.cumsum(valid.long(), 1) - 1                                            # rank among the valid rows
    n = valid.sum(1, keepdim=True)
    scored = valid & (j >= skip[0]) & (j < n - skip[1])
    nearest = torch.where(valid[:, None, :], nearest, torch.full_like(nearest, float("inf")))
    hinge = (margin - nearest).clamp(min=0) / margin * scored[:, None, :]
    return nearest, hinge.sum(-1) / scored.sum(1).clamp(min=1)[:, None]


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def inputs(B, G, L, C, H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(BOUNDS[0]), torch.tensor(BOUNDS[1])
    start = lo + (0.3 + 0.4 * torch.rand(B, 1, 1, 3, generator=g)) * (hi - lo)
    pos = start + 0.05 * torch.randn(B, G, 1, 3, generator=g) + torch.cumsum(0.0115 * torch.randn(B, G, L, 3, generator=g), 2)
    P = torch.cat([pos, torch.randn(B, G, L, 4, generator=g), torch.rand(B, G, L, 1, generator=g)], -1)
    pad = torch.randint(0, L // 4 + 1, (B,), generator=g)
    mask = torch.arange(L)[None] >= (L - pad)[:, None]
    scene = lo.view(1, 1, 3, 1, 1) + torch.rand(B, C, 3, H, W, generator=g) * (hi - lo).view(1, 1, 3, 1, 1)
    scene = torch.where(torch.rand(B, C, 3, H, W, generator=g) < 0.02 / 3, torch.full_like(scene, float("nan")), scene)
    scene_mask = torch.rand(B, C, H, W, generator=g) < 0.1
    return P.to(dev), mask.to(dev), scene.to(dev), scene_mask.to(dev)


def peak_temp_bytes(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    kept = sum(t.numel() * t.element_size() for t in out if torch.is_tensor(t))
    return max(0, torch.cuda.max_memory_allocated() - base - kept)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trajectory_clearance.py needs the GPU")
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    result = {"reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "margin": MARGIN, "skip": SKIP, "shapes": []}
    for B, G, L, C, H, W in SHAPES:
        P, mask, scene, scene_mask = inputs(B, G, L, C, H, W, dev)
        runs = {"kernel": lambda: tuple(a3d.trajectory_clearance(P, mask, scene, scene_mask, MARGIN, SKIP)),
                "torch": lambda: torch_clearance(P, mask, scene, scene_mask, MARGIN, SKIP)}
        for run in runs.values():
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        diff = float((runs["kernel"]()[1] - runs["torch"]()[1]).abs().max())
        with CountOps() as c:
            runs["torch"]()
        launches = {"kernel": 2, "torch": c.n}
        temp = {k: peak_temp_bytes(run) for k, run in runs.items()}
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, run in runs.items():
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                st.record()
                for _ in range(a.reps):
                    run()
                en.record()
                torch.cuda.synchronize()
                times[k].append(st.elapsed_time(en) / a.reps * 1e3)
        rec = {"B": B, "G": G, "L": L, "C": C, "H": H, "W": W, "clearance_max_abs_diff": diff}
        for k in runs:
            t = times[k]
            rec[k] = {"us_median": statistics.median(t), "us_min": min(t), "us_max": max(t), "launches": launches[k],
                      "peak_temp_bytes": temp[k]}
            print(f"(B, G, L, C, H, W) = ({B}, {G}, {L}, {C}, {H}, {W}) {k:7s} {rec[k]['us_median']:10.1f} [{min(t):.1f} .. {max(t):.1f}] "
                  f"us per call  launches {launches[k]:3d}  temporaries {temp[k]} B  clearance max abs diff: {diff:.2e}", flush=True)
        result["shapes"].append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
