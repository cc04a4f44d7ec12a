"""Bit record of the scene-cloud scan refactor (csrc/traj_points.h: tc_scan_partial, tc_scan_plan): SHA-256 of every output tensor of
a3d_traj_clearance / a3d_traj_guide and of trajectory_clearance / guide_trajectories on seeded inputs, taken once on the parent's
checkout and once on this tree, one process each.

    python profiles/traj_scan_equivalence.py [--root CHECKOUT] --out listing.txt         # one line per tensor: <call> <tensor> <sha256>
    python profiles/traj_scan_equivalence.py --join parent.txt new.txt --out profiles/traj_scan_equivalence.txt

--root names the checkout whose package is imported (default: this file's); the cases are this file's, the inputs those of the seeded
generators of tests/traj_clearance_ref.py and tests/traj_guide_ref.py (seed 0, Dp 8 / D 10).  Cases: the six shapes of the GPU tests
and the two-tile shape (1, 64, 17, 1, 3, 7) x mask kind (none, suffix, scattered) x with / without a scene mask; the raw entries with
n_chunks 1, 3 and 0, the public functions once.  Guidance: push 1, smooth 0.5.  --join puts two listings side by side, one line per
call, every digest cut to its first 16 hex digits, and ends with the SHA-256 of each whole listing.  No GPU: recording fails."""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import traj_clearance_ref as C  # noqa: E402
import traj_guide_ref as GR  # noqa: E402

SHAPES = [(1, 1, 1, 1, 1, 1), (2, 3, 5, 1, 3, 7), (2, 4, 17, 3, 16, 16), (1, 8, 50, 2, 64, 64), (1, 64, 16, 1, 33, 31),
          (2, 2, 100, 4, 32, 32), (1, 64, 17, 1, 3, 7)]
MASKS = ("none", "suffix", "scattered")
PUSH, SMOOTH = 1.0, 0.5


def sha(x):
    return hashlib.sha256(x.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def t(x, dev, dtype=None):
    return None if x is None else torch.from_numpy(np.array(x, dtype=dtype, order="C")).to(dev).contiguous()


def raw_clearance(a3d, P, tm, S, sm, n_chunks):
    B, G, L, Dp = P.shape
    n_cam, n_pix = S.shape[1], S.shape[3] * S.shape[4]
    ws = torch.empty(a3d.lib.load().a3d_traj_clearance_ws_floats(B, G, L, n_cam * n_pix, n_chunks), device=P.device)
    near, clear = torch.empty(B, G, L, device=P.device), torch.empty(B, G, device=P.device)
    a3d.lib.call("a3d_traj_clearance", P.data_ptr(), tm.data_ptr(), S.data_ptr(), None if sm is None else sm.data_ptr(), n_cam, n_pix,
                 float(C.MARGIN), int(C.SKIP[0]), int(C.SKIP[1]), near.data_ptr(), clear.data_ptr(), ws.data_ptr(), n_chunks, B, G, L, Dp,
                 a3d.lib.stream())
    return near, clear


def raw_guide(a3d, X, tm, cm, bd, S, sm, n_chunks):
    B, G, L, D = X.shape
    n_cam, n_pix = S.shape[1], S.shape[3] * S.shape[4]
    ws = torch.empty(a3d.lib.load().a3d_traj_guide_ws_floats(B, G, L, n_cam * n_pix, n_chunks), device=X.device)
    x, near = X.clone(), torch.empty(B, G, L, device=X.device)
    a3d.lib.call("a3d_traj_guide", x.data_ptr(), D, tm.data_ptr(), cm.data_ptr(), bd.data_ptr(), S.data_ptr(),
                 None if sm is None else sm.data_ptr(), n_cam, n_pix, float(GR.MARGIN), int(GR.SKIP[0]), int(GR.SKIP[1]), PUSH, SMOOTH,
                 near.data_ptr(), ws.data_ptr(), n_chunks, B, G, L, a3d.lib.stream())
    return x, near


def record(a3d, dev):
    """-> the lines "<call> <tensor> <sha256>"; a call is named without blanks"""
    lines = []
    for shape in SHAPES:
        for kind in MASKS:
            for with_mask in (False, True):
                tag = "%s/%s/%s" % ("x".join(map(str, shape)), kind, "scene-mask" if with_mask else "all-points")
                P, mask, _, _, S, sm = C.make_inputs(0, *shape, 8, kind)
                Pd, tm, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(S, dev), (t(sm, dev, np.uint8) if with_mask else None)
                calls = [("a3d_traj_clearance/n_chunks=%d" % c, raw_clearance(a3d, Pd, tm, Sd, smd, c)) for c in (1, 3, 0)]
                calls.append(("trajectory_clearance", tuple(a3d.trajectory_clearance(Pd, tm.bool(), Sd, None if smd is None else smd.bool()))))
                lines += ["%s/%s %s %s" % (tag, name, k, sha(v)) for name, out in calls for k, v in zip(("nearest", "clearance"), out)]
                P, mask, bounds, S, sm, cm = GR.make_inputs(0, *shape, 10, kind)
                bd, tm, Sd, cmd = t(bounds, dev), t(mask, dev, np.uint8), t(S, dev), t(cm, dev)
                smd = t(sm, dev, np.uint8) if with_mask else None
                X = a3d.diffusion.pose_to_signal(t(P, dev), bd)
                calls = [("a3d_traj_guide/n_chunks=%d" % c, raw_guide(a3d, X, tm, cmd, bd, Sd, smd, c)) for c in (1, 3, 0)]
                x = X.clone()
                near = a3d.guide_trajectories(x, tm.bool(), Sd, bd, scene_mask=None if smd is None else smd.bool(), cond_mask=cmd, push=PUSH,
                                              smooth=SMOOTH, want_nearest=True)
                calls.append(("guide_trajectories", (x, near)))
                lines += ["%s/%s %s %s" % (tag, name, k, sha(v)) for name, out in calls for k, v in zip(("signals", "nearest"), out)]
    torch.cuda.synchronize()
    return lines


def join(parent, new):
    """two listings side by side: <call> then per tensor <name> <parent digest> <new digest>, digests cut to 16 hex digits"""
    texts = [open(p).read() for p in (parent, new)]
    a, b = (x.splitlines() for x in texts)
    assert len(a) == len(b) and len(a) % 2 == 0, (len(a), len(b))
    equal = sum(x == y for x, y in zip(a, b))
    out = ["profiles/traj_scan_equivalence.py on an MI355X: the parent commit's checkout (--root) and this tree, one process each.",
           "<call>  <tensor> <parent> <new>  <tensor> <parent> <new>: SHA-256 per output tensor, first 16 hex digits.  %d tensors, %d equal."
           % (len(a), equal), ""]
    for i in range(0, len(a), 2):
        cells = []
        for x, y in zip(a[i:i + 2], b[i:i + 2]):
            (cx, kx, hx), (cy, ky, hy) = x.split(" "), y.split(" ")
            assert (cx, kx) == (cy, ky) and cx == a[i].split(" ")[0]
            cells.append("%s %s %s" % (kx, hx[:16], hy[:16]))
        out.append("%s  %s" % (a[i].split(" ")[0], "  ".join(cells)))
    out += ["", "SHA-256 of the whole listing (full digests): parent %s" % hashlib.sha256(texts[0].encode()).hexdigest(),
            "                                             new    %s" % hashlib.sha256(texts[1].encode()).hexdigest()]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--join", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.join:
        text = join(*a.join)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("traj_scan_equivalence.py needs the GPU")
        sys.path.insert(0, os.path.abspath(a.root))
        lines = record(importlib.import_module("act3d-chained-diffuser_amd"), torch.device("cuda:0"))
        text = "\n".join(lines) + "\n"
        print("%d tensors, digest of the listing %s" % (len(lines), hashlib.sha256(text.encode()).hexdigest()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
