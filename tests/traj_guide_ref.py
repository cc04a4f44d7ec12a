"""Float64 restatement of one clearance-guidance step (a3d_traj_guide, csrc/traj_guide.hip; diffusion.guide_trajectories,
compute_trajectory(guide=...)), the seeded inputs of its tests and the per-row error bound of the GPU test.

CPU-only module shared by tests/test_traj_guide_cpu.py (the restatement is right) and tests/test_traj_guide_gpu.py (the kernel against
it).  Nothing here imports the package under test; poses, masks and scenes come from tests/traj_clearance_ref.py.

Semantics.  signals X (B, G, L, D), D in {9, 10}, only channels 0..2 are read or written: positions normalised to bounds (2, 3) = lo, hi.
mask (B, L), non-zero = padded row, any pattern; cond_mask None or (B G, L, D) bytes, the sampler's in-painting mask; scene, scene_mask,
margin, skip and "counted point" as in traj_clearance_ref.
    world     p = (x + 1) / 2 * (hi - lo) + lo
    free row  valid; skip_head <= j < n_b - skip_tail over the rank j among the n_b valid rows of the scene; cond_mask[row][0] == 0;
              p finite.  Every other row keeps its values, and so do channels 3.. of every row.
    push      s* = the counted point of smallest d^2 (ties: the smallest index n = c n_pix + pixel), d = sqrt(d^2);
              u = push (margin - d) (p - s*) / d when 0 < d < margin, else 0 (d == 0 and no counted point included)
    smooth    v = smooth ((p_prev + p_next) / 2 - p): prev and next are the neighbouring VALID rows by rank (pinned rows count), all
              positions read before any update; 0 when a neighbour is missing or not finite
    update    x' = x + (u + v) 2 / (hi - lo)
    nearest   d before the push; +inf without a counted point and on padded rows, NaN where the row's xyz is not finite
"""
import numpy as np

import traj_clearance_ref as C
import traj_rank_ref as R

MARGIN = C.MARGIN
SKIP = C.SKIP
NEAR_TIE = 2e-6          # metres: counted points this close to the float64 minimum are near-tied for an fp32 arg-min
PUSH_SMOOTH = ((1.0, 0.0), (0.5, 0.25), (0.0, 0.5))


def world(x, bounds):
    lo, hi = np.asarray(bounds).astype(np.float64)
    return (np.asarray(x).astype(np.float64) + 1.0) / 2.0 * (hi - lo) + lo


def push_of(p, s, margin, push):
    """u of one waypoint p (3,) against the point s (3,), float64"""
    d = np.sqrt(((p - s) ** 2).sum())
    if not (0.0 < d < margin):
        return np.zeros(3)
    return push * (margin - d) * (p - s) / d


def guide_ref(signals, mask, cond_mask, bounds, scene, scene_mask=None, margin=MARGIN, skip=SKIP, push=1.0, smooth=0.0):
    """-> dict: x (B, G, L, D) float64 after the step (the inputs' stored fp32 values taken exactly), nearest (B, G, L), free, pushed
    (B, G, L) bool, d (B, G, L) = nearest, index (B, G, L) of s* in the kernel's order (-1 without one), u, v (B, G, L, 3) in world
    coordinates, alts {(b, g, i): (k, 3) normalised xyz'} for the pushed rows with k > 1 counted points within NEAR_TIE of the minimum"""
    X = np.asarray(signals).astype(np.float64)
    B, G, L, D = X.shape
    lo, hi = np.asarray(bounds).astype(np.float64)
    valid = np.asarray(mask).reshape(B, L) == 0
    pinned = np.zeros((B, G, L), dtype=bool) if cond_mask is None else np.asarray(cond_mask).reshape(B, G, L, D)[..., 0] != 0
    pts, counted = C.scene_points(scene, scene_mask)
    with np.errstate(invalid="ignore", over="ignore"):
        P = world(X[..., :3], bounds)
    finite = np.isfinite(P).all(-1)
    nearest = np.full((B, G, L), np.inf)
    index = np.full((B, G, L), -1, dtype=np.int64)
    free = np.zeros((B, G, L), dtype=bool)
    u = np.zeros((B, G, L, 3))
    v = np.zeros((B, G, L, 3))
    alts = {}
    for b in range(B):
        where = np.nonzero(counted[b])[0]
        pb = pts[b][where]
        idx = np.nonzero(valid[b])[0]
        n = len(idx)
        scored = idx[skip[0]:max(n - skip[1], 0)]
        free[b][:, scored] = True
        free[b] &= finite[b] & ~pinned[b]
        for g in range(G):
            for i in idx:
                if not finite[b, g, i]:
                    nearest[b, g, i] = np.nan
                    continue
                if not len(pb):
                    continue
                df = P[b, g, i] - pb
                d2 = df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1] + df[:, 2] * df[:, 2]
                k = int(np.argmin(d2))                                   # the first minimum: the lowest index
                nearest[b, g, i], index[b, g, i] = np.sqrt(d2[k]), where[k]
                if free[b, g, i] and push > 0:
                    u[b, g, i] = push_of(P[b, g, i], pb[k], margin, push)
                    near = np.nonzero(np.sqrt(d2) <= nearest[b, g, i] + NEAR_TIE)[0]
                    if len(near) > 1 and 0.0 < nearest[b, g, i] < margin:
                        alts[(b, g, i)] = np.stack([push_of(P[b, g, i], pb[q], margin, push) for q in near])
            if smooth > 0:
                for j in range(1, n - 1):
                    i, ip, inx = idx[j], idx[j - 1], idx[j + 1]
                    if free[b, g, i] and finite[b, g, ip] and finite[b, g, inx]:
                        v[b, g, i] = smooth * ((P[b, g, ip] + P[b, g, inx]) / 2.0 - P[b, g, i])
    out = X.copy()
    scale = 2.0 / (hi - lo)
    out[..., :3] = np.where(free[..., None], X[..., :3] + (u + v) * scale, X[..., :3])
    alts = {key: X[key][:3] + (a + v[key]) * scale for key, a in alts.items()}
    pushed = free & (np.abs(u).sum(-1) > 0)
    return {"x": out, "nearest": nearest, "free": free, "pushed": pushed, "d": nearest, "index": index, "u": u, "v": v, "alts": alts,
            "world": P}


def row_bar(ref, bounds, margin, push, smooth):
    """(B, G, L, 3): 4 x the derived bound of the kernel's fp32 error on x' of a free row.  World coordinates carry about
    e_p = 2^-22 max|coordinate| (the coordinates of the row, its neighbours and the points are all bounded by the bounds box and the
    scene around it: the largest |world coordinate| of the case is taken); the direction (p - s*) / d carries sqrt(3) e_p / d, so
    |err u| <= push sqrt(3) e_p ((margin - d) / d + 1) and |err v| <= 2 smooth e_p; converted with 2 / (hi - lo), plus 2^-23 |x'|."""
    lo, hi = np.asarray(bounds).astype(np.float64)
    P = ref["world"]
    e_p = 2.0 ** -22 * float(np.abs(P[np.isfinite(P)]).max()) if np.isfinite(P).any() else 0.0
    d = ref["d"]
    with np.errstate(invalid="ignore", divide="ignore"):
        eu = np.where(ref["pushed"], push * np.sqrt(3.0) * e_p * ((margin - d) / d + 1.0), 0.0)
    ev = 2.0 * smooth * e_p
    return 4.0 * ((eu + ev)[..., None] * (2.0 / (hi - lo)) + 2.0 ** -23 * np.abs(ref["x"][..., :3]))


def conditions(ref):
    """(near-tied pushed rows, pushed rows, smallest d of a pushed row): the GPU test needs ties <= 2 % and d >= 1e-4 m"""
    n_push = int(ref["pushed"].sum())
    d_min = float(ref["d"][ref["pushed"]].min()) if n_push else np.inf
    return len(ref["alts"]), n_push, d_min


# ------------------------------------------------------------------------------------------------ seeded inputs
def signals_of(poses, bounds):
    """numpy stand-in of pose_to_signal for CPU-side checks: normalised xyz in fp32, then the remaining pose channels padded to D = Dp + 2
    (the rotation channels are not read by the guide step: any values do)"""
    P = np.asarray(poses, dtype=np.float32)
    lo, hi = np.asarray(bounds, dtype=np.float32)
    xyz = ((P[..., :3] - lo) / (hi - lo) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    rest = np.concatenate([P[..., 3:], P[..., 3:5]], -1)
    return np.ascontiguousarray(np.concatenate([xyz, rest], -1), dtype=np.float32)


def make_cond_mask(seed, mask, G, D):
    """the sampler's in-painting pattern (row 0 and every row from the last valid one on) plus 10 % more pinned rows, all D bytes of a
    row alike -> (B G, L, D) uint8"""
    rng = np.random.default_rng(7 * seed + 11)
    mask = np.asarray(mask)
    B, L = mask.shape
    cm = rng.random((B, G, L)) < 0.1
    cm[:, :, 0] = True
    gidx = L - mask.sum(1) - 1
    cm |= (np.arange(L)[None] >= gidx[:, None])[:, None, :]
    return np.ascontiguousarray(np.broadcast_to(cm.reshape(B * G, L, 1), (B * G, L, D)), dtype=np.uint8)


def make_inputs(seed, B, G, L, C_, H, W, D, mask_kind):
    """traj_clearance_ref.make_inputs(seed) with Dp = D - 2 -> poses, mask, bounds, scene, scene_mask, cond_mask"""
    P, mask, _, bounds, scene, scene_mask = C.make_inputs(seed, B, G, L, C_, H, W, D - 2, mask_kind)
    return P, mask, bounds, scene, scene_mask, make_cond_mask(seed, mask, G, D)


def find_seed(B, G, L, C_, H, W, D, mask_kind, with_scene_mask, start=0, tries=1000):
    """the first seed >= start whose case meets the conditions of the GPU test in the restatement (push 1 pushes the most rows)"""
    for seed in range(start, start + tries):
        P, mask, bounds, scene, sm, cm = make_inputs(seed, B, G, L, C_, H, W, D, mask_kind)
        ref = guide_ref(signals_of(P, bounds), mask, cm, bounds, scene, sm if with_scene_mask else None)
        ties, n_push, d_min = conditions(ref)
        if ties <= 0.02 * n_push and d_min >= 1e-4:
            return seed
    return None


MASKS = R.MASKS
