"""Float64 restatement of the scene clearance term (a3d_traj_clearance, csrc/traj_clearance.hip; diffusion.trajectory_clearance,
rank_trajectories(select={"clearance": w})), the seeded scene generator of its tests and the seed finder for exact ranks.

CPU-only module shared by tests/test_traj_clearance_cpu.py (the restatement is right) and tests/test_traj_clearance_gpu.py (the kernel
against it).  Nothing here imports the package under test; poses, masks and the five-term ranking come from tests/traj_rank_ref.py.

Semantics.  poses P (B, G, L, Dp), Dp in {7, 8}, world coordinates, only xyz is read; mask (B, L), non-zero = padded row, any pattern.
scene S (B, C, 3, H, W) fp32, channel-planar per camera: point p of camera c is S[b, c, :, p]; N = C H W points per scene.
scene_mask (B, C, H, W), non-zero = ignore the point.
    counted   a point that is not masked and whose three coordinates are finite
    nearest[b,g,i]   min over the counted points of scene b of |p_{b,g,i} - s|_2 = sqrt(min(dx dx + dy dy + dz dz));
                     +inf when no point is counted; +inf (not computed) on padded rows; NaN where the row's xyz is not finite
    scored    j = rank of a valid row among the n_b valid rows of its scene; scored: skip_head <= j < n_b - skip_tail
    clearance[b,g]   mean over the scored rows of max(0, margin - nearest) / margin, in [0, 1]; 0 without a scored row; NaN as soon
                     as a scored row's nearest is NaN
    score     the five-term sum of traj_rank_ref, then + w_clearance * clearance, added last; +inf where that is not finite
"""
import numpy as np

import traj_rank_ref as R

MARGIN = 0.05
SKIP = (1, 1)
TERM = "clearance"
RULE = {"consensus": 1.0, TERM: 5.0}              # the rule of the ranking tests


def scene_points(scene, scene_mask=None):
    """(B, C, 3, H, W) -> points (B, N, 3) float64 in the kernel's order, counted (B, N) bool"""
    S = np.asarray(scene)
    B, C = S.shape[:2]
    pts = S.reshape(B, C, 3, -1).transpose(0, 1, 3, 2).reshape(B, -1, 3).astype(np.float64)
    counted = np.isfinite(pts).all(-1)
    if scene_mask is not None:
        counted &= np.asarray(scene_mask).reshape(B, -1) == 0
    return pts, counted


def clearance_ref(poses, mask, scene, scene_mask=None, margin=MARGIN, skip=SKIP):
    """-> nearest (B, G, L), clearance (B, G); float64 throughout, the inputs' stored (fp32) values taken exactly"""
    P = np.asarray(poses)[..., :3].astype(np.float64)
    B, G, L = P.shape[:3]
    valid = np.asarray(mask).reshape(B, L) == 0
    pts, counted = scene_points(scene, scene_mask)
    nearest = np.full((B, G, L), np.inf)
    clear = np.zeros((B, G))
    for b in range(B):
        pb = pts[b][counted[b]]                                          # (M, 3)
        idx = np.nonzero(valid[b])[0]
        for i in idx:
            rows = P[b, :, i]                                            # (G, 3)
            if len(pb):
                d = rows[:, None, :] - pb[None]
                with np.errstate(invalid="ignore", over="ignore"):
                    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
                    nearest[b, :, i] = np.sqrt(d2.min(-1))
            nearest[b, ~np.isfinite(rows).all(-1), i] = np.nan
        n = len(idx)
        scored = idx[skip[0]:max(n - skip[1], 0)]                        # skip_head <= j < n - skip_tail
        if len(scored):
            with np.errstate(invalid="ignore"):
                h = np.maximum(0.0, margin - nearest[b][:, scored]) / margin
            h = np.where(np.isnan(nearest[b][:, scored]), np.nan, h)      # np.maximum propagates NaN already; said out loud
            clear[b] = h.mean(-1)
    return nearest, clear


def scene_rank_ref(poses, mask, goal, bounds, select, scene, scene_mask=None, margin=MARGIN, skip=SKIP, rot_weight=1.0):
    """traj_rank_ref.rank_ref with the clearance term added last -> its dict plus "clearance" and "nearest" """
    select = {TERM: 1.0} if select == "clear" else select
    five = {k: v for k, v in select.items() if k != TERM} if isinstance(select, dict) else select
    wc = float(select.get(TERM, 0.0)) if isinstance(select, dict) else 0.0
    ref = R.rank_ref(poses, mask, goal, bounds, five, rot_weight)
    nearest, clear = clearance_ref(poses, mask, scene, scene_mask, margin, skip)
    with np.errstate(invalid="ignore", over="ignore"):
        scores = (ref["terms"] * R.weights_of(five)).sum(-1)
        if wc != 0.0:
            scores = scores + wc * clear
    scores = np.where(np.isfinite(scores), scores, np.inf)
    order = np.argsort(scores, axis=1, kind="stable").astype(np.int64)
    best = order[:, 0].copy()
    P = np.asarray(poses)
    return {"best": best, "order": order, "scores": scores, "terms": ref["terms"], "selected": P[np.arange(P.shape[0]), best],
            "clearance": clear, "nearest": nearest}


# ------------------------------------------------------------------------------------------------ seeded inputs
def make_scene(seed, B, C, H, W, poses=None, masked=0.1, broken=0.05):
    """A synthetic tabletop around the trajectories: half of the points on a table plane 2 cm below the lowest waypoint, the rest on
    the faces of four boxes (half sizes 1 .. 5 cm) set about 3 cm from waypoints of the scene, so that a share of the rows lies
    inside the default margin.  `masked` of the points are flagged in scene_mask, `broken` of them get a NaN or an infinite
    coordinate.  poses None: the anchors are drawn inside traj_rank_ref.BOUNDS.
    -> scene (B, C, 3, H, W) fp32, scene_mask (B, C, H, W) bool"""
    rng = np.random.default_rng(100003 * seed + 7919)
    N = C * H * W
    lo, hi = R.BOUNDS.astype(np.float64)
    pts = np.zeros((B, N, 3))
    for b in range(B):
        anchors = None if poses is None else np.asarray(poses)[b, ..., :3].reshape(-1, 3).astype(np.float64)
        if anchors is not None:
            anchors = anchors[np.isfinite(anchors).all(-1)]
        if anchors is None or not len(anchors):
            anchors = lo + rng.random((16, 3)) * (hi - lo)
        n_plane = N // 2
        a_lo, a_hi = anchors.min(0), anchors.max(0)
        xy = a_lo[:2] - 0.1 + rng.random((n_plane, 2)) * (a_hi[:2] - a_lo[:2] + 0.2)
        pts[b, :n_plane] = np.concatenate([xy, a_lo[2] - 0.02 + 0.001 * rng.normal(0.0, 1.0, (n_plane, 1))], -1)
        n_box = N - n_plane
        centre = anchors[rng.integers(0, len(anchors), 4)] + rng.normal(0.0, 0.03, (4, 3))
        half = 0.01 + 0.04 * rng.random((4, 3))
        which = rng.integers(0, 4, n_box)
        u = rng.uniform(-1.0, 1.0, (n_box, 3))
        face = rng.integers(0, 3, n_box)
        u[np.arange(n_box), face] = rng.choice([-1.0, 1.0], n_box)        # onto one of the six faces
        pts[b, n_plane:] = centre[which] + u * half[which]
    bad = rng.random((B, N)) < broken
    kind = rng.integers(0, 3, (B, N))
    value = rng.choice([np.nan, np.inf, -np.inf], (B, N))
    for k in range(3):
        pts[..., k] = np.where(bad & (kind == k), value, pts[..., k])
    order = np.stack([rng.permutation(N) for _ in range(B)])              # plane and boxes mixed over cameras and chunks
    pts = np.take_along_axis(pts, order[..., None], 1)
    scene = np.ascontiguousarray(pts.reshape(B, C, H * W, 3).transpose(0, 1, 3, 2).reshape(B, C, 3, H, W), dtype=np.float32)
    scene_mask = (rng.random((B, C, H, W)) < masked)
    return scene, scene_mask


def make_inputs(seed, B, G, L, C, H, W, Dp, mask_kind):
    """traj_rank_ref.make_case(seed) and the scene built around it -> poses, mask, goal, bounds, scene, scene_mask"""
    P, mask, goal, bounds = R.make_case(seed, B, G, L, Dp, mask_kind)
    scene, scene_mask = make_scene(seed, B, C, H, W, poses=P)
    return P, mask, goal, bounds, scene, scene_mask


def find_seed(B, G, L, C, H, W, Dp, mask_kind, with_scene_mask, select=None, start=0, tries=100000):
    """the first seed >= start whose case meets traj_rank_ref.gaps_ok in the float64 restatement with the clearance term weighed (how
    the seed table of the GPU test was made)"""
    select = RULE if select is None else select
    for seed in range(start, start + tries):
        P, mask, goal, bounds, scene, scene_mask = make_inputs(seed, B, G, L, C, H, W, Dp, mask_kind)
        ref = scene_rank_ref(P, mask, goal, bounds, select, scene, scene_mask if with_scene_mask else None)
        if R.gaps_ok(ref["scores"]):
            return seed
    return None
