"""Float64 restatement of the body-aware swept clearance (a3d_traj_body_clearance, csrc/traj_body.hip; trajectory.body_clearance,
rank_trajectories(body=...)), the seeded body generator of its tests, the bars of the GPU test and the seed finder for exact ranks.

CPU-only module shared by tests/test_traj_body_cpu.py (the restatement is right) and tests/test_traj_body_gpu.py (the kernel against
it).  Nothing here imports the package under test; scenes and the point-distance term come from tests/traj_clearance_ref.py, poses,
masks and the five-term ranking from tests/traj_rank_ref.py.

Semantics.  poses P (B, G, L, Dp), Dp in {7, 8}, world coordinates, rows [xyz | quaternion (w, x, y, z) | ..]; mask (B, L), non-zero =
padded row, any pattern; scene, scene_mask, "counted point", margin, skip: as traj_clearance_ref.  body: offsets (K, 3) sphere
centres in the tool frame, radii (K,) >= 0, sweep 0 / 1, 1 <= K <= 8.
    R(q)      q^ = q / max(|q|, 1e-10), t = 2 / |q^|^2; columns [1 - t(yy + zz), t(xy + zw), t(xz - yw)], [t(xy - zw), 1 - t(xx + zz),
              t(yz + xw)], [t(xz + yw), t(yz - xw), 1 - t(xx + yy)].  A zero quaternion gives a non-finite R.
    ranks     the valid rows of scene b have ranks j = 0 .. n - 1; row j is scored when skip_head <= j < n - skip_tail
    end row   e(j) = j + 1 when sweep is set and j + 1 < n - skip_tail, else j: one rule for every valid row
    sphere k of row j   a = p_j + R(q_j) o_k, c = p_e + R(q_e) o_k; dist_k = min over the counted points s and t in [0, 1] of
              |s - (a + t (c - a))|_2
    nearest[b,g,i_j]   min_k (dist_k - r_k), signed; +inf without a counted point and on padded rows; NaN where a or c of any sphere
              of the row is not finite
    clearance[b,g]   mean over the scored rows of max(0, margin - nearest) / margin, not clamped above; 0 without a scored row; NaN
              as soon as a scored row is NaN
    score     the five-term sum of traj_rank_ref, then + w_clearance * clearance, added last; +inf where that is not finite
"""
import numpy as np

import traj_clearance_ref as C
import traj_rank_ref as R

MAX_SPHERES = 8
# Roundings of the fp32 expression on the way to one `nearest`, each taken at the scale of the case's largest coordinate:
#   q^            4 squares, 3 adds, the root, the division                      9
#   t             4 squares, 3 adds, the division                                8
#   an entry of R 2 products, 1 add / subtract, the product with t, 1 - ..       5
#   R o           3 products, 2 adds                                             5
#   p + R o       1                                                              1      -> a: 28, c: 28 more
#   d = c - a     1;  |d|^2: 3;  inv: 1                                          5
#   u = s - a     1;  the dot product: 3;  times inv: 1                          5
#   w             one fmaf per coordinate                                        1
#   d^2           3;  the root: 1;  minus r: 1                                   5
ROUNDINGS = 28 + 28 + 5 + 5 + 1 + 5


def rotation(q):
    """(.., 4) quaternions (w, x, y, z) -> (.., 3, 3) float64, R[.., row, column]"""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-10)
        w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
        t = 2.0 / (w * w + x * x + y * y + z * z)
        cols = [[1.0 - t * (y * y + z * z), t * (x * y + z * w), t * (x * z - y * w)],
                [t * (x * y - z * w), 1.0 - t * (x * x + z * z), t * (y * z + x * w)],
                [t * (x * z + y * w), t * (y * z - x * w), 1.0 - t * (x * x + y * y)]]
    return np.stack([np.stack(c, -1) for c in cols], -1)


def end_rows(mask_row, sweep, skip):
    """one scene's mask row (L,) -> idx (the valid rows in rank order), end (the end ROW of each of them), scored (bool per rank)"""
    idx = np.nonzero(np.asarray(mask_row) == 0)[0]
    n = len(idx)
    j = np.arange(n)
    step = (j + 1 < n - skip[1]) if sweep else np.zeros(n, dtype=bool)
    end = idx[np.where(step, np.minimum(j + 1, max(n - 1, 0)), j)] if n else idx
    scored = (j >= skip[0]) & (j < n - skip[1])
    return idx, end, scored


def segment_dist(a, c, pts):
    """a, c (.., 3) segment ends, pts (M, 3) -> (..) the distance of each segment to the nearest point; +inf when M = 0"""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if not len(pts):
        return np.full(a.shape[:-1], np.inf)
    d = c - a
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dd = (d * d).sum(-1)
        inv = np.where(dd == 0.0, 0.0, 1.0 / np.where(dd == 0.0, 1.0, dd))
        u = pts - a[..., None, :]                                          # (.., M, 3)
        t = np.clip((u * d[..., None, :]).sum(-1) * inv[..., None], 0.0, 1.0)
        w = u - t[..., None] * d[..., None, :]
        d2 = (w * w).sum(-1)
        d2 = np.where(np.isnan(d2), np.inf, d2)                            # a non-finite segment: its row is NaN, decided by the caller
        return np.sqrt(d2.min(-1))


def body_ref(poses, mask, scene, offsets, radii, sweep, scene_mask=None, margin=C.MARGIN, skip=C.SKIP):
    """-> nearest (B, G, L), clearance (B, G); float64 throughout, the inputs' stored (fp32) values taken exactly"""
    P = np.asarray(poses).astype(np.float64)
    B, G, L = P.shape[:3]
    o = np.asarray(offsets).astype(np.float64).reshape(-1, 3)
    r = np.asarray(radii).astype(np.float64).reshape(-1)
    assert 1 <= len(o) <= MAX_SPHERES and r.shape == (len(o),)
    pts, counted = C.scene_points(scene, scene_mask)
    nearest = np.full((B, G, L), np.inf)
    clear = np.zeros((B, G))
    for b in range(B):
        idx, end, scored = end_rows(np.asarray(mask).reshape(B, L)[b], sweep, skip)
        if not len(idx):
            continue
        pb = pts[b][counted[b]]
        with np.errstate(invalid="ignore", over="ignore"):
            centre = P[b, :, :, None, :3] + np.einsum("glij,kj->glki", rotation(P[b, :, :, 3:7]), o)      # (G, L, K, 3)
        for g in range(G):
            a, c = centre[g, idx], centre[g, end]                          # (n, K, 3)
            with np.errstate(invalid="ignore"):
                near = (segment_dist(a, c, pb) - r).min(-1)                # (n,)
            bad = ~(np.isfinite(a).all((-1, -2)) & np.isfinite(c).all((-1, -2)))
            nearest[b, g, idx] = np.where(bad, np.nan, near)
        if scored.any():
            nr = nearest[b][:, idx[scored]]
            with np.errstate(invalid="ignore"):
                h = np.maximum(0.0, margin - nr) / margin
            clear[b] = np.where(np.isnan(nr), np.nan, h).mean(-1)
    return nearest, clear


def body_rank_ref(poses, mask, goal, bounds, select, scene, offsets, radii, sweep, scene_mask=None, margin=C.MARGIN, skip=C.SKIP,
                  rot_weight=1.0):
    """traj_rank_ref.rank_ref with the body clearance term added last -> its dict plus "clearance" and "nearest" """
    select = {C.TERM: 1.0} if select == "clear" else select
    five = {k: v for k, v in select.items() if k != C.TERM} if isinstance(select, dict) else select
    wc = float(select.get(C.TERM, 0.0)) if isinstance(select, dict) else 0.0
    ref = R.rank_ref(poses, mask, goal, bounds, five, rot_weight)
    nearest, clear = body_ref(poses, mask, scene, offsets, radii, sweep, scene_mask, margin, skip)
    with np.errstate(invalid="ignore", over="ignore"):
        scores = (ref["terms"] * R.weights_of(five)).sum(-1)
        if wc != 0.0:
            scores = scores + wc * clear
    scores = np.where(np.isfinite(scores), scores, np.inf)
    order = np.argsort(scores, axis=1, kind="stable").astype(np.int64)
    best = order[:, 0].copy()
    Pn = np.asarray(poses)
    return {"best": best, "order": order, "scores": scores, "terms": ref["terms"], "selected": Pn[np.arange(Pn.shape[0]), best],
            "clearance": clear, "nearest": nearest}


# ------------------------------------------------------------------------------------------------ bars
def largest_coordinate(poses, scene, offsets):
    """the scale of a case: the largest finite |coordinate| of the waypoints, the scene points and the offsets"""
    vals = [np.abs(np.asarray(x, dtype=np.float64)).ravel() for x in (np.asarray(poses)[..., :3], scene, offsets)]
    v = np.concatenate(vals)
    v = v[np.isfinite(v)]
    return float(v.max()) if len(v) else 1.0


def nearest_bar(poses, scene, offsets):
    """ABSOLUTE bar on a finite `nearest` (metres): 5 x the roundings of the expression x 2^-24 x the case's largest |coordinate|"""
    return 5.0 * ROUNDINGS * 2.0 ** -24 * largest_coordinate(poses, scene, offsets)


# ------------------------------------------------------------------------------------------------ seeded inputs
def make_body(seed, K):
    """offsets (K, 3) fp32 within +-8 cm, radii (K,) fp32 within 0 .. 3 cm"""
    rng = np.random.default_rng(7919 * seed + 104729 * K + 13)
    return rng.uniform(-0.08, 0.08, (K, 3)).astype(np.float32), rng.uniform(0.0, 0.03, (K,)).astype(np.float32)


TRIVIAL = (np.zeros((1, 3), dtype=np.float32), np.zeros((1,), dtype=np.float32), 0)       # the tool point itself


def make_inputs(seed, B, G, L, K, C_, H, W, Dp, mask_kind):
    """traj_clearance_ref.make_inputs(seed) and a body -> poses, mask, goal, bounds, scene, scene_mask, offsets, radii"""
    return C.make_inputs(seed, B, G, L, C_, H, W, Dp, mask_kind) + make_body(seed, K)


def find_seed(B, G, L, K, C_, H, W, Dp, mask_kind, with_scene_mask, sweep, select=None, start=0, tries=100000):
    """the first seed >= start whose case meets traj_rank_ref.gaps_ok in the float64 restatement with the body term weighed (how the
    seed table of the GPU test was made)"""
    select = C.RULE if select is None else select
    for seed in range(start, start + tries):
        P, mask, goal, bounds, scene, scene_mask, o, r = make_inputs(seed, B, G, L, K, C_, H, W, Dp, mask_kind)
        ref = body_rank_ref(P, mask, goal, bounds, select, scene, o, r, sweep, scene_mask if with_scene_mask else None)
        if R.gaps_ok(ref["scores"]):
            return seed
    return None
