"""Float64 restatement of the candidate ranking (a3d_traj_rank, csrc/traj_rank.hip; diffusion.rank_trajectories), the seeded
input generator of its tests and the gap condition under which `best` / `order` must be reproduced exactly.

CPU-only module shared by tests/test_traj_rank_cpu.py (the restatement is right) and tests/test_traj_rank_gpu.py (the kernel against
it).  Nothing here imports the package under test.

Semantics.  poses P (B, G, L, Dp), Dp in {7, 8}: xyz | quaternion | optional gripper opening (never scored); mask (B, L), non-zero =
padded row, any pattern; a row is valid where its mask entry is 0, n_b = valid rows of scene b.  Quaternions are divided by
max(|q|, 1e-10).
    rho(q, r) = 1 - <q, r>^2   (sin^2 of half the angle; sign-invariant), evaluated as  sum_{i<j} (q_i r_j - q_j r_i)^2:
                Lagrange's identity |q|^2 |r|^2 - <q, r>^2 = sum_{i<j} (q_i r_j - q_j r_i)^2 with |q| = |r| = 1.  The minor form
                has no cancellation against 1 and is an exact 0 for q = r, which the consensus sum needs for its h = g entry.
    d(a, b)   = |p_a - p_b|_2 + rot_weight * rho(q_a, q_b)
    consensus = 1 / max(G - 1, 1) * sum_{h = 0 .. G - 1} 1 / max(n_b, 1) * sum_{valid i} d(P[b,g,i], P[b,h,i])     (h = g included: 0)
                Non-finite poses: a pair sum (g, h), h != g, that is not finite is left out of candidate g's sum, so one NaN
                candidate does not turn every score of its scene into NaN; its own entry h = g is NaN and keeps it last.  With
                finite inputs nothing is left out.
    goal      = d(P[b,g,i*], goal_b), i* the highest valid row index; 0 when n_b = 0 or no goal is given
    smooth    = mean over i with rows i - 1, i, i + 1 all valid of |(p_{i+1} - p_i) - (p_i - p_{i-1})|^2; 0 without such a triple
    length    = sum over i with rows i, i + 1 both valid of |p_{i+1} - p_i|_2
    bounds    = (valid rows with any coordinate outside [lo, hi]) / max(n_b, 1); 0 when no bounds are given
    score     = sum_k w_k term_k, +inf where that is not finite
    order[b]  = stable ascending ranking: rank of g = #{h : s_h < s_g or (s_h = s_g and h < g)};  best[b] = order[b][0]
    selected[b] = P[b, best[b]], all Dp channels, padded rows included
"""
import numpy as np

TERMS = ("consensus", "goal", "smooth", "length", "bounds")
PRESETS = {"consensus": "consensus", "goal": "goal", "smooth": "smooth", "shortest": "length"}
GAP = 1e-3          # smallest adjacent gap of a scene's sorted scores, relative to the scene's largest score


def weights_of(select):
    """the five weights of a preset name or a {term: weight} dict, in TERMS order"""
    if isinstance(select, str):
        select = {PRESETS[select]: 1.0}
    return np.array([float(select.get(k, 0.0)) for k in TERMS], dtype=np.float64)


def unit_quat(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), 1e-10)


def rho(q, r):
    """1 - <q, r>^2 of unit quaternions by the 2x2 minors (module docstring); broadcasts over leading axes"""
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    out = 0.0
    for i in range(3):
        for j in range(i + 1, 4):
            m = q[..., i] * r[..., j] - q[..., j] * r[..., i]
            out = out + m * m
    return out


def pose_dist(a, b, rot_weight):
    """d of rows [xyz | UNIT quaternion]; broadcasts"""
    dp = a[..., :3] - b[..., :3]
    return np.sqrt((dp * dp).sum(-1)) + rot_weight * rho(a[..., 3:7], b[..., 3:7])


def rank_ref(poses, mask, goal=None, bounds=None, select="consensus", rot_weight=1.0):
    """-> dict(best (B,), order (B, G), scores (B, G), terms (B, G, 5), selected (B, L, Dp)); float64 throughout, the inputs'
    stored (fp32) values taken exactly.  goal: (B, >= 7) or None; bounds: (2, 3) or None."""
    P = np.asarray(poses)
    B, G, L, Dp = P.shape
    X = np.concatenate([P[..., :3].astype(np.float64), unit_quat(P[..., 3:7])], -1)          # (B, G, L, 7)
    valid = np.asarray(mask).reshape(B, L) == 0
    w = weights_of(select)
    rw = float(rot_weight)
    terms = np.zeros((B, G, 5), dtype=np.float64)
    for b in range(B):
        v = valid[b]
        n = int(v.sum())
        idx = np.nonzero(v)[0]
        Xv = X[b][:, idx]                                                                     # (G, n, 7)
        # consensus: the sum over h in index order
        cons = np.zeros(G)
        for h in range(G):
            with np.errstate(invalid="ignore", over="ignore"):
                dh = pose_dist(Xv, Xv[h][None], rw).sum(-1) / max(n, 1)
            # a non-finite candidate h is left out of the OTHER candidates' sums; its own entry (h = g) keeps its NaN
            cons = cons + np.where(np.isfinite(dh) | (np.arange(G) == h), dh, 0.0)
        terms[b, :, 0] = cons / max(G - 1, 1)
        if goal is not None and n > 0:
            gl = np.asarray(goal)[b].astype(np.float64)
            grow = np.concatenate([gl[:3], unit_quat(gl[3:7])])
            terms[b, :, 1] = pose_dist(X[b][:, idx[-1]], grow[None], rw)
        p = X[b][..., :3]
        pair = v[:-1] & v[1:] if L > 1 else np.zeros(0, dtype=bool)                           # rows i, i + 1
        step = p[:, 1:] - p[:, :-1]                                                           # (G, L - 1, 3)
        if pair.any():
            terms[b, :, 3] = np.sqrt((step * step).sum(-1))[:, pair].sum(-1)
        if L > 2:
            tri = v[:-2] & v[1:-1] & v[2:]                                                    # rows i - 1, i, i + 1
            if tri.any():
                acc = step[:, 1:] - step[:, :-1]
                terms[b, :, 2] = (acc * acc).sum(-1)[:, tri].mean(-1)
        if bounds is not None:
            lo, hi = np.asarray(bounds, dtype=np.float64)
            out = ((p < lo) | (p > hi)).any(-1)                                               # (G, L)
            terms[b, :, 4] = out[:, v].sum(-1) / max(n, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        scores = (terms * w).sum(-1)
    scores = np.where(np.isfinite(scores), scores, np.inf)
    order = np.argsort(scores, axis=1, kind="stable").astype(np.int64)
    best = order[:, 0].copy()
    selected = P[np.arange(B), best]
    return {"best": best, "order": order, "scores": scores, "terms": terms, "selected": selected}


def structural_tie(G, select):
    """d is symmetric, so with G = 2 the consensus term is the SAME number for both candidates: D[0][1] = D[1][0], bit for bit in the
    restatement and in any arithmetic that treats its two arguments alike.  No input separates them; the index decides."""
    return G == 2 and isinstance(select, str) and select == "consensus"


def gaps_ok(scores, gap=GAP, exact_ties=False):
    """every adjacent gap of every scene's sorted scores is at least `gap` of that scene's largest score (all must be finite).
    exact_ties (structural_tie cases only): a gap may instead be exactly 0."""
    s = np.sort(np.asarray(scores, dtype=np.float64), axis=1)
    if not np.isfinite(s).all():
        return False
    if s.shape[1] == 1:
        return True
    d = np.diff(s, axis=1)
    ok = d >= gap * np.abs(s).max(1, keepdims=True)
    if exact_ties:
        ok = ok | (d == 0.0)
    return bool(ok.all())


# ------------------------------------------------------------------------------------------------ seeded inputs
BOUNDS = np.array([[-0.3, -0.5, 0.6], [0.7, 0.5, 1.6]], dtype=np.float32)
MASKS = ("none", "suffix", "scattered", "padded_scene")
MIXED = {"consensus": 1.0, "goal": 0.5, "smooth": 20.0, "length": 0.3, "bounds": 0.2}
SELECTS = ("consensus", "goal", "smooth", "shortest", MIXED)


def make_mask(rng, B, L, kind):
    m = np.zeros((B, L), dtype=bool)
    if kind == "suffix":
        for b in range(B):
            m[b, L - int(rng.integers(0, max(L // 2, 1) + 1)):] = L > 1
    elif kind == "scattered":
        m = rng.random((B, L)) < 0.3
        m[:, 0] = False                                            # at least one valid row per scene
    elif kind == "padded_scene":
        m = rng.random((B, L)) < 0.2
        m[B - 1] = True                                            # the last scene has no valid row at all
    return m


def make_case(seed, B, G, L, Dp, mask_kind):
    """Seeded random walks inside BOUNDS (step ~ 0.02) with random rotations; candidate g deviates from the scene's base walk by an
    amplitude of its own (G <= 8) or walks a scaled copy of it from an offset start (G > 8), a few rows are pushed outside the bounds, quaternions are stored un-normalised (either sign).
    -> poses (B, G, L, Dp) fp32, mask (B, L) bool, goal (B, 8) fp32, bounds (2, 3) fp32"""
    rng = np.random.default_rng(seed)
    lo, hi = BOUNDS.astype(np.float64)
    start = lo + (0.3 + 0.4 * rng.random((B, 1, 1, 3))) * (hi - lo)
    if G > 8:
        start[..., 2] = lo[2] + 0.93 * (hi[2] - lo[2])
    base_step = rng.normal(0.0, 0.02 / np.sqrt(3.0), (B, 1, L, 3))
    amp = np.stack([(rng.permutation(G) + 1.0) / G for _ in range(B)]).reshape(B, G, 1, 1)
    if G > 8:
        # many candidates: path length and smoothness of independent walks crowd into a band far narrower than G gaps of 1e-3, so
        # candidate g walks the scene's base steps scaled by 0.5 .. 1.5 in an order of its own (step 0.01 .. 0.03), 0.03 % jitter
        rank = np.stack([rng.permutation(G) for _ in range(B)]).reshape(B, G, 1, 1)
        step = (0.5 + rank / G) * base_step * (1.0 + 0.0003 * rng.normal(0.0, 1.0, (B, G, L, 1)))
    else:
        step = base_step + amp * rng.normal(0.0, 0.012, (B, G, L, 3))
    pos = start + 0.08 * amp * rng.normal(0.0, 1.0, (B, G, 1, 3)) + np.cumsum(step, axis=2)
    # rows outside the bounds: scattered rows pushed 1.5 up (G <= 8); with G > 8 the walks start just below the upper z bound and
    # cross it on their own (a far row would add the same large jump to the path length, the goal distance and the consensus of
    # every candidate that has one, and crowd the other scores together relative to the largest)
    outside = rng.random((B, G, L)) < 0.08 if G <= 8 else np.zeros((B, G, L), dtype=bool)
    pos = np.where(outside[..., None], pos + np.array([0.0, 0.0, 1.5]), pos)
    qbase = rng.normal(0.0, 1.0, (B, 1, L, 4))
    quat = unit_quat(qbase) + 0.7 * amp * rng.normal(0.0, 1.0, (B, G, L, 4))
    quat = unit_quat(quat) * rng.uniform(0.5, 2.0, (B, G, L, 1)) * rng.choice([-1.0, 1.0], (B, G, L, 1))
    P = np.concatenate([pos, quat] + ([rng.random((B, G, L, 1))] if Dp == 8 else []), -1).astype(np.float32)
    mask = make_mask(rng, B, L, mask_kind)
    goal = np.concatenate([pos[:, 0, -1] + rng.normal(0.0, 0.05, (B, 3)), rng.normal(0.0, 1.0, (B, 4)), rng.random((B, 1))],
                          -1).astype(np.float32)
    return P, mask, goal, BOUNDS.copy()


def find_seed(B, G, L, Dp, mask_kind, select, start=0, tries=100000, rot_weight=1.0):
    """the first seed >= start whose case meets gaps_ok in the float64 restatement (how the seed tables of the GPU test were made)"""
    for seed in range(start, start + tries):
        P, mask, goal, bounds = make_case(seed, B, G, L, Dp, mask_kind)
        if gaps_ok(rank_ref(P, mask, goal, bounds, select, rot_weight)["scores"], exact_ties=structural_tie(G, select)):
            return seed
    return None
