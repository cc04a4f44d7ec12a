"""GPU tests of the scene clearance term: the kernel (a3d_traj_clearance) against the float64 restatement of
tests/traj_clearance_ref.py, the ranking with the term weighed (a3d_traj_rank_extra), chunking and determinism, the mechanics of the
entries (guard bands, NULL outputs, the scene read in place, the (B, N, 3) form, graph capture) and the integration into
rank_trajectories, compute_trajectory(select={"clearance": w}) and Actioner.predict.

Bars.  `nearest`: 2e-6 relative where finite -- the differences of fp32 inputs, three squares, two adds and one square root are about
6 roundings of 2^-24 = 3.6e-7, the bar is about 5 times that; +inf and NaN positions exactly.  `clearance`: 5e-6 absolute -- the
same error through the hinge, divided by the margin, on values in [0, 1], plus the rounding of the mean.  `scores`: 5e-5 of the
largest score of the call, the bar of tests/test_traj_rank_gpu.py.  `best` and `order`: EXACTLY the restatement's, under the
condition of that file, asserted on the restatement first: adjacent float64 scores of a scene differ by at least 1e-3 of the scene's
largest.  The seeds below were found on the CPU (traj_clearance_ref.find_seed); no case is skipped."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import traj_clearance_ref as C  # noqa: E402
import traj_rank_ref as R  # noqa: E402
from test_actioner_gpu import candidate_noise, make_keypose, make_planner, observation, set_rng, by_hand  # noqa: E402

pytestmark = pytest.mark.gpu
NEAR_RTOL = 2e-6
CLEAR_ATOL = 5e-6
SCORE_TOL = 5e-5
GUARD = 64
POISON = -12345.5

SHAPES = [(1, 1, 1, 1, 1, 1), (2, 3, 5, 1, 3, 7), (2, 4, 17, 3, 16, 16), (1, 8, 50, 2, 64, 64), (1, 64, 16, 1, 33, 31),
          (2, 2, 100, 4, 32, 32)]
# (B, G, L, C, H, W) -> mask kind -> seeds for (Dp 7, Dp 7 + scene_mask, Dp 8, Dp 8 + scene_mask); 0 where not listed
SEEDS = {(1, 64, 16, 1, 33, 31): {"none": (113, 93, 113, 93), "suffix": (141, 148, 141, 54), "scattered": (163, 163, 241, 624)}}


def seed_of(shape, mask_kind, Dp, with_mask):
    return SEEDS.get(shape, {}).get(mask_kind, (0,) * 4)[2 * (Dp == 8) + int(with_mask)]


@functools.lru_cache(maxsize=None)
def case(shape, mask_kind, Dp, with_mask):
    """inputs and restatement of one case, computed once and left unchanged -> (numpy inputs, ref dict)"""
    P, mask, goal, bounds, S, sm = C.make_inputs(seed_of(shape, mask_kind, Dp, with_mask), *shape, Dp, mask_kind)
    sm = sm if with_mask else None
    ref = C.scene_rank_ref(P, mask, goal, bounds, C.RULE, S, sm)
    for a in (P, mask, goal, bounds, S) + ((sm,) if with_mask else ()):
        a.setflags(write=False)
    return (P, mask, goal, bounds, S, sm), ref


def t(x, dev, dtype=None):
    """a numpy array as a contiguous device tensor (the raw entries read memory, not strides)"""
    return None if x is None else torch.from_numpy(np.array(x, dtype=dtype, order="C")).to(dev).contiguous()


# ------------------------------------------------------------------------------------------------ calling the entries
def guarded(n, dev, dtype=torch.float32):
    whole = torch.full((n + 2 * GUARD,), -7 if dtype == torch.int32 else POISON, device=dev, dtype=dtype)
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    want = -7 if whole.dtype == torch.int32 else POISON
    return bool((whole[:GUARD] == want).all()) and bool((whole[GUARD + n:] == want).all())


def raw_clearance(a3d, P, mask_u8, S, sm_u8, n_chunks=0, margin=C.MARGIN, skip=C.SKIP, want_nearest=True):
    """a3d_traj_clearance on guarded buffers (workspace included) -> nearest (B, G, L) or None, clearance (B, G), guards ok"""
    B, G, L, Dp = P.shape
    n_cam, n_pix = S.shape[1], S.shape[3] * S.shape[4]
    n_ws = a3d.lib.load().a3d_traj_clearance_ws_floats(B, G, L, n_cam * n_pix, n_chunks)
    assert n_ws >= max(n_chunks, 1) * B * G * L + B * L
    bufs = {"nearest": guarded(B * G * L, P.device), "clearance": guarded(B * G, P.device), "ws": guarded(n_ws, P.device)}
    a3d.lib.call("a3d_traj_clearance", P.data_ptr(), mask_u8.data_ptr(), S.data_ptr(), None if sm_u8 is None else sm_u8.data_ptr(),
                 n_cam, n_pix, float(margin), int(skip[0]), int(skip[1]), bufs["nearest"][1].data_ptr() if want_nearest else None,
                 bufs["clearance"][1].data_ptr(), bufs["ws"][1].data_ptr(), n_chunks, B, G, L, Dp, a3d.lib.stream())
    torch.cuda.synchronize()
    ok = all(guards_intact(w, v.numel()) for w, v in bufs.values())
    if not want_nearest:
        ok = ok and bool((bufs["nearest"][1] == POISON).all())
    return (bufs["nearest"][1].view(B, G, L) if want_nearest else None), bufs["clearance"][1].view(B, G), ok


def raw_rank(a3d, entry, P, mask_u8, goal, bounds, w, rw, tail=()):
    B, G, L, Dp = P.shape
    dev = P.device
    sizes = {"best": (B, torch.int32), "order": (B * G, torch.int32), "scores": (B * G, torch.float32),
             "terms": (B * G * 5, torch.float32), "selected": (B * L * Dp, torch.float32)}
    buf = {k: guarded(n, dev, dt) for k, (n, dt) in sizes.items()}
    a3d.lib.call(entry, P.data_ptr(), mask_u8.data_ptr(), goal.data_ptr(), goal.shape[1], bounds.data_ptr(), *[float(x) for x in w],
                 float(rw), *[buf[k][1].data_ptr() for k in ("best", "order", "scores", "terms", "selected")], B, G, L, Dp, *tail,
                 a3d.lib.stream())
    torch.cuda.synchronize()
    shapes = {"best": (B,), "order": (B, G), "scores": (B, G), "terms": (B, G, 5), "selected": (B, L, Dp)}
    out = {k: v[1].view(shapes[k]) for k, v in buf.items()}
    out["_ok"] = all(guards_intact(v[0], sizes[k][0]) for k, v in buf.items())
    return out


def check_nearest(got, ref, name):
    got = got.cpu().numpy().astype(np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)), name + ": +inf positions"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name + ": NaN positions"
    err = float((np.abs(got[fin] - ref[fin]) / ref[fin]).max()) if fin.any() and (ref[fin] > 0).all() else 0.0
    if fin.any() and not (ref[fin] > 0).all():
        err = float(np.abs(got[fin] - ref[fin]).max())                 # an exact hit: absolute
    return err


# ------------------------------------------------------------------------------------------------ 1: against the restatement
@pytest.mark.parametrize("Dp", [7, 8])
@pytest.mark.parametrize("with_mask", [False, True], ids=["all-points", "scene-mask"])
@pytest.mark.parametrize("mask_kind", R.MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_float64_restatement(a3d, dev, shape, mask_kind, with_mask, Dp):
    (P, mask, goal, bounds, S, sm), ref = case(shape, mask_kind, Dp, with_mask)
    name = "traj_clearance %s %s Dp%d %s" % ("x".join(map(str, shape)), mask_kind, Dp, "scene-mask" if with_mask else "all-points")
    assert R.gaps_ok(ref["scores"]), name                              # the condition for exact ranks, on the restatement
    Pd, md, gd, bd, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(goal, dev), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8)
    near, clear, ok = raw_clearance(a3d, Pd, md, Sd, smd)
    assert ok, name + ": guard bands"
    n_err = check_nearest(near, ref["nearest"], name)
    c_err = float(np.abs(clear.cpu().numpy().astype(np.float64) - ref["clearance"]).max())
    # chunking and determinism: the minimum is exact
    for chunks in (1, 3, 0):
        n2, c2, ok2 = raw_clearance(a3d, Pd, md, Sd, smd, n_chunks=chunks)
        assert ok2 and torch.equal(n2.view(torch.int32), near.view(torch.int32)) and torch.equal(c2.view(torch.int32), clear.view(torch.int32)), \
            "%s: n_chunks=%d" % (name, chunks)
    # the ranking with the term weighed
    w5 = R.weights_of({k: v for k, v in C.RULE.items() if k != C.TERM})
    got = raw_rank(a3d, "a3d_traj_rank_extra", Pd, md, gd, bd, w5, 1.0, tail=(clear.data_ptr(), float(C.RULE[C.TERM])))
    assert got["_ok"], name
    scores = got["scores"].cpu().numpy().astype(np.float64)
    s_scale, s_err = np.abs(ref["scores"]).max(), np.abs(scores - ref["scores"]).max()
    print("[parity] %s: nearest max_rel_err %.2e (bar %.0e), clearance max_abs_err %.2e (bar %.0e), scores %.2e/%.2e, "
          "rows inside the margin %d/%d" % (name, n_err, NEAR_RTOL, c_err, CLEAR_ATOL, s_err, s_scale,
                                            int((ref["nearest"] < C.MARGIN).sum()), int(np.isfinite(ref["nearest"]).sum())))
    assert n_err <= NEAR_RTOL, "%s: nearest max rel err %.3e > %g" % (name, n_err, NEAR_RTOL)
    assert c_err <= CLEAR_ATOL, "%s: clearance max abs err %.3e > %g" % (name, c_err, CLEAR_ATOL)
    assert s_err <= SCORE_TOL * s_scale, "%s: scores max err %.3e > %g * %.3e" % (name, s_err, SCORE_TOL, s_scale)
    assert np.array_equal(got["best"].cpu().numpy(), ref["best"]), name
    assert np.array_equal(got["order"].cpu().numpy(), ref["order"]), name
    assert np.array_equal(got["selected"].cpu().numpy(), ref["selected"]), name


# G L = 1088 rows: two row tiles of 1024 slots (4 per lane), the second holds 64 rows -- the only shape here whose tile index is not 0;
# 21 points: less than one staged tile, n_chunks = 3 gives chunks of 7
TWO_TILES = (1, 64, 17, 1, 3, 7)


@pytest.mark.parametrize("with_mask", [False, True], ids=["all-points", "scene-mask"])
@pytest.mark.parametrize("mask_kind", R.MASKS)
def test_two_row_tiles_vs_float64_restatement(a3d, dev, mask_kind, with_mask):
    """nearest and clearance of the second row tile (rows 1024 .. 1087), the bars of this file; no ranking, so no condition on gaps"""
    P, mask, _, _, S, sm = C.make_inputs(0, *TWO_TILES, 8, mask_kind)
    sm = sm if with_mask else None
    name = "traj_clearance two tiles %s %s" % (mask_kind, "scene-mask" if with_mask else "all-points")
    assert P.shape[1] * P.shape[2] == 1024 + 64
    near_ref, clear_ref = C.clearance_ref(P, mask, S, sm)
    Pd, md, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(S, dev), t(sm, dev, np.uint8)
    near, clear, ok = raw_clearance(a3d, Pd, md, Sd, smd)
    assert ok, name + ": guard bands"
    n_err = check_nearest(near, near_ref, name)
    got = clear.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(clear_ref)), name
    fin = ~np.isnan(clear_ref)
    c_err = float(np.abs(got[fin] - clear_ref[fin]).max()) if fin.any() else 0.0
    print("[parity] %s: nearest max_rel_err %.2e (bar %.0e), clearance max_abs_err %.2e (bar %.0e), finite rows of tile 1: %d" % (
        name, n_err, NEAR_RTOL, c_err, CLEAR_ATOL, int(np.isfinite(near_ref.reshape(-1)[1024:]).sum())))
    assert n_err <= NEAR_RTOL, "%s: nearest max rel err %.3e > %g" % (name, n_err, NEAR_RTOL)
    assert c_err <= CLEAR_ATOL, "%s: clearance max abs err %.3e > %g" % (name, c_err, CLEAR_ATOL)
    for chunks in (1, 3, 0):
        n2, c2, ok2 = raw_clearance(a3d, Pd, md, Sd, smd, n_chunks=chunks)
        assert ok2 and torch.equal(n2.view(torch.int32), near.view(torch.int32)) and torch.equal(c2.view(torch.int32), clear.view(torch.int32)), \
            "%s: n_chunks=%d" % (name, chunks)


# ------------------------------------------------------------------------------------------------ 2: special values
def test_no_counted_point_padded_rows_nan_rows_and_eaten_skips(a3d, dev):
    (P, mask, goal, bounds, S, sm), _ = case((2, 4, 17, 3, 16, 16), "scattered", 8, True)
    P = P.copy()
    P[0, 1, 3, 1] = np.nan
    P[1, 2, 0, 0] = np.inf
    P[1, 3, :, 2] = np.nan                                            # a whole candidate
    S2 = S.copy()
    S2[1] = np.nan                                                     # scene 1 has no counted point at all
    Pd, md, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(S2, dev), t(sm, dev, np.uint8)
    for skip in ((1, 1), (0, 0), (20, 0), (3, 30)):
        near_ref, clear_ref = C.clearance_ref(P, mask, S2, sm, skip=skip)
        near, clear, ok = raw_clearance(a3d, Pd, md, Sd, smd, skip=skip)
        assert ok
        assert check_nearest(near, near_ref, "special") <= NEAR_RTOL
        got = clear.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(clear_ref)), skip
        np.testing.assert_allclose(got[~np.isnan(got)], clear_ref[~np.isnan(clear_ref)], rtol=0, atol=CLEAR_ATOL)
    assert np.isnan(clear_ref).sum() == 0 and (clear_ref == 0).all()   # the last skip eats every row: 0, not NaN
    assert np.isposinf(near_ref[1, :3]).sum() > 3 * 8 and np.isnan(near_ref[1, 3]).sum() > 8 and np.isnan(near_ref[1, 2, 0])
    # another margin reaches the kernel
    near_ref, clear_ref = C.clearance_ref(P, mask, S2, sm, margin=0.2)
    _, clear, _ = raw_clearance(a3d, Pd, md, Sd, smd, margin=0.2)
    fin = ~np.isnan(clear_ref)
    np.testing.assert_allclose(clear.cpu().numpy()[fin], clear_ref[fin], rtol=0, atol=CLEAR_ATOL)
    assert (clear_ref[fin] > 0.2).any()


# ------------------------------------------------------------------------------------------------ 3: mechanics
def test_null_nearest_second_launch_and_the_public_function(a3d, dev):
    (P, mask, goal, bounds, S, sm), ref = case((1, 8, 50, 2, 64, 64), "suffix", 8, True)
    Pd, md, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(S, dev), t(sm, dev, np.uint8)
    near, clear, ok = raw_clearance(a3d, Pd, md, Sd, smd)
    near2, clear2, ok2 = raw_clearance(a3d, Pd, md, Sd, smd)
    assert ok and ok2 and torch.equal(near, near2) and torch.equal(clear, clear2)          # a second launch: the same bits
    none, clear3, ok3 = raw_clearance(a3d, Pd, md, Sd, smd, want_nearest=False)
    assert none is None and ok3 and torch.equal(clear3, clear)
    out = a3d.trajectory_clearance(Pd, md.bool(), Sd, smd.bool())
    assert isinstance(out, a3d.TrajectoryClearance) and torch.equal(out.nearest, near) and torch.equal(out.clearance, clear)
    assert torch.equal(a3d.trajectory_clearance(Pd, md, Sd, smd).clearance, clear)         # uint8 masks
    # the scene read in place through a slice of a (B, history, C, 3, H, W) observation
    pcds = torch.full((1, 3) + tuple(Sd.shape[1:]), float("nan"), device=dev)
    pcds[:, -1] = Sd
    view = pcds[:, -1]
    assert view.is_contiguous() and view.data_ptr() != pcds.data_ptr()
    assert torch.equal(a3d.trajectory_clearance(Pd, md.bool(), view, smd.bool()).nearest, near)
    # the (B, N, 3) form: the same points as rows
    rows = Sd.reshape(1, 2, 3, -1).permute(0, 1, 3, 2).reshape(1, -1, 3)
    assert not rows.is_contiguous() or rows.shape == (1, 8192, 3)
    out = a3d.trajectory_clearance(Pd, md.bool(), rows, smd.reshape(1, -1))
    assert torch.equal(out.nearest, near) and torch.equal(out.clearance, clear)
    # without a scene mask more points count: nowhere farther, somewhere nearer
    free = a3d.trajectory_clearance(Pd, md.bool(), Sd)
    fin = torch.isfinite(near)
    assert (free.nearest[fin] <= near[fin]).all() and (free.nearest[fin] < near[fin]).any()


def test_rank_extra_without_the_term_has_the_bits_of_rank(a3d, dev):
    for shape, kind in (((2, 4, 17, 3, 16, 16), "scattered"), ((1, 64, 16, 1, 33, 31), "none")):
        (P, mask, goal, bounds, S, sm), _ = case(shape, kind, 8, True)
        Pd, md, gd, bd = t(P, dev), t(mask, dev, np.uint8), t(goal, dev), t(bounds, dev)
        w = R.weights_of(R.MIXED)
        a = raw_rank(a3d, "a3d_traj_rank", Pd, md, gd, bd, w, 1.0)
        b = raw_rank(a3d, "a3d_traj_rank_extra", Pd, md, gd, bd, w, 1.0, tail=(None, 0.0))
        nan_extra = torch.full((P.shape[0], P.shape[1]), float("nan"), device=dev)
        c = raw_rank(a3d, "a3d_traj_rank_extra", Pd, md, gd, bd, w, 1.0, tail=(nan_extra.data_ptr(), 0.0))   # given, not weighed
        for k in ("best", "order", "scores", "terms", "selected"):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
        assert a["_ok"] and b["_ok"] and c["_ok"]


def test_rank_trajectories_with_and_without_the_term(a3d, dev):
    (P, mask, goal, bounds, S, sm), ref = case((2, 4, 17, 3, 16, 16), "scattered", 8, True)
    Pd, md, gd, bd, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(goal, dev), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8)
    # a rule that does not name the term: today's launch, today's tuple, whatever the scene arguments are
    raw = raw_rank(a3d, "a3d_traj_rank", Pd, md, gd, bd, R.weights_of(R.MIXED), 1.0)
    for kw in ({}, dict(scene=Sd, scene_mask=smd.bool()), dict(scene=Sd, margin=0.2, skip=(0, 3))):
        rk = a3d.rank_trajectories(Pd, md.bool(), goal=gd, bounds=bd, select=R.MIXED, **kw)
        assert type(rk) is a3d.TrajectoryRanking and len(rk) == 5
        for k in rk._fields:
            assert torch.equal(getattr(rk, k), raw[k]), k
    rk0 = a3d.rank_trajectories(Pd, md.bool(), goal=gd, bounds=bd, select=dict(R.MIXED, clearance=0.0))
    assert type(rk0) is a3d.TrajectoryRanking and torch.equal(rk0.scores, raw["scores"])
    # the term weighed
    rk = a3d.rank_trajectories(Pd, md.bool(), goal=gd, bounds=bd, select=C.RULE, scene=Sd, scene_mask=smd.bool())
    assert type(rk) is a3d.SceneTrajectoryRanking and rk._fields[:5] == a3d.TrajectoryRanking._fields
    cl = a3d.trajectory_clearance(Pd, md.bool(), Sd, smd.bool())
    assert torch.equal(rk.clearance, cl.clearance) and torch.equal(rk.nearest, cl.nearest) and rk.terms.shape == (2, 4, 5)
    assert np.array_equal(rk.best.cpu().numpy(), ref["best"]) and np.array_equal(rk.order.cpu().numpy(), ref["order"])
    np.testing.assert_allclose(rk.scores.cpu().numpy(), ref["scores"], rtol=0, atol=SCORE_TOL * np.abs(ref["scores"]).max())
    # the preset: the term alone
    ref1 = C.scene_rank_ref(P, mask, goal, bounds, "clear", S, sm)
    rk1 = a3d.rank_trajectories(Pd, md.bool(), select="clear", scene=Sd, scene_mask=smd.bool())
    assert torch.equal(rk1.scores, cl.clearance) and torch.equal(rk1.clearance, cl.clearance)
    np.testing.assert_allclose(rk1.scores.cpu().numpy(), ref1["scores"], rtol=0, atol=CLEAR_ATOL)
    # margin and skip reach the kernel
    rk2 = a3d.rank_trajectories(Pd, md.bool(), select="clear", scene=Sd, margin=0.2, skip=(0, 2))
    _, c2 = C.clearance_ref(P, mask, S, None, margin=0.2, skip=(0, 2))
    np.testing.assert_allclose(rk2.clearance.cpu().numpy(), c2, rtol=0, atol=CLEAR_ATOL)


def test_one_call_captured_in_a_graph_and_replayed_with_a_changed_cloud(a3d, dev):
    shape = (2, 4, 17, 3, 16, 16)
    (P, mask, goal, bounds, S, sm), _ = case(shape, "suffix", 8, True)
    Pd, md, gd, bd, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(goal, dev), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8)
    sP, sm_, sS, sM = Pd.clone(), md.bool().clone(), Sd.clone(), smd.bool().clone()
    call = lambda: a3d.rank_trajectories(sP, sm_, goal=gd, bounds=bd, select=C.RULE, scene=sS, scene_mask=sM)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                        # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for seed, kind in ((0, "suffix"), (5, "scattered"), (6, "none")):
        P2, mask2, _, _, S2, sm2 = C.make_inputs(seed, *shape, 8, kind)
        sP.copy_(t(P2, dev)), sm_.copy_(t(mask2, dev, np.uint8).bool()), sS.copy_(t(S2, dev)), sM.copy_(t(sm2, dev, np.uint8).bool())
        g.replay()
        eager = a3d.rank_trajectories(t(P2, dev), t(mask2, dev, np.uint8).bool(), goal=gd, bounds=bd, select=C.RULE, scene=t(S2, dev),
                                      scene_mask=t(sm2, dev, np.uint8).bool())
        for k in eager._fields:
            a, b = getattr(out, k), getattr(eager, k)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (seed, k)    # bits: NaN and +inf positions included


# ------------------------------------------------------------------------------------------------ 4: integration
@pytest.fixture(scope="module")
def models(a3d, dev):
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        kp = make_keypose(a3d, dev)
        pl = make_planner(a3d, dev, backbone_of=kp)
        instr = torch.randn(1, 53, 512, generator=torch.Generator().manual_seed(77)).to(dev)
        o = observation(dev, 1, 2, 16)
        for _ in range(2):                       # settle the convolution library's algorithm choice
            by_hand(kp, pl, instr, o, n_steps=1)
        return kp, pl, instr
    finally:
        torch.backends.cudnn.deterministic = old


KW = dict(num_inference_steps=4, scheduler="ddim")
E2E_RULE = {"consensus": 1, "clearance": 5}
E2E_CLEAR = dict(clear_margin=0.08, clear_skip=(1, 2))


def hand_written(a3d, cands, mask, goal, bounds, scene, scene_mask):
    """what a user writes without the option: sample, then trajectory_clearance, then rank_trajectories"""
    cl = a3d.trajectory_clearance(cands, mask, scene, scene_mask, margin=E2E_CLEAR["clear_margin"], skip=E2E_CLEAR["clear_skip"])
    rk = a3d.rank_trajectories(cands, mask, goal=goal, bounds=bounds, select=E2E_RULE, scene=scene, scene_mask=scene_mask,
                               margin=E2E_CLEAR["clear_margin"], skip=E2E_CLEAR["clear_skip"])
    assert torch.equal(rk.clearance, cl.clearance) and torch.equal(rk.nearest, cl.nearest)
    ref = C.scene_rank_ref(cands.cpu().numpy(), mask.cpu().numpy(), goal.cpu().numpy(), bounds.cpu().numpy(), E2E_RULE,
                           scene.cpu().numpy(), scene_mask.cpu().numpy(), margin=E2E_CLEAR["clear_margin"], skip=E2E_CLEAR["clear_skip"])
    np.testing.assert_allclose(rk.scores.cpu().numpy(), ref["scores"], rtol=0, atol=SCORE_TOL * np.abs(ref["scores"]).max())
    np.testing.assert_allclose(rk.clearance.cpu().numpy(), ref["clearance"], rtol=0, atol=CLEAR_ATOL)
    if R.gaps_ok(ref["scores"]):
        assert np.array_equal(rk.best.cpu().numpy(), ref["best"])
    return rk


def scene_mask_of(dev, pcd, seed):
    return (torch.rand(pcd.shape[0], pcd.shape[1], pcd.shape[3], pcd.shape[4], generator=torch.Generator().manual_seed(seed)) < 0.2).to(dev)


def test_compute_trajectory_select_clearance(a3d, models, dev):
    kp, pl, instr = models
    B, G, Ln = 2, 3, 16
    o = observation(dev, 51, B, Ln)
    init, _ = candidate_noise(dev, B, G, Ln, 4)
    goal = o["gt_action"][:, -1, :7]
    pcd = o["pcds"][:, -1]                                             # a slice of the observation: read in place
    smask = scene_mask_of(dev, pcd, 3)
    args = (o["mask"], o["rgbs"][:, -1] / 2 + 0.5, pcd, instr.expand(B, -1, -1).contiguous(), o["gripper"][:, -1, :7], goal)
    kw = dict(KW, num_samples=G, init_noise=init)
    cands = pl.compute_trajectory(*args, **kw)
    want = hand_written(a3d, cands, o["mask"], goal, pl.gripper_loc_bounds, pcd, smask)
    sel = pl.compute_trajectory(*args, select=E2E_RULE, scene_mask=smask, **E2E_CLEAR, **kw)
    rk = pl.last_ranking
    assert sel.shape == (B, Ln, 7) and torch.equal(sel, want.selected) and torch.equal(sel, rk.selected)
    assert rk._fields == a3d.SceneTrajectoryRanking._fields + ("candidates",) and torch.equal(rk.candidates, cands)
    for k in want._fields:
        assert torch.equal(getattr(rk, k), getattr(want, k)), k
    assert rk.clearance.shape == (B, G) and rk.nearest.shape == (B, G, Ln) and torch.isfinite(rk.clearance).all()
    # through forward(run_inference=True)
    out = pl(None, *args, run_inference=True, select=E2E_RULE, scene_mask=smask, **E2E_CLEAR, **kw)
    assert torch.equal(out, sel)
    # a rule without the term leaves today's tuple on the planner
    pl.compute_trajectory(*args, select="consensus", **kw)
    assert pl.last_ranking._fields == a3d.TrajectoryRanking._fields + ("candidates",)
    # the captured loop, then the clearance and ranking launches after the replay
    for _ in range(2):
        assert torch.equal(pl.compute_trajectory(*args, select=E2E_RULE, scene_mask=smask, use_graph=True, **E2E_CLEAR, **kw), sel)
        assert torch.equal(pl.last_ranking.clearance, want.clearance)
    pl._graph = None


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_actioner_predict_select_clearance(a3d, models, dev, use_graph):
    kp, pl, instr = models
    B, G, Ln = 2, 3, 16
    o = observation(dev, 52, B, Ln)
    init, _ = candidate_noise(dev, B, G, Ln, 4, seed=10)
    smask = scene_mask_of(dev, o["pcds"][:, -1], 4)
    act = a3d.Actioner(kp, pl, predict_trajectory=True)
    act.set_instruction(instr)
    set_rng(kp)
    all_ = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], num_samples=G, init_noise=init, use_graph=use_graph, **KW)
    assert all_["trajectory"].shape == (B, G, Ln, 7)
    cands = all_["trajectory"].clone()
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], num_samples=G, init_noise=init, select=E2E_RULE,
                      scene_mask=smask, use_graph=use_graph, **E2E_CLEAR, **KW)
    assert out["trajectory"].shape == (B, Ln, 7) and torch.equal(out["action"], all_["action"])
    assert act.last_ranking is pl.last_ranking and torch.equal(act.last_ranking.candidates, cands)
    want = hand_written(a3d, cands, o["mask"], out["action"][..., :7], pl.gripper_loc_bounds, o["pcds"][:, -1], smask)
    assert torch.equal(out["trajectory"], want.selected)
    for k in want._fields:
        assert torch.equal(getattr(act.last_ranking, k), getattr(want, k)), k
    pl._graph = None
