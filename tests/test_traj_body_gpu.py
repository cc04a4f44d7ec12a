"""GPU tests of the body-aware swept clearance: the kernels (a3d_traj_body_clearance) against the float64 restatement of
tests/traj_body_ref.py, the ranking with the term weighed (a3d_traj_rank_extra), chunking and determinism, the trivial body against
a3d_traj_clearance bit for bit, the public functions against the raw launches (the shared scan header moved nothing), the mechanics
of the entry (guard bands, NULL nearest, the scene read in place, the (B, N, 3) form, graph capture with a changed cloud and body),
the integration into rank_trajectories, compute_trajectory(clear_body=) and Actioner.predict, and a case with meaning.

Bars.  `nearest`: ABSOLUTE, 5 x 72 roundings x 2^-24 x the case's largest |coordinate| where finite (traj_body_ref.nearest_bar, the
count is written out next to traj_body_ref.ROUNDINGS: rotation, p + R o, the segment expression, the root, the radius); +inf and NaN
positions exactly.  A relative bar would not do: w = u - t d cancels where a point lies millimetres from a segment.  `clearance`: that
bar divided by the margin (the hinge has slope 1 / margin; the mean does not amplify).  `scores`: 5e-5 of the largest score of the
call, the bar of tests/test_traj_rank_gpu.py for the five-term sum, plus the weight times the clearance bar.  `best` and `order`:
EXACTLY the restatement's on seeds that meet traj_rank_ref.gaps_ok in the restatement (asserted first); the seeds below were found on
the CPU (traj_body_ref.find_seed); no case is skipped."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import traj_body_ref as Bd  # noqa: E402
import traj_clearance_ref as C  # noqa: E402
import traj_rank_ref as R  # noqa: E402
from test_actioner_gpu import candidate_noise, make_keypose, make_planner, observation, set_rng, by_hand  # noqa: E402
from test_traj_clearance_gpu import POISON, SCORE_TOL, guarded, guards_intact, raw_clearance, raw_rank, scene_mask_of, t  # noqa: E402
from test_traj_guide_gpu import case_inputs as guide_inputs, raw_guide  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, G, L, K, C, H, W)
SHAPES = [(1, 1, 1, 1, 1, 1, 1), (2, 3, 5, 2, 1, 3, 7), (2, 4, 17, 3, 3, 16, 16), (1, 8, 50, 8, 2, 32, 32), (1, 16, 4, 8, 1, 16, 16),
          (1, 64, 16, 1, 1, 33, 31), (2, 2, 100, 2, 4, 32, 32)]
# shape -> mask kind -> {"<Dp is 8><scene_mask><sweep>": seed}; 0 where not listed
SEEDS = {
    (2, 4, 17, 3, 3, 16, 16): {"none": {"010": 1, "110": 1}},
    (1, 8, 50, 8, 2, 32, 32): {"suffix": {"000": 1, "010": 1, "100": 1, "110": 1}, "none": {"000": 1, "100": 1}, "scattered": {"111": 1}},
    (1, 16, 4, 8, 1, 16, 16): {"none": {"001": 1, "101": 1}, "suffix": {"001": 2}, "scattered": {"001": 2, "101": 1}},
    (1, 64, 16, 1, 1, 33, 31): {
        "suffix": {"000": 359, "001": 1241, "010": 281, "011": 1844, "100": 359, "101": 1241, "110": 377, "111": 1844},
        "none": {"000": 3164, "001": 536, "010": 462, "011": 891, "100": 3164, "101": 536, "110": 462, "111": 891},
        "scattered": {"000": 804, "001": 362, "010": 612, "011": 5, "100": 432, "101": 687, "110": 1224, "111": 157}},
}


def seed_of(shape, mask_kind, Dp, with_mask, sweep):
    return SEEDS.get(shape, {}).get(mask_kind, {}).get("%d%d%d" % (Dp == 8, with_mask, sweep), 0)


@functools.lru_cache(maxsize=None)
def case(shape, mask_kind, Dp, with_mask, sweep):
    """inputs and restatement of one case, computed once and left unchanged -> (numpy inputs, ref dict)"""
    P, mask, goal, bounds, S, sm, o, r = Bd.make_inputs(seed_of(shape, mask_kind, Dp, with_mask, sweep), *shape, Dp, mask_kind)
    sm = sm if with_mask else None
    ref = Bd.body_rank_ref(P, mask, goal, bounds, C.RULE, S, o, r, sweep, sm)
    for a in (P, mask, goal, bounds, S, o, r) + ((sm,) if with_mask else ()):
        a.setflags(write=False)
    return (P, mask, goal, bounds, S, sm, o, r), ref


def bits(x):
    return x.contiguous().view(torch.int32)


def raw_body(a3d, P, mask_u8, o, r, sweep, S, sm_u8, n_chunks=0, margin=C.MARGIN, skip=C.SKIP, want_nearest=True):
    """a3d_traj_body_clearance on guarded buffers (workspace included) -> nearest (B, G, L) or None, clearance (B, G), guards ok"""
    B, G, L, Dp = P.shape
    K = o.shape[0]
    n_cam, n_pix = S.shape[1], S.shape[3] * S.shape[4]
    n_ws = a3d.lib.load().a3d_traj_body_clearance_ws_floats(B, G, L, K, n_cam * n_pix, n_chunks)
    assert n_ws >= (max(n_chunks, 1) + 8) * B * G * K * L + 3 * B * L
    bufs = {"nearest": guarded(B * G * L, P.device), "clearance": guarded(B * G, P.device), "ws": guarded(n_ws, P.device)}
    a3d.lib.call("a3d_traj_body_clearance", P.data_ptr(), mask_u8.data_ptr(), o.data_ptr(), r.data_ptr(), K, int(sweep), S.data_ptr(),
                 None if sm_u8 is None else sm_u8.data_ptr(), n_cam, n_pix, float(margin), int(skip[0]), int(skip[1]),
                 bufs["nearest"][1].data_ptr() if want_nearest else None, bufs["clearance"][1].data_ptr(), bufs["ws"][1].data_ptr(),
                 n_chunks, B, G, L, Dp, a3d.lib.stream())
    torch.cuda.synchronize()
    ok = all(guards_intact(w, v.numel()) for w, v in bufs.values())
    if not want_nearest:
        ok = ok and bool((bufs["nearest"][1] == POISON).all())
    return (bufs["nearest"][1].view(B, G, L) if want_nearest else None), bufs["clearance"][1].view(B, G), ok


def nearest_err(got, ref, name):
    """+inf / NaN positions exactly -> the largest ABSOLUTE error on the finite values"""
    got = got.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)), name + ": +inf positions"
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name + ": NaN positions"
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all(), name
    return float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0


def clearance_err(got, ref, name):
    got = got.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name + ": NaN candidates"
    fin = ~np.isnan(ref)
    return float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0


# ------------------------------------------------------------------------------------------------ 1: against the restatement
@pytest.mark.parametrize("sweep", [0, 1], ids=["still", "swept"])
@pytest.mark.parametrize("Dp", [7, 8])
@pytest.mark.parametrize("with_mask", [False, True], ids=["all-points", "scene-mask"])
@pytest.mark.parametrize("mask_kind", R.MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_float64_restatement(a3d, dev, shape, mask_kind, with_mask, Dp, sweep):
    (P, mask, goal, bounds, S, sm, o, r), ref = case(shape, mask_kind, Dp, with_mask, sweep)
    name = "traj_body %s %s Dp%d %s %s" % ("x".join(map(str, shape)), mask_kind, Dp, "scene-mask" if with_mask else "all-points",
                                           "swept" if sweep else "still")
    assert R.gaps_ok(ref["scores"]), name                              # the condition for exact ranks, on the restatement
    near_bar = Bd.nearest_bar(P, S, o)
    clear_bar = near_bar / C.MARGIN
    Pd, md, gd, bd, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(goal, dev), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8)
    od, rd = t(o, dev), t(r, dev)
    near, clear, ok = raw_body(a3d, Pd, md, od, rd, sweep, Sd, smd)
    assert ok, name + ": guard bands"
    n_err = nearest_err(near, ref["nearest"], name)
    c_err = clearance_err(clear, ref["clearance"], name)
    # chunking, determinism and a second launch: the minimum is exact
    for chunks in (1, 3, 0):
        n2, c2, ok2 = raw_body(a3d, Pd, md, od, rd, sweep, Sd, smd, n_chunks=chunks)
        assert ok2 and torch.equal(bits(n2), bits(near)) and torch.equal(bits(c2), bits(clear)), "%s: n_chunks=%d" % (name, chunks)
    # the ranking with the term weighed
    w5 = R.weights_of({k: v for k, v in C.RULE.items() if k != C.TERM})
    wc = float(C.RULE[C.TERM])
    got = raw_rank(a3d, "a3d_traj_rank_extra", Pd, md, gd, bd, w5, 1.0, tail=(clear.data_ptr(), wc))
    assert got["_ok"], name
    scores = got["scores"].cpu().numpy().astype(np.float64)
    s_scale, s_err = np.abs(ref["scores"]).max(), np.abs(scores - ref["scores"]).max()
    fin = np.isfinite(ref["nearest"])
    print("[parity] %s: nearest max_abs_err %.2e m (bar %.2e), clearance max_abs_err %.2e (bar %.2e), scores %.2e/%.2e, "
          "rows inside the margin %d/%d, rows with a sphere in contact %d" % (
              name, n_err, near_bar, c_err, clear_bar, s_err, s_scale, int((ref["nearest"][fin] < C.MARGIN).sum()), int(fin.sum()),
              int((ref["nearest"][fin] < 0).sum())))
    assert n_err <= near_bar, "%s: nearest max abs err %.3e > %.3e" % (name, n_err, near_bar)
    assert c_err <= clear_bar, "%s: clearance max abs err %.3e > %.3e" % (name, c_err, clear_bar)
    assert s_err <= SCORE_TOL * s_scale + wc * clear_bar, "%s: scores max err %.3e" % (name, s_err)
    assert np.array_equal(got["best"].cpu().numpy(), ref["best"]), name
    assert np.array_equal(got["order"].cpu().numpy(), ref["order"]), name
    assert np.array_equal(got["selected"].cpu().numpy(), ref["selected"]), name


def test_special_rows_nan_poses_zero_quaternions_no_counted_point_and_eaten_skips(a3d, dev):
    (P, mask, goal, bounds, S, sm, o, r), _ = case((2, 4, 17, 3, 3, 16, 16), "scattered", 8, True, 1)
    P = P.copy()
    P[0, 1, 3, 1] = np.nan                                             # poisons its own row and, through e(j), the valid row before it
    P[0, 2, 6, 3:7] = 0                                                # a zero quaternion
    P[0, 3, 8, 5] = np.inf                                             # a non-finite quaternion component
    P[1, 3, :, 2] = np.nan                                             # a whole candidate
    S2 = S.copy()
    S2[1] = np.nan                                                     # scene 1 has no counted point at all
    Pd, md, Sd, smd, od, rd = t(P, dev), t(mask, dev, np.uint8), t(S2, dev), t(sm, dev, np.uint8), t(o, dev), t(r, dev)
    near_bar = Bd.nearest_bar(P, S2, o)
    for sweep in (1, 0):
        for skip in ((1, 1), (0, 0), (20, 0), (3, 30)):
            near_ref, clear_ref = Bd.body_ref(P, mask, S2, o, r, sweep, sm, skip=skip)
            near, clear, ok = raw_body(a3d, Pd, md, od, rd, sweep, Sd, smd, skip=skip)
            assert ok
            assert nearest_err(near, near_ref, "special %s" % (skip,)) <= near_bar
            assert clearance_err(clear, clear_ref, "special %s" % (skip,)) <= near_bar / C.MARGIN
        assert (clear_ref == 0).all()                                  # the last skip eats every row: 0, not NaN
    assert np.isnan(Bd.body_ref(P, mask, S2, o, r, 1, sm)[0][0, 1:4]).sum() >= 4
    # another margin reaches the kernel
    near_ref, clear_ref = Bd.body_ref(P, mask, S2, o, r, 1, sm, margin=0.2)
    _, clear, _ = raw_body(a3d, Pd, md, od, rd, 1, Sd, smd, margin=0.2)
    assert clearance_err(clear, clear_ref, "margin") <= near_bar / 0.2 and (clear_ref[~np.isnan(clear_ref)] > 0.2).any()


# ------------------------------------------------------------------------------------------------ 2: bits
@pytest.mark.parametrize("mask_kind", R.MASKS)
@pytest.mark.parametrize("shape", [(2, 3, 5, 1, 3, 7), (2, 4, 17, 3, 16, 16), (1, 8, 50, 2, 32, 32), (1, 64, 17, 1, 3, 7), (2, 2, 100, 4, 32, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_the_trivial_body_has_the_bits_of_traj_clearance(a3d, dev, shape, mask_kind):
    """K = 1, zero offset, zero radius, sweep = 0 against a3d_traj_clearance on the same inputs (1 x 64 x 17: two row tiles)"""
    P, mask, _, _, S, sm = C.make_inputs(1, *shape, 8, mask_kind)
    o, r, sweep = Bd.TRIVIAL
    Pd, md, Sd, smd, od, rd = t(P, dev), t(mask, dev, np.uint8), t(S, dev), t(sm, dev, np.uint8), t(o, dev), t(r, dev)
    for m in (None, smd):
        for skip in ((1, 1), (0, 2)):
            near0, clear0, ok0 = raw_clearance(a3d, Pd, md, Sd, m, skip=skip)
            near1, clear1, ok1 = raw_body(a3d, Pd, md, od, rd, sweep, Sd, m, skip=skip)
            assert ok0 and ok1 and torch.equal(bits(near1), bits(near0)) and torch.equal(bits(clear1), bits(clear0)), (shape, mask_kind, skip)
    out = a3d.body_clearance(Pd, md.bool(), Sd, a3d.GripperBody(od, rd, False), smd.bool(), skip=(0, 2))
    assert torch.equal(bits(out.nearest), bits(near0)) and torch.equal(bits(out.clearance), bits(clear0))


def test_the_public_functions_have_the_bits_of_the_raw_launches(a3d, dev):
    """trajectory_clearance, guide_trajectories and rank_trajectories(body=None) on a fixed seeded case against a3d_traj_clearance,
    a3d_traj_guide and a3d_traj_rank_extra called directly: the wrappers add nothing, and None is today's call"""
    shape = (2, 4, 17, 3, 16, 16)
    P, mask, goal, bounds, S, sm = C.make_inputs(0, *shape, 8, "scattered")
    Pd, md, gd, bd, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(goal, dev), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8)
    near, clear, ok = raw_clearance(a3d, Pd, md, Sd, smd)
    out = a3d.trajectory_clearance(Pd, md.bool(), Sd, smd.bool())
    assert ok and torch.equal(bits(out.nearest), bits(near)) and torch.equal(bits(out.clearance), bits(clear))
    w5 = R.weights_of({k: v for k, v in C.RULE.items() if k != C.TERM})
    raw = raw_rank(a3d, "a3d_traj_rank_extra", Pd, md, gd, bd, w5, 1.0, tail=(clear.data_ptr(), float(C.RULE[C.TERM])))
    for kw in ({}, dict(body=None)):
        rk = a3d.rank_trajectories(Pd, md.bool(), goal=gd, bounds=bd, select=C.RULE, scene=Sd, scene_mask=smd.bool(), **kw)
        assert type(rk) is a3d.SceneTrajectoryRanking
        for k in a3d.TrajectoryRanking._fields:
            assert torch.equal(bits(getattr(rk, k)), bits(raw[k])), k
        assert torch.equal(bits(rk.nearest), bits(near)) and torch.equal(bits(rk.clearance), bits(clear))
    # a body with a rule that does not weigh the term: checked and otherwise ignored
    plain = a3d.rank_trajectories(Pd, md.bool(), goal=gd, bounds=bd, select=R.MIXED)
    with_body = a3d.rank_trajectories(Pd, md.bool(), goal=gd, bounds=bd, select=R.MIXED, scene=Sd, body=a3d.GripperBody([[0, 0, 0.05]], [0.02]))
    assert type(with_body) is a3d.TrajectoryRanking and all(torch.equal(bits(a), bits(b)) for a, b in zip(plain, with_body))
    # the guide step
    GP, gmask, gbounds, GS, gsm, cm = guide_inputs(shape, "scattered", 10)
    gmd, gbd, GSd, gsmd, cmd = t(gmask, dev, np.uint8), t(gbounds, dev), t(GS, dev), t(gsm, dev, np.uint8), t(cm, dev)
    Xd = a3d.diffusion.pose_to_signal(t(GP, dev), gbd)                 # the signals the sampler would hold for these poses
    assert Xd.shape == GP.shape[:3] + (10,) and Xd.is_contiguous()
    x_raw, n_raw, okg = raw_guide(a3d, Xd, gmd, cmd, gbd, GSd, gsmd, push=0.7, smooth=0.2)
    x_pub = Xd.clone()
    n_pub = a3d.guide_trajectories(x_pub, gmd.bool(), GSd, gbd, scene_mask=gsmd.bool(), cond_mask=cmd, push=0.7, smooth=0.2, want_nearest=True)
    assert okg and torch.equal(bits(x_pub), bits(x_raw)) and torch.equal(bits(n_pub), bits(n_raw))
    assert not torch.equal(x_pub, Xd)                                  # the step moved something


# ------------------------------------------------------------------------------------------------ 3: mechanics
def test_null_nearest_the_public_function_and_the_scene_forms(a3d, dev):
    (P, mask, goal, bounds, S, sm, o, r), ref = case((1, 8, 50, 8, 2, 32, 32), "suffix", 8, True, 1)
    Pd, md, Sd, smd, od, rd = t(P, dev), t(mask, dev, np.uint8), t(S, dev), t(sm, dev, np.uint8), t(o, dev), t(r, dev)
    near, clear, ok = raw_body(a3d, Pd, md, od, rd, 1, Sd, smd)
    none, clear3, ok3 = raw_body(a3d, Pd, md, od, rd, 1, Sd, smd, want_nearest=False)
    assert ok and none is None and ok3 and torch.equal(bits(clear3), bits(clear))
    body = a3d.GripperBody(od, rd)                                     # sweep defaults to True
    out = a3d.body_clearance(Pd, md.bool(), Sd, body, smd.bool())
    assert isinstance(out, a3d.TrajectoryClearance) and torch.equal(bits(out.nearest), bits(near)) and torch.equal(bits(out.clearance), bits(clear))
    # a dict, host tensors, uint8 masks
    out = a3d.body_clearance(Pd, md, Sd, {"offsets": torch.from_numpy(o.copy()), "radii": r.tolist(), "sweep": True}, smd)
    assert torch.equal(bits(out.nearest), bits(near)) and torch.equal(bits(out.clearance), bits(clear))
    still = a3d.body_clearance(Pd, md.bool(), Sd, body._replace(sweep=False), smd.bool())
    fin = torch.isfinite(near)
    assert (near[fin] <= still.nearest[fin]).all() and (near[fin] < still.nearest[fin]).any()         # a segment contains its start
    # the scene read in place through a slice of a (B, history, C, 3, H, W) observation
    pcds = torch.full((1, 3) + tuple(Sd.shape[1:]), float("nan"), device=dev)
    pcds[:, -1] = Sd
    view = pcds[:, -1]
    assert view.is_contiguous() and view.data_ptr() != pcds.data_ptr()
    assert torch.equal(bits(a3d.body_clearance(Pd, md.bool(), view, body, smd.bool()).nearest), bits(near))
    # the (B, N, 3) form: the same points as rows
    rows = Sd.reshape(1, 2, 3, -1).permute(0, 1, 3, 2).reshape(1, -1, 3)
    out = a3d.body_clearance(Pd, md.bool(), rows, body, smd.reshape(1, -1))
    assert torch.equal(bits(out.nearest), bits(near)) and torch.equal(bits(out.clearance), bits(clear))
    # through rank_trajectories: the term and nearest come from body_clearance
    gd, bd = t(goal, dev), t(bounds, dev)
    rk = a3d.rank_trajectories(Pd, md.bool(), goal=gd, bounds=bd, select=C.RULE, scene=Sd, scene_mask=smd.bool(), body=body)
    assert type(rk) is a3d.SceneTrajectoryRanking and torch.equal(bits(rk.nearest), bits(near)) and torch.equal(bits(rk.clearance), bits(clear))
    assert np.array_equal(rk.best.cpu().numpy(), ref["best"]) and np.array_equal(rk.order.cpu().numpy(), ref["order"])


def test_one_call_captured_in_a_graph_and_replayed_with_a_changed_cloud_and_body(a3d, dev):
    shape = (2, 4, 17, 3, 3, 16, 16)
    (P, mask, goal, bounds, S, sm, o, r), _ = case(shape, "suffix", 8, True, 1)
    Pd, md, gd, bd, Sd, smd = t(P, dev), t(mask, dev, np.uint8), t(goal, dev), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8)
    sP, sm_, sS, sM, sO, sR = Pd.clone(), md.bool().clone(), Sd.clone(), smd.bool().clone(), t(o, dev), t(r, dev)
    body = a3d.GripperBody(sO, sR)                                     # device tensors: read at launch time, nothing is copied
    call = lambda: a3d.rank_trajectories(sP, sm_, goal=gd, bounds=bd, select=C.RULE, scene=sS, scene_mask=sM, body=body)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                        # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    seen = []
    for seed, kind in ((0, "suffix"), (5, "scattered"), (6, "none")):
        P2, mask2, _, _, S2, sm2, o2, r2 = Bd.make_inputs(seed, *shape, 8, kind)
        sP.copy_(t(P2, dev)), sm_.copy_(t(mask2, dev, np.uint8).bool()), sS.copy_(t(S2, dev)), sM.copy_(t(sm2, dev, np.uint8).bool())
        sO.copy_(t(o2, dev)), sR.copy_(t(r2, dev))
        g.replay()
        eager = a3d.rank_trajectories(t(P2, dev), t(mask2, dev, np.uint8).bool(), goal=gd, bounds=bd, select=C.RULE, scene=t(S2, dev),
                                      scene_mask=t(sm2, dev, np.uint8).bool(), body=a3d.GripperBody(t(o2, dev), t(r2, dev)))
        for k in eager._fields:
            assert torch.equal(bits(getattr(out, k)), bits(getattr(eager, k))), (seed, k)             # NaN and +inf positions included
        seen.append(out.clearance.clone())
    # the body alone: same poses and cloud, other spheres
    sR.add_(0.01)
    g.replay()
    assert not torch.equal(out.clearance, seen[-1]) and (out.clearance >= seen[-1]).all()


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
# made-up numbers, as every body in these tests: no preset ships
E2E_BODY = dict(offsets=[[0.0, 0.0, -0.06], [0.0, 0.04, 0.0], [0.0, -0.04, 0.0]], radii=[0.04, 0.015, 0.015])


def hand_written(a3d, cands, mask, goal, bounds, scene, scene_mask, body):
    """what a user writes without the option: sample, then body_clearance, then rank_trajectories"""
    cl = a3d.body_clearance(cands, mask, scene, body, scene_mask, margin=E2E_CLEAR["clear_margin"], skip=E2E_CLEAR["clear_skip"])
    rk = a3d.rank_trajectories(cands, mask, goal=goal, bounds=bounds, select=E2E_RULE, scene=scene, scene_mask=scene_mask,
                               margin=E2E_CLEAR["clear_margin"], skip=E2E_CLEAR["clear_skip"], body=body)
    assert torch.equal(bits(rk.clearance), bits(cl.clearance)) and torch.equal(bits(rk.nearest), bits(cl.nearest))
    o, r = np.float32(E2E_BODY["offsets"]), np.float32(E2E_BODY["radii"])
    ref = Bd.body_rank_ref(cands.cpu().numpy(), mask.cpu().numpy(), goal.cpu().numpy(), bounds.cpu().numpy(), E2E_RULE, scene.cpu().numpy(),
                           o, r, 1, scene_mask.cpu().numpy(), margin=E2E_CLEAR["clear_margin"], skip=E2E_CLEAR["clear_skip"])
    clear_bar = Bd.nearest_bar(cands.cpu().numpy(), scene.cpu().numpy(), o) / E2E_CLEAR["clear_margin"]
    np.testing.assert_allclose(rk.clearance.cpu().numpy(), ref["clearance"], rtol=0, atol=clear_bar)
    np.testing.assert_allclose(rk.scores.cpu().numpy(), ref["scores"], rtol=0,
                               atol=SCORE_TOL * np.abs(ref["scores"]).max() + E2E_RULE["clearance"] * clear_bar)
    if R.gaps_ok(ref["scores"]):
        assert np.array_equal(rk.best.cpu().numpy(), ref["best"])
    return rk


def test_compute_trajectory_select_clear_body(a3d, models, dev):
    kp, pl, instr = models
    B, G, Ln = 2, 3, 16
    o = observation(dev, 51, B, Ln)
    init, _ = candidate_noise(dev, B, G, Ln, 4)
    goal = o["gt_action"][:, -1, :7]
    pcd = o["pcds"][:, -1]                                             # a slice of the observation: read in place
    smask = scene_mask_of(dev, pcd, 3)
    args = (o["mask"], o["rgbs"][:, -1] / 2 + 0.5, pcd, instr.expand(B, -1, -1).contiguous(), o["gripper"][:, -1, :7], goal)
    kw = dict(KW, num_samples=G, init_noise=init)
    body = a3d.GripperBody(**E2E_BODY)
    cands = pl.compute_trajectory(*args, **kw)
    want = hand_written(a3d, cands, o["mask"], goal, pl.gripper_loc_bounds, pcd, smask, body)
    point = a3d.rank_trajectories(cands, o["mask"], goal=goal, bounds=pl.gripper_loc_bounds, select=E2E_RULE, scene=pcd, scene_mask=smask,
                                  margin=E2E_CLEAR["clear_margin"], skip=E2E_CLEAR["clear_skip"])
    fin = torch.isfinite(point.nearest)
    assert (want.nearest[fin] < point.nearest[fin]).any()              # the body reaches further than the tool point
    sel = pl.compute_trajectory(*args, select=E2E_RULE, scene_mask=smask, clear_body=body, **E2E_CLEAR, **kw)
    rk = pl.last_ranking
    assert sel.shape == (B, Ln, 7) and torch.equal(sel, want.selected) and torch.equal(sel, rk.selected)
    assert rk._fields == a3d.SceneTrajectoryRanking._fields + ("candidates",) and torch.equal(rk.candidates, cands)
    for k in want._fields:
        assert torch.equal(bits(getattr(rk, k)), bits(getattr(want, k))), k
    # None is today's call, bit for bit
    pl.compute_trajectory(*args, select=E2E_RULE, scene_mask=smask, clear_body=None, **E2E_CLEAR, **kw)
    for k in point._fields:
        assert torch.equal(bits(getattr(pl.last_ranking, k)), bits(getattr(point, k))), k
    # a rule without the term: the body is checked and otherwise ignored
    pl.compute_trajectory(*args, select="consensus", clear_body=body, **kw)
    assert pl.last_ranking._fields == a3d.TrajectoryRanking._fields + ("candidates",)
    # the captured loop, then the clearance and ranking launches after the replay
    for _ in range(2):
        assert torch.equal(pl.compute_trajectory(*args, select=E2E_RULE, scene_mask=smask, clear_body=body, use_graph=True, **E2E_CLEAR, **kw), sel)
        assert torch.equal(bits(pl.last_ranking.clearance), bits(want.clearance))
    pl._graph = None


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_actioner_predict_select_clear_body(a3d, models, dev, use_graph):
    kp, pl, instr = models
    B, G, Ln = 2, 3, 16
    o = observation(dev, 52, B, Ln)
    init, _ = candidate_noise(dev, B, G, Ln, 4, seed=10)
    smask = scene_mask_of(dev, o["pcds"][:, -1], 4)
    body = a3d.GripperBody(**E2E_BODY)
    act = a3d.Actioner(kp, pl, predict_trajectory=True)
    act.set_instruction(instr)
    set_rng(kp)
    all_ = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], num_samples=G, init_noise=init, use_graph=use_graph, **KW)
    assert all_["trajectory"].shape == (B, G, Ln, 7)
    cands = all_["trajectory"].clone()
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], num_samples=G, init_noise=init, select=E2E_RULE,
                      scene_mask=smask, clear_body=body, use_graph=use_graph, **E2E_CLEAR, **KW)
    assert out["trajectory"].shape == (B, Ln, 7) and torch.equal(out["action"], all_["action"])
    assert act.last_ranking is pl.last_ranking and torch.equal(act.last_ranking.candidates, cands)
    want = hand_written(a3d, cands, o["mask"], out["action"][..., :7], pl.gripper_loc_bounds, o["pcds"][:, -1], smask, body)
    assert torch.equal(out["trajectory"], want.selected)
    for k in want._fields:
        assert torch.equal(bits(getattr(act.last_ranking, k)), bits(getattr(want, k))), k
    pl._graph = None


# ------------------------------------------------------------------------------------------------ 5: a case with meaning
def test_a_segment_through_a_box_is_seen_by_the_swept_body_and_not_by_the_point_term(a3d, dev):
    """Two candidates whose waypoints are mirror images in x about a box of scene points centred at the origin (the box is symmetric
    in x, so every waypoint of one has the distance of its mirror image, bit for bit).  Rows 1 -> 2 of candidate 0 run straight
    through the box; those of candidate 1 pass 18 cm beside it.  The tool-point term cannot tell them apart; the swept body can."""
    g = np.float32([-0.02, -0.01, 0.0, 0.01, 0.02])
    box = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)                            # 125 points, symmetric in x
    assert np.array_equal(np.sort(box[:, 0]), np.sort(-box[:, 0])) and (box == 0).all(-1).any()
    through = [[-0.4, 0.1, 0], [-0.2, 0.1, 0], [0.2, -0.1, 0], [0.4, -0.1, 0]]
    beside = [[-0.4, 0.1, 0], [-0.2, 0.1, 0], [-0.2, -0.1, 0], [-0.4, -0.1, 0]]
    xyz = np.float32([through, beside])
    q = np.broadcast_to(np.float32([1, 0, 0, 0]), (2, 4, 4))
    P = t(np.concatenate([xyz, q], -1)[None], dev)
    mask = torch.zeros(1, 4, dtype=torch.bool, device=dev)
    S = t(box.T.reshape(1, 1, 3, 5, 25), dev)
    body = a3d.GripperBody([[0.0, 0.0, 0.0]], [0.01])                  # made-up: one 1 cm sphere at the tool point
    point = a3d.trajectory_clearance(P, mask, S, margin=0.3)
    assert torch.equal(bits(point.nearest[0, 0]), bits(point.nearest[0, 1])) and torch.equal(point.clearance[0, 0], point.clearance[0, 1])
    assert 0 < float(point.clearance[0, 0]) < 0.5                      # both inside the margin, neither near contact
    tie = a3d.rank_trajectories(P, mask, select="clear", scene=S, margin=0.3)
    assert int(tie.best[0]) == 0 and float(tie.scores[0, 0]) == float(tie.scores[0, 1])               # a tie: the index decides
    swept = a3d.body_clearance(P, mask, S, body, margin=0.3)
    assert float(swept.nearest[0, 0, 1]) <= -0.01 + 1e-6               # the segment passes through the grid point at the origin
    assert float(swept.nearest[0, 1, 1]) > 0.15
    assert float(swept.clearance[0, 0]) > float(swept.clearance[0, 1]) + 0.2
    rk = a3d.rank_trajectories(P, mask, select="clear", scene=S, margin=0.3, body=body)
    assert int(rk.best[0]) == 1 and rk.order[0].tolist() == [1, 0]
    still = a3d.body_clearance(P, mask, S, body._replace(sweep=False), margin=0.3)                  # without the sweep: equal again
    assert torch.equal(bits(still.clearance[0, 0]), bits(still.clearance[0, 1]))
    # the restatement agrees
    near_ref, clear_ref = Bd.body_ref(P.cpu().numpy(), mask.cpu().numpy(), S.cpu().numpy(), np.zeros((1, 3), np.float32), np.float32([0.01]), 1,
                                      margin=0.3)
    np.testing.assert_allclose(swept.nearest.cpu().numpy(), near_ref, rtol=0, atol=Bd.nearest_bar(P.cpu().numpy(), S.cpu().numpy(), [0.0]))
    assert clear_ref[0, 0] > clear_ref[0, 1] + 0.2
