"""GPU tests of clearance-guided sampling: the kernel pair (a3d_traj_guide) against the float64 restatement of tests/traj_guide_ref.py,
chunking and determinism, the exact-tie rule on the device, the mechanics of the entry (guard bands, NULL arguments, the (B, N, 3)
scene form, graph capture) and the integration into compute_trajectory(guide=...) and Actioner.predict.

Bars.  x' of a free row: 4 x the bound derived in traj_guide_ref.row_bar, per row, from the restatement's d -- world coordinates carry
e_p = 2^-22 max|coordinate|, the direction sqrt(3) e_p / d, so |err u| <= push sqrt(3) e_p ((margin - d) / d + 1) and |err v| <=
2 smooth e_p, converted with 2 / (hi - lo), plus 2^-23 |x'|.  An fp32 arg-min may differ from float64 where two points are almost
equidistant, so a pushed row may match the push from ANY counted point whose float64 distance is within 2e-6 m of the minimum; no row
is skipped.  The condition, asserted on the restatement first: such rows are at most 2 % of the pushed rows of a case and no pushed
row has d < 1e-4 m (checked on the CPU for seed 0 of every case below: at most 2 of 124 rows = 1.6 %, smallest d 6.9e-4 m).
`nearest`: 2e-6 relative, +inf / NaN positions exactly, as tests/test_traj_clearance_gpu.py.  Every row and channel outside the free
rows' xyz: the input's bits."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import traj_guide_ref as GR  # noqa: E402
from test_actioner_gpu import candidate_noise, make_keypose, make_planner, observation, set_rng, by_hand  # noqa: E402
from test_traj_clearance_gpu import POISON, NEAR_RTOL, check_nearest, guarded, guards_intact, scene_mask_of, t  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1, 1), (2, 3, 5, 1, 3, 7), (2, 4, 17, 3, 16, 16), (1, 8, 50, 2, 64, 64), (1, 64, 16, 1, 33, 31),
          (2, 2, 100, 4, 32, 32)]
SEED = 0


def bits(x):
    return x.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case_inputs(shape, mask_kind, D):
    P, mask, bounds, S, sm, cm = GR.make_inputs(SEED, *shape, D, mask_kind)
    for a in (P, mask, bounds, S, sm, cm):
        a.setflags(write=False)
    return P, mask, bounds, S, sm, cm


def raw_guide(a3d, X, mask_u8, cm_u8, bounds, S, sm_u8, n_chunks=0, margin=GR.MARGIN, skip=GR.SKIP, push=1.0, smooth=0.0,
              want_nearest=True):
    """a3d_traj_guide on guarded copies (signals, nearest, workspace) -> x' (B, G, L, D), nearest (B, G, L) or None, guards ok"""
    B, G, L, D = X.shape
    n_cam, n_pix = S.shape[1], S.shape[3] * S.shape[4]
    n_ws = a3d.lib.load().a3d_traj_guide_ws_floats(B, G, L, n_cam * n_pix, n_chunks)
    assert n_ws >= 2 * max(n_chunks, 1) * B * G * L
    bufs = {"x": guarded(X.numel(), X.device), "nearest": guarded(B * G * L, X.device), "ws": guarded(n_ws, X.device)}
    bufs["x"][1].copy_(X.reshape(-1))
    a3d.lib.call("a3d_traj_guide", bufs["x"][1].data_ptr(), D, mask_u8.data_ptr(), None if cm_u8 is None else cm_u8.data_ptr(),
                 bounds.data_ptr(), S.data_ptr(), None if sm_u8 is None else sm_u8.data_ptr(), n_cam, n_pix, float(margin), int(skip[0]),
                 int(skip[1]), float(push), float(smooth), bufs["nearest"][1].data_ptr() if want_nearest else None,
                 bufs["ws"][1].data_ptr(), n_chunks, B, G, L, a3d.lib.stream())
    torch.cuda.synchronize()
    ok = all(guards_intact(w, v.numel()) for w, v in bufs.values())
    if not want_nearest:
        ok = ok and bool((bufs["nearest"][1] == POISON).all())
    return bufs["x"][1].view(B, G, L, D), (bufs["nearest"][1].view(B, G, L) if want_nearest else None), ok


def check_against(got, X, ref, bar, name):
    """got, X: (B, G, L, D) device tensors after / before the step.  -> (largest error / bar over the free rows, rows that matched an
    alternative of a near tie)"""
    free = torch.from_numpy(ref["free"]).to(X.device)
    keep = torch.ones_like(X, dtype=torch.bool)
    keep[..., :3] = ~free[..., None]
    assert torch.equal(bits(got)[keep], bits(X)[keep]), name + ": a value outside the free rows' xyz changed"
    g = got[..., :3].cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - ref["x"][..., :3])                             # rows that are not finite are not free: not looked at
    worst, via_alt = 0.0, 0
    for key in zip(*np.nonzero(ref["free"])):
        ratio = (err[key] / bar[key]).max()
        if ratio > 1.0 and key in ref["alts"]:
            ratio = min((np.abs(g[key] - a) / bar[key]).max() for a in ref["alts"][key])
            via_alt += 1
        assert ratio <= 1.0, "%s: row %s off by %s, bar %s (d = %.3e)" % (name, key, err[key], bar[key], ref["d"][key])
        worst = max(worst, ratio)
    return worst, via_alt


# ------------------------------------------------------------------------------------------------ 1: against the restatement
@pytest.mark.parametrize("D", [9, 10])
@pytest.mark.parametrize("with_mask", [False, True], ids=["all-points", "scene-mask"])
@pytest.mark.parametrize("mask_kind", GR.MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_float64_restatement(a3d, dev, shape, mask_kind, with_mask, D):
    P, mask, bounds, S, sm, cm = case_inputs(shape, mask_kind, D)
    sm = sm if with_mask else None
    Pd, md, bd, Sd, smd, cmd = t(P, dev), t(mask, dev, np.uint8), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8), t(cm, dev)
    X = a3d.diffusion.pose_to_signal(Pd, bd)                           # the signals the sampler would hold for these poses
    assert X.shape == P.shape[:3] + (D,) and X.is_contiguous()
    Xn = X.cpu().numpy()
    for push, smooth in GR.PUSH_SMOOTH:
        name = "traj_guide %s %s D%d %s push %g smooth %g" % ("x".join(map(str, shape)), mask_kind, D,
                                                                "scene-mask" if with_mask else "all-points", push, smooth)
        ref = GR.guide_ref(Xn, mask, cm, bounds, S, sm, push=push, smooth=smooth)
        ties, n_push, d_min = GR.conditions(ref)
        assert ties <= 0.02 * n_push and d_min >= 1e-4, "%s: the case misses the condition (%d near ties of %d pushed rows, d_min %.2e)" % (
            name, ties, n_push, d_min)
        bar = GR.row_bar(ref, bounds, GR.MARGIN, push, smooth)
        got, near, ok = raw_guide(a3d, X, md, cmd, bd, Sd, smd, push=push, smooth=smooth)
        assert ok, name + ": guard bands"
        worst, via_alt = check_against(got, X, ref, bar, name)
        n_err = check_nearest(near, ref["nearest"], name)
        print("[parity] %s: x' max err / bar %.3f (bar = 4 x bound), nearest max_rel_err %.2e (bar %.0e), free rows %d, pushed %d, "
              "near ties %d (matched through an alternative: %d), d_min %.2e" % (name, worst, n_err, NEAR_RTOL, int(ref["free"].sum()),
                                                                               n_push, ties, via_alt, d_min))
        assert n_err <= NEAR_RTOL, "%s: nearest max rel err %.3e > %g" % (name, n_err, NEAR_RTOL)
        # chunking, a second launch: the minimum is exact and the tie rule total
        for chunks in (1, 3, 0):
            g2, n2, ok2 = raw_guide(a3d, X, md, cmd, bd, Sd, smd, n_chunks=chunks, push=push, smooth=smooth)
            assert ok2 and torch.equal(bits(g2), bits(got)) and torch.equal(bits(n2), bits(near)), "%s: n_chunks=%d" % (name, chunks)


# G L = 1088 rows: two row tiles of 1024 slots (4 per lane), the second holds 64 rows -- the only shape here whose tile index is not 0
TWO_TILES = (1, 64, 17, 1, 3, 7)


@pytest.mark.parametrize("with_mask", [False, True], ids=["all-points", "scene-mask"])
@pytest.mark.parametrize("mask_kind", GR.MASKS)
def test_two_row_tiles_vs_float64_restatement(a3d, dev, mask_kind, with_mask):
    """x' and nearest of the second row tile (rows 1024 .. 1087), D = 9, push 1, smooth 0.5, the bars and the condition of this file"""
    P, mask, bounds, S, sm, cm = GR.make_inputs(SEED, *TWO_TILES, 9, mask_kind)
    sm = sm if with_mask else None
    push, smooth = 1.0, 0.5
    name = "traj_guide two tiles %s %s" % (mask_kind, "scene-mask" if with_mask else "all-points")
    Pd, md, bd, Sd, smd, cmd = t(P, dev), t(mask, dev, np.uint8), t(bounds, dev), t(S, dev), t(sm, dev, np.uint8), t(cm, dev)
    X = a3d.diffusion.pose_to_signal(Pd, bd)
    assert X.shape == (1, 64, 17, 9) and X.shape[1] * X.shape[2] == 1024 + 64
    ref = GR.guide_ref(X.cpu().numpy(), mask, cm, bounds, S, sm, push=push, smooth=smooth)
    ties, n_push, d_min = GR.conditions(ref)
    assert ties <= 0.02 * n_push and d_min >= 1e-4, "%s: the case misses the condition (%d near ties of %d pushed rows, d_min %.2e)" % (
        name, ties, n_push, d_min)
    got, near, ok = raw_guide(a3d, X, md, cmd, bd, Sd, smd, push=push, smooth=smooth)
    assert ok, name + ": guard bands"
    worst, via_alt = check_against(got, X, ref, GR.row_bar(ref, bounds, GR.MARGIN, push, smooth), name)
    n_err = check_nearest(near, ref["nearest"], name)
    print("[parity] %s: x' max err / bar %.3f (bar = 4 x bound), nearest max_rel_err %.2e (bar %.0e), free rows %d (tile 1: %d), pushed %d "
          "(tile 1: %d), near ties %d (matched through an alternative: %d)" % (
              name, worst, n_err, NEAR_RTOL, int(ref["free"].sum()), int(ref["free"].reshape(-1)[1024:].sum()), n_push,
              int(ref["pushed"].reshape(-1)[1024:].sum()), ties, via_alt))
    assert n_err <= NEAR_RTOL, "%s: nearest max rel err %.3e > %g" % (name, n_err, NEAR_RTOL)
    for chunks in (1, 3, 0):
        g2, n2, ok2 = raw_guide(a3d, X, md, cmd, bd, Sd, smd, n_chunks=chunks, push=push, smooth=smooth)
        assert ok2 and torch.equal(bits(g2), bits(got)) and torch.equal(bits(n2), bits(near)), "%s: n_chunks=%d" % (name, chunks)


# ------------------------------------------------------------------------------------------------ 2: the tie rule and special values
def test_an_exact_tie_goes_to_the_lower_index_across_lanes_groups_passes_and_chunks(a3d, dev):
    """bounds (-1, 1): world == normalised, every value below is exact in fp32.  Two points exactly 0.25 from the row, everything
    else far away; wherever the two sit (the same group of four, two point groups of a tile, two staged passes, two chunks) the row is
    pushed away from the one with the LOWER index: x' = -(that point)."""
    bd = torch.tensor([[-1.0, -1, -1], [1, 1, 1]], device=dev)
    a, b = [0.25, 0.0, 0.0], [0.0, 0.25, 0.0]
    N = 1200
    for G, L in ((1, 1), (2, 50), (8, 50)):                             # 4, 2 and 1 point groups per tile; RPT 1, 1 and 2
        X = torch.zeros(1, G, L, 9, device=dev)
        X[..., 3:] = 0.5
        md = torch.zeros(1, L, dtype=torch.uint8, device=dev)
        for i1, i2 in ((1, 2), (1, 5), (6, 9), (5, 600), (2, 1100), (511, 512), (0, N - 1)):
            for first, second in ((a, b), (b, a)):
                S = torch.full((1, 1, 3, 1, N), 9.0, device=dev)
                S[0, 0, :, 0, i1] = torch.tensor(first, device=dev)
                S[0, 0, :, 0, i2] = torch.tensor(second, device=dev)
                for chunks in (1, 3, 0):
                    got, near, ok = raw_guide(a3d, X, md, None, bd, S, None, n_chunks=chunks, margin=0.5, skip=(0, 0), push=1.0)
                    assert ok and bool((near == 0.25).all())
                    want = X.clone()
                    want[..., :3] = -torch.tensor(first, device=dev)
                    assert torch.equal(got, want), (G, L, i1, i2, first, chunks)


def test_special_rows_no_counted_point_eaten_skips_and_nan(a3d, dev):
    P, mask, bounds, S, sm, cm = case_inputs((2, 4, 17, 3, 16, 16), "scattered", 10)
    bd = t(bounds, dev)
    X = a3d.diffusion.pose_to_signal(t(P, dev), bd)
    X[0, 1, 3, 1] = float("nan")
    X[1, 2, 0, 0] = float("inf")
    X[1, 3, :, 2] = float("nan")                                       # a whole candidate
    X[0, 2, 5, 4] = float("nan")                                       # a rotation channel: not read
    S2 = S.copy()
    S2[1] = np.nan                                                     # scene 1 has no counted point at all
    md, Sd, smd, cmd = t(mask, dev, np.uint8), t(S2, dev), t(sm, dev, np.uint8), t(cm, dev)
    Xn = X.cpu().numpy()
    for skip in ((1, 1), (0, 0), (20, 0), (3, 30)):
        ref = GR.guide_ref(Xn, mask, cm, bounds, S2, sm, skip=skip, push=1.0, smooth=0.5)
        got, near, ok = raw_guide(a3d, X, md, cmd, bd, Sd, smd, skip=skip, push=1.0, smooth=0.5)
        assert ok
        check_against(got, X, ref, GR.row_bar(ref, bounds, GR.MARGIN, 1.0, 0.5), "special skip %s" % (skip,))
        assert check_nearest(near, ref["nearest"], "special") <= NEAR_RTOL
    assert not ref["free"].any() and torch.equal(bits(got), bits(X))   # the last skip eats every row: nothing moves
    ref = GR.guide_ref(Xn, mask, cm, bounds, S2, sm, push=1.0, smooth=0.5)
    assert np.isposinf(ref["nearest"][1, :3]).sum() > 3 * 8 and np.isnan(ref["nearest"][1, 3]).sum() > 8 and np.isnan(ref["nearest"][0, 1, 3])
    assert ref["free"][1].any() and not ref["pushed"][1].any() and ref["pushed"][0].any()
    # another margin reaches the kernel
    ref = GR.guide_ref(Xn, mask, cm, bounds, S2, sm, margin=0.2, push=0.5)
    got, near, ok = raw_guide(a3d, X, md, cmd, bd, Sd, smd, margin=0.2, push=0.5)
    check_against(got, X, ref, GR.row_bar(ref, bounds, 0.2, 0.5, 0.0), "margin 0.2")
    narrow = GR.guide_ref(Xn, mask, cm, bounds, S2, sm, push=0.5)
    assert ok and ref["pushed"].sum() >= narrow["pushed"].sum() > 0 and np.abs(ref["u"]).sum() > 2 * np.abs(narrow["u"]).sum()


# ------------------------------------------------------------------------------------------------ 3: mechanics
def test_null_arguments_the_public_function_and_the_scene_forms(a3d, dev):
    P, mask, bounds, S, sm, cm = case_inputs((1, 8, 50, 2, 64, 64), "suffix", 10)
    bd, md, Sd, smd, cmd = t(bounds, dev), t(mask, dev, np.uint8), t(S, dev), t(sm, dev, np.uint8), t(cm, dev)
    X = a3d.diffusion.pose_to_signal(t(P, dev), bd)
    kw = dict(push=0.5, smooth=0.25)
    got, near, ok = raw_guide(a3d, X, md, cmd, bd, Sd, smd, **kw)
    got2, near2, ok2 = raw_guide(a3d, X, md, cmd, bd, Sd, smd, **kw)
    assert ok and ok2 and torch.equal(bits(got), bits(got2)) and torch.equal(bits(near), bits(near2))     # a second launch: the same bits
    got3, none, ok3 = raw_guide(a3d, X, md, cmd, bd, Sd, smd, want_nearest=False, **kw)
    assert none is None and ok3 and torch.equal(bits(got3), bits(got))
    # NULL cond_mask: the pinned rows move too (the restatement without a mask)
    free_all, near4, ok4 = raw_guide(a3d, X, md, None, bd, Sd, smd, **kw)
    Xn = X.cpu().numpy()
    ref = GR.guide_ref(Xn, mask, None, bounds, S, sm, **kw)
    check_against(free_all, X, ref, GR.row_bar(ref, bounds, GR.MARGIN, 0.5, 0.25), "no cond_mask")
    assert ok4 and torch.equal(bits(near4), bits(near)) and ref["free"].sum() > GR.guide_ref(Xn, mask, cm, bounds, S, sm, **kw)["free"].sum()
    # the public function: in place, returns nearest or None
    x = X.clone()
    out = a3d.guide_trajectories(x, md.bool(), Sd, bd, scene_mask=smd.bool(), cond_mask=cmd, want_nearest=True, **kw)
    assert torch.equal(bits(x), bits(got)) and torch.equal(bits(out), bits(near)) and out.shape == (1, 8, 50)
    x = X.clone()
    assert a3d.guide_trajectories(x, md, Sd, bd, scene_mask=smd, cond_mask=cmd.bool().view(1, 8, 50, 10), **kw) is None   # uint8 masks
    assert torch.equal(bits(x), bits(got))
    x = X.clone()
    a3d.guide_trajectories(x, md.bool(), Sd, bounds.tolist(), scene_mask=smd.bool(), cond_mask=cmd, **kw)                  # bounds as a list
    assert torch.equal(bits(x), bits(got))
    # (B, L, D) signals: one trajectory per scene
    x1 = X[:, 0].clone()
    n1 = a3d.guide_trajectories(x1, md.bool(), Sd, bd, scene_mask=smd.bool(), cond_mask=cmd[:1], want_nearest=True, **kw)
    assert torch.equal(bits(x1), bits(got[:, 0])) and n1.shape == (1, 50) and torch.equal(bits(n1), bits(near[:, 0]))
    # the scene read in place through a slice of a (B, history, C, 3, H, W) observation
    pcds = torch.full((1, 3) + tuple(Sd.shape[1:]), float("nan"), device=dev)
    pcds[:, -1] = Sd
    x = X.clone()
    a3d.guide_trajectories(x, md.bool(), pcds[:, -1], bd, scene_mask=smd.bool(), cond_mask=cmd, **kw)
    assert torch.equal(bits(x), bits(got))
    # the (B, N, 3) form: the same points as rows
    rows = Sd.reshape(1, 2, 3, -1).permute(0, 1, 3, 2).reshape(1, -1, 3)
    x = X.clone()
    out = a3d.guide_trajectories(x, md.bool(), rows, bd, scene_mask=smd.reshape(1, -1), cond_mask=cmd, want_nearest=True, **kw)
    assert torch.equal(bits(x), bits(got)) and torch.equal(bits(out), bits(near))
    # after a push of 1 no free row is left inside the margin of the point it was pushed from: trajectory_clearance agrees
    x = X.clone()
    a3d.guide_trajectories(x, md.bool(), Sd, bd, scene_mask=smd.bool(), cond_mask=cmd, push=1.0)
    before = a3d.trajectory_clearance(a3d.diffusion.signal_to_pose(X, bd), md.bool(), Sd, smd.bool()).nearest
    after = a3d.trajectory_clearance(a3d.diffusion.signal_to_pose(x, bd), md.bool(), Sd, smd.bool()).nearest
    free = torch.from_numpy(GR.guide_ref(Xn, mask, cm, bounds, S, sm)["free"]).to(dev)
    assert after[free].mean() > before[free].mean() and (after[free] < 0.99 * GR.MARGIN).sum() < (before[free] < 0.99 * GR.MARGIN).sum()


def test_one_call_captured_in_a_graph_and_replayed_with_a_changed_cloud(a3d, dev):
    shape = (2, 4, 17, 3, 16, 16)
    P, mask, bounds, S, sm, cm = case_inputs(shape, "suffix", 10)
    bd = t(bounds, dev)
    sX = a3d.diffusion.pose_to_signal(t(P, dev), bd)
    sM, sS, sSM, sCM = t(mask, dev, np.uint8).bool(), t(S, dev), t(sm, dev, np.uint8).bool(), t(cm, dev)
    call = lambda: a3d.guide_trajectories(sX, sM, sS, bd, scene_mask=sSM, cond_mask=sCM, push=0.5, smooth=0.25, want_nearest=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                        # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        near = call()
    for seed, kind in ((0, "suffix"), (5, "scattered"), (6, "none")):
        P2, mask2, _, S2, sm2, cm2 = GR.make_inputs(seed, *shape, 10, kind)
        X2 = a3d.diffusion.pose_to_signal(t(P2, dev), bd)
        sX.copy_(X2), sM.copy_(t(mask2, dev, np.uint8).bool()), sS.copy_(t(S2, dev)), sSM.copy_(t(sm2, dev, np.uint8).bool()), sCM.copy_(t(cm2, dev))
        g.replay()
        x = X2.clone()
        eager = a3d.guide_trajectories(x, t(mask2, dev, np.uint8).bool(), t(S2, dev), bd, scene_mask=t(sm2, dev, np.uint8).bool(),
                                       cond_mask=t(cm2, dev), push=0.5, smooth=0.25, want_nearest=True)
        assert torch.equal(bits(sX), bits(x)) and torch.equal(bits(near), bits(eager)), seed
        assert not torch.equal(x, X2)


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
CLEAR = dict(clear_margin=0.08, clear_skip=(1, 2))
B_, G_, L_ = 2, 3, 16


def call_args(dev, instr, seed):
    o = observation(dev, seed, B_, L_)
    init, _ = candidate_noise(dev, B_, G_, L_, 4)
    goal = o["gt_action"][:, -1, :7]
    pcd = o["pcds"][:, -1]                                             # a slice of the observation: read in place
    smask = scene_mask_of(dev, pcd, seed)
    args = (o["mask"], o["rgbs"][:, -1] / 2 + 0.5, pcd, instr.expand(B_, -1, -1).contiguous(), o["gripper"][:, -1, :7], goal)
    return o, args, dict(KW, num_samples=G_, init_noise=init, scene_mask=smask, **CLEAR)


def guide_by_hand(a3d, pl, signal, args, kw, push, smooth, want_nearest=False):
    """what compute_trajectory does after a guided step, written with the public function -> (the guided copy, nearest)"""
    mask, _, pcd, _, curr, goal = args
    cmask = a3d.diffusion.traj_condition(curr, goal, pl.gripper_loc_bounds, mask, None, G_, pl._use_goal_at_test)[3]
    x = signal.clone()
    near = a3d.guide_trajectories(x, mask, pcd, pl.gripper_loc_bounds, scene_mask=kw["scene_mask"], cond_mask=cmask,
                                  margin=kw["clear_margin"], skip=kw["clear_skip"], push=push, smooth=smooth, want_nearest=want_nearest)
    return x, near


@pytest.mark.parametrize("fused", [None, False], ids=["persistent", "op-by-op"])
def test_compute_trajectory_guide(a3d, models, dev, fused):
    kp, pl, instr = models
    o, args, kw = call_args(dev, instr, 61)
    kw["fused"] = fused
    pcd_before = args[2].clone()
    # without the keyword = guide=None: today's path, today's bits
    base = pl.compute_trajectory(*args, **kw)
    path = pl.last_sampler_path
    assert ("persistent" in path) == (fused is None) and pl.last_guidance is None
    none = pl.compute_trajectory(*args, guide=None, **kw)
    assert torch.equal(none, base) and pl.last_sampler_path == path and pl.last_guidance is None
    final0, trace0 = pl.compute_trajectory(*args, return_trace=True, **kw)
    assert torch.equal(final0, base) and len(trace0) == 4 and trace0[-1].shape == (B_, G_, L_, 9)
    # start = 3/4: only the terminal step is guided
    g34 = {"push": 1.0, "smooth": 0.25, "start": 0.75}
    got = pl.compute_trajectory(*args, guide=g34, **kw)
    want_x, want_near = guide_by_hand(a3d, pl, trace0[-1], args, kw, 1.0, 0.25, want_nearest=True)
    assert torch.equal(got, a3d.diffusion.signal_to_pose(want_x, pl.gripper_loc_bounds)) and not torch.equal(got, base)
    assert pl.last_sampler_path == path and type(pl.last_guidance) is a3d.Guidance and pl.last_guidance.steps == (3,)
    assert pl.last_guidance.nearest.shape == (B_, G_, L_) and torch.equal(bits(pl.last_guidance.nearest), bits(want_near))
    valid_free = ~o["mask"][:, None, :].expand(B_, G_, L_)
    assert (want_near[valid_free] < CLEAR["clear_margin"]).any()      # the cloud is dense: rows were pushed
    # start = 0.5, traced: entries 0..1 are the unguided ones, entry 2 is the guide step applied to the unguided entry 2
    g12 = {"push": 0.5, "smooth": 0.25}
    final1, trace1 = pl.compute_trajectory(*args, guide=g12, return_trace=True, **kw)
    assert len(trace1) == 4 and torch.equal(trace1[0], trace0[0]) and torch.equal(trace1[1], trace0[1])
    assert torch.equal(trace1[2], guide_by_hand(a3d, pl, trace0[2], args, kw, 0.5, 0.25)[0]) and not torch.equal(trace1[2], trace0[2])
    assert pl.last_guidance.steps == (2, 3)
    # the traced call's result equals the untraced one: the segmented and the per-step launch lists
    untraced = pl.compute_trajectory(*args, guide=g12, **kw)
    assert torch.equal(untraced, final1) and torch.equal(final1, a3d.diffusion.signal_to_pose(trace1[-1], pl.gripper_loc_bounds))
    # a bare number is the push, from the middle of the loop on
    assert torch.equal(pl.compute_trajectory(*args, guide=0.5, **kw), pl.compute_trajectory(*args, guide={"push": 0.5, "start": 0.5}, **kw))
    # start = 0 guides every step
    pl.compute_trajectory(*args, guide={"push": 1.0, "start": 0}, **kw)
    assert pl.last_guidance.steps == (0, 1, 2, 3)
    # one trajectory per scene (no candidate axis)
    kw1 = dict(kw, init_noise=kw["init_noise"][:, 0].contiguous())
    del kw1["num_samples"]
    one = pl.compute_trajectory(*args, guide=g34, **kw1)
    assert one.shape == (B_, L_, 7) and pl.last_guidance.nearest.shape == (B_, L_)
    assert not torch.equal(one, pl.compute_trajectory(*args, **kw1))
    assert torch.equal(args[2], pcd_before)                           # the caller's cloud is only read


def test_compute_trajectory_guide_graph_replay_and_select(a3d, models, dev):
    kp, pl, instr = models
    guide = {"push": 1.0, "smooth": 0.25, "start": 0.5}
    pl._graph = None
    calls = [call_args(dev, instr, seed) for seed in (62, 63)]        # two observations: another cloud, another mask of points
    eager = []
    for o, args, kw in calls:
        eager.append((pl.compute_trajectory(*args, guide=guide, **kw), pl.last_guidance.nearest.clone()))
    assert not torch.equal(eager[0][0], eager[1][0])
    for rounds in range(2):
        for (o, args, kw), (want, want_near) in zip(calls, eager):
            pcd_before = args[2].clone()
            got = pl.compute_trajectory(*args, guide=guide, use_graph=True, **kw)
            assert torch.equal(got, want) and torch.equal(bits(pl.last_guidance.nearest), bits(want_near))
            assert pl.last_guidance.steps == (2, 3) and torch.equal(args[2], pcd_before)
    key = pl._graph["key"]
    # another guide is another graph
    o, args, kw = calls[0]
    other = pl.compute_trajectory(*args, guide=0.5, use_graph=True, **kw)
    assert pl._graph["key"] != key and torch.equal(other, pl.compute_trajectory(*args, guide=0.5, **kw))
    pl._graph = None
    # together with select="clear": the guided candidates are ranked as the unguided ones are
    cands = pl.compute_trajectory(*args, guide=guide, **kw)
    assert torch.equal(cands, eager[0][0])
    rk = a3d.rank_trajectories(cands, args[0], goal=args[5], bounds=pl.gripper_loc_bounds, select="clear", scene=args[2],
                               scene_mask=kw["scene_mask"], margin=CLEAR["clear_margin"], skip=CLEAR["clear_skip"])
    sel = pl.compute_trajectory(*args, guide=guide, select="clear", **kw)
    assert sel.shape == (B_, L_, 7) and torch.equal(sel, rk.selected) and torch.equal(pl.last_ranking.candidates, cands)
    assert torch.equal(pl.last_ranking.clearance, rk.clearance) and pl.last_guidance.steps == (2, 3)
    unguided = pl.compute_trajectory(*args, select="clear", **kw)
    assert pl.last_guidance is None and unguided.shape == sel.shape


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_actioner_predict_guide(a3d, models, dev, use_graph):
    kp, pl, instr = models
    o = observation(dev, 64, B_, L_)
    init, _ = candidate_noise(dev, B_, G_, L_, 4, seed=10)
    smask = scene_mask_of(dev, o["pcds"][:, -1], 5)
    guide = {"push": 1.0, "smooth": 0.25, "start": 0.5}
    kw = dict(KW, num_samples=G_, init_noise=init, scene_mask=smask, **CLEAR)
    act = a3d.Actioner(kp, pl, predict_trajectory=True)
    act.set_instruction(instr)
    pl._graph = None
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], guide=guide, use_graph=use_graph, **kw)
    assert out["trajectory"].shape == (B_, G_, L_, 7) and pl.last_guidance.steps == (2, 3)
    near = pl.last_guidance.nearest.clone()
    # compute_trajectory on the chained inputs: the predicted keypose as the goal
    set_rng(kp)
    action, want, _ = by_hand(kp, pl, instr, o, guide=guide, **kw)
    assert torch.equal(out["action"], action) and torch.equal(out["trajectory"], want)
    assert torch.equal(bits(pl.last_guidance.nearest), bits(near))
    set_rng(kp)
    plain = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], use_graph=use_graph, **kw)
    assert not torch.equal(plain["trajectory"], out["trajectory"]) and pl.last_guidance is None
    # with select the guided candidates are ranked
    set_rng(kp)
    sel = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], guide=guide, select="clear", use_graph=use_graph, **kw)
    assert sel["trajectory"].shape == (B_, L_, 7) and torch.equal(act.last_ranking.candidates, want)
    pl._graph = None
