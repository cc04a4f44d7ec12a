"""CPU-only tests of the scene clearance term (a3d_traj_clearance, a3d_traj_rank_extra, diffusion.trajectory_clearance,
rank_trajectories / compute_trajectory / Actioner.predict with select={"clearance": w}): self-checks of the float64 restatement in
tests/traj_clearance_ref.py on hand-computed cases, the three C-ABI entries (export, header arity, every argument error without a
device) and every host-side ValueError on CPU tensors before any library call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import traj_clearance_ref as C
import traj_rank_ref as R
from conftest import ROOT, load_pkg
from test_actioner_cpu import _Keypose, _Planner, _obs

ID = [1.0, 0.0, 0.0, 0.0]


def poses_of(xyz):
    """(G, L, 3) -> (1, G, L, 7) fp32 with identity rotations"""
    xyz = np.asarray(xyz, dtype=np.float32)
    q = np.broadcast_to(np.float32(ID), xyz.shape[:-1] + (4,))
    return np.concatenate([xyz, q], -1)[None]


def cloud_of(points):
    """(N, 3) -> (1, 1, 3, 1, N) fp32, channel-planar"""
    return np.asarray(points, dtype=np.float32).T.reshape(1, 1, 3, 1, -1)


# ------------------------------------------------------------------------------------------------ the restatement
def test_hand_computed_one_point():
    """one candidate walks along x at height 0.03 above the single point (1, 0, 0): rows at x = 0, 1, 1.04, 2"""
    P = poses_of([[[0, 0, 0.03], [1, 0, 0.03], [1.04, 0, 0.03], [2, 0, 0.03]]])
    mask = np.zeros((1, 4), dtype=bool)
    S = cloud_of([[1, 0, 0]])
    p64 = P[0, 0, :, :3].astype(np.float64)
    want = np.sqrt(((p64 - np.float64(np.float32([1, 0, 0]))) ** 2).sum(-1))
    near, clear = C.clearance_ref(P, mask, S, None, margin=0.05, skip=(0, 0))
    np.testing.assert_allclose(near[0, 0], want, rtol=1e-15)
    np.testing.assert_allclose(want[:2], [np.sqrt(1 + 0.03 ** 2), 0.03], rtol=1e-7)                  # fp32 storage of 0.03
    h = np.maximum(0, 0.05 - want) / 0.05                                                             # rows 0 and 3 are clear
    assert h[0] == 0 and h[3] == 0 and abs(h[1] - 0.4) < 1e-6 and 0 <= h[2] < 1e-5                    # row 2: 5 cm, up to fp32 storage
    np.testing.assert_allclose(clear[0, 0], h.mean(), rtol=1e-15)
    # the default skips drop row 0 and the last valid row; with row 3 padded that is row 2
    _, c11 = C.clearance_ref(P, mask, S)
    np.testing.assert_allclose(c11[0, 0], h[1:3].mean(), rtol=1e-15)
    near, c_pad = C.clearance_ref(P, np.array([[False, False, False, True]]), S)
    np.testing.assert_allclose(c_pad[0, 0], h[1], rtol=1e-15)
    assert np.isposinf(near[0, 0, 3]) and np.isfinite(near[0, 0, :3]).all()                           # a padded row is not computed
    # a scattered mask: valid rows 0, 2, 3 have ranks 0, 1, 2 -> only row 2 is scored
    _, c_sc = C.clearance_ref(P, np.array([[False, True, False, False]]), S)
    assert c_sc[0, 0] == h[2]


def test_a_point_exactly_at_the_margin_scores_zero_and_one_just_inside_does_not():
    m = 0.5                                                                                           # exact in fp32
    P = poses_of([[[9, 9, 9], [0, 0, 0], [0, 0, 0.25], [9, 9, 9]]])
    S = cloud_of([[0, 0, 0.5]])
    near, clear = C.clearance_ref(P, np.zeros((1, 4), dtype=bool), S, None, margin=m)
    assert near[0, 0, 1] == 0.5 and near[0, 0, 2] == 0.25
    assert clear[0, 0] == (0.0 + 0.5) / 2                                                             # hinge 0 at the margin, 1/2 half way


def test_masked_and_broken_points_do_not_count():
    P = poses_of([[[0, 0, 0], [0, 0, 0.01], [0, 0, 0.02], [0, 0, 0.03]], [[1, 0, 0], [1, 0, 0.01], [1, 0, 0.02], [1, 0, 0.03]]])
    mask = np.zeros((1, 4), dtype=bool)
    pts = [[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    S = cloud_of(pts)
    near, clear = C.clearance_ref(P, mask, S, None, skip=(0, 0))
    np.testing.assert_allclose(near[0], [[0, 0.01, 0.02, 0.03]] * 2, rtol=1e-6)
    # mask the first point: candidate 0 now sees only the point one metre away
    sm = np.zeros((1, 1, 1, 5), dtype=bool)
    sm[..., 0] = True
    near, clear = C.clearance_ref(P, mask, S, sm, skip=(0, 0))
    assert (near[0, 0] > 0.99).all() and clear[0, 0] == 0 and clear[0, 1] > 0.6
    # every point masked or broken: +inf everywhere, the hinge is 0
    sm[..., 1] = True
    near, clear = C.clearance_ref(P, mask, S, sm)
    assert np.isposinf(near).all() and (clear == 0).all()
    pts_c, counted = C.scene_points(S, sm)
    assert pts_c.shape == (1, 5, 3) and not counted.any()


def test_the_skips_can_eat_every_row():
    P = poses_of([[[0, 0, 0], [0, 0, 0.01], [0, 0, 0.02]]])
    S = cloud_of([[0, 0, 0]])
    mask = np.zeros((1, 3), dtype=bool)
    assert C.clearance_ref(P, mask, S, skip=(0, 0))[1][0, 0] > 0.7
    for skip in ((2, 1), (1, 2), (3, 0), (0, 3), (5, 5)):
        near, clear = C.clearance_ref(P, mask, S, skip=skip)
        assert clear[0, 0] == 0 and np.isfinite(near).all(), skip
    # two valid rows and the default skips: nothing in between
    assert C.clearance_ref(P, np.array([[False, True, False]]), S)[1][0, 0] == 0
    # a scene without a valid row
    near, clear = C.clearance_ref(P, np.ones((1, 3), dtype=bool), S)
    assert np.isposinf(near).all() and clear[0, 0] == 0


def test_a_nan_row_is_nan_and_spoils_its_candidate_only_where_it_is_scored():
    P = poses_of([[[0, 0, 0], [0, 0, 0.01], [0, 0, 0.02], [0, 0, 0.03]]] * 3)
    P[0, 0, 2, 1] = np.nan                                                                            # a scored row of candidate 0
    P[0, 1, 0, 0] = np.inf                                                                            # the skipped head of candidate 1
    S = cloud_of([[0, 0, 0]])
    near, clear = C.clearance_ref(P, np.zeros((1, 4), dtype=bool), S)
    assert np.isnan(near[0, 0, 2]) and np.isnan(near[0, 1, 0]) and np.isfinite(near[0, 2]).all()
    assert np.isnan(clear[0, 0]) and np.isfinite(clear[0, 1:]).all() and clear[0, 1] == clear[0, 2]
    # ... and ranks last; so does candidate 1, through the five-term sum (0 * NaN), as in traj_rank_ref
    ref = C.scene_rank_ref(P, np.zeros((1, 4), dtype=bool), None, None, "clear", S)
    assert np.isposinf(ref["scores"][0, :2]).all() and list(ref["order"][0]) == [2, 0, 1] and ref["best"][0] == 2
    assert ref["scores"][0, 2] == ref["clearance"][0, 2] > 0


def test_the_score_adds_the_weighed_term_last_and_the_seeded_cases_are_not_trivial():
    shape = (2, 4, 17, 3, 16, 16)
    P, mask, goal, bounds, S, sm = C.make_inputs(0, *shape, 8, "scattered")
    assert S.shape == (2, 3, 3, 16, 16) and S.dtype == np.float32 and sm.shape == (2, 3, 16, 16) and sm.dtype == bool
    assert 0.02 < sm.mean() < 0.25 and 0.01 < (~np.isfinite(S)).any(2).mean() < 0.15
    five = R.rank_ref(P, mask, goal, bounds, R.MIXED)
    rule = dict(R.MIXED, clearance=3.0)
    ref = C.scene_rank_ref(P, mask, goal, bounds, rule, S, sm)
    np.testing.assert_allclose(ref["scores"], five["scores"] + 3.0 * ref["clearance"], rtol=1e-15)
    assert np.array_equal(ref["terms"], five["terms"])
    assert (ref["clearance"] > 0.01).any() and (ref["clearance"] >= 0).all() and (ref["clearance"] <= 1).all()
    inside = ref["nearest"][np.isfinite(ref["nearest"])] < C.MARGIN
    assert 0.05 < inside.mean() < 0.95                                                                # rows on both sides of the hinge
    # a rule without the term is traj_rank_ref's
    same = C.scene_rank_ref(P, mask, goal, bounds, R.MIXED, S, sm)
    assert np.array_equal(same["scores"], five["scores"]) and np.array_equal(same["order"], five["order"])
    # the finder returns the seed the table of the GPU test holds for this case
    assert C.find_seed(*shape, 8, "scattered", True, tries=3) == 0


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.mark.parametrize("name,arity", [("a3d_traj_clearance_ws_floats", 5), ("a3d_traj_clearance", 18), ("a3d_traj_rank_extra", 23)])
def test_entries_are_exported_with_a_signature_of_the_header_arity(name, arity):
    a3d = load_pkg()
    lib = a3d.lib.load()
    header = open(os.path.join(ROOT, "include", "act3d_hip.h")).read()
    assert name in a3d.lib.exported_symbols() and hasattr(lib, name)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, "%s is not declared in include/act3d_hip.h" % name
    n_header = len([p for p in m.group(1).split(",") if p.strip()])
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_header == arity
    assert "traj_clearance.hip" in a3d.build.__globals__["SOURCES"]
    # a3d_traj_rank keeps its 21 arguments; the extra entry has them in the same order, then extra and w_extra before the stream
    assert len(lib.a3d_traj_rank.argtypes) == 21
    assert list(lib.a3d_traj_rank_extra.argtypes[:20]) == list(lib.a3d_traj_rank.argtypes[:20])


def test_workspace_size_without_a_device():
    a3d = load_pkg()
    ws = a3d.lib.load().a3d_traj_clearance_ws_floats
    B, G, L = 2, 3, 5
    for chunks in (1, 3, 7):
        assert ws(B, G, L, 1000, chunks) == chunks * B * G * L + B * L
    chosen = ws(1, 16, 50, 4 * 256 * 256, 0)
    assert (chosen - 50) % 800 == 0 and 1 <= (chosen - 50) // 800 <= 4096
    assert ws(1, 1, 1, 1, 0) == 1 + 1                                                                 # one point: one chunk
    assert ws(0, G, L, 10, 0) == 0 and ws(B, G, L, 10, -1) == 0


def test_traj_clearance_rejects_bad_arguments_without_a_device():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    d = ctypes.c_void_p(64)                                         # aligned, never dereferenced
    call = lib.a3d_traj_clearance

    def args(**kw):
        a = dict(poses=d, tmask=d, scene=d, smask=d, n_cam=2, n_pix=64, margin=0.05, sh=1, st=1, nearest=d, clearance=d, ws=d,
                 n_chunks=0, B=2, G=3, L=16, Dp=8)
        a.update(kw)
        return list(a.values()) + [None]

    def refused(**kw):
        assert call(*args(**kw)) == -22, kw
        assert b"a3d_traj_clearance" in lib.a3d_last_error_string(), kw

    for name in ("poses", "tmask", "scene", "clearance", "ws"):     # the required pointers (scene_mask and nearest may be NULL)
        refused(**{name: None})
    for name in ("B", "G", "L", "n_cam", "n_pix"):
        for v in (0, -1):
            refused(**{name: v})
    refused(G=65)
    for v in (6, 9, 0):
        refused(Dp=v)
    for v in (0.0, -0.05, float("nan"), float("inf")):
        refused(margin=v)
    refused(sh=-1)
    refused(st=-1)
    refused(n_chunks=-1)


def test_traj_rank_extra_rejects_bad_arguments_without_a_device():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    d = ctypes.c_void_p(64)
    call = lib.a3d_traj_rank_extra

    def args(**kw):
        a = dict(poses=d, tmask=d, goal=d, ldg=8, bounds=d, wc=1.0, wg=0.0, ws=0.0, wl=0.0, wb=0.0, rw=1.0, best=d, order=d, scores=d,
                 terms=d, selected=d, B=2, G=3, L=16, Dp=8, extra=d, we=1.0)
        a.update(kw)
        return list(a.values()) + [None]

    def refused(**kw):
        assert call(*args(**kw)) == -22, kw
        assert b"a3d_traj_rank_extra" in lib.a3d_last_error_string(), kw

    refused(extra=None)                                             # a non-zero weight without the term
    for v in (-1.0, float("nan"), float("inf")):
        refused(we=v)
    # ... and what a3d_traj_rank refuses, under this entry's name
    for name in ("poses", "tmask", "best"):
        refused(**{name: None})
    refused(G=65)
    refused(Dp=6)
    refused(B=0)
    refused(wg=1.0, goal=None)
    refused(wc=-1.0)


# ------------------------------------------------------------------------------------------------ host-side ValueErrors
def test_exports_and_unchanged_names():
    a3d = load_pkg()
    D = a3d.diffusion
    assert a3d.trajectory_clearance is D.trajectory_clearance and a3d.TrajectoryClearance is D.TrajectoryClearance
    assert a3d.SceneTrajectoryRanking is D.SceneTrajectoryRanking
    assert a3d.TrajectoryClearance._fields == ("nearest", "clearance")
    assert a3d.SceneTrajectoryRanking._fields == a3d.TrajectoryRanking._fields + ("clearance", "nearest")
    assert a3d.TrajectoryRanking._fields == ("best", "order", "scores", "terms", "selected")
    assert D.RANK_TERMS == ("consensus", "goal", "smooth", "length", "bounds") and "clear" not in D.RANK_PRESETS
    for kw in ("scene_mask", "clear_margin", "clear_skip"):
        assert kw in a3d.actioner._TRAJ_KW


def test_check_select_is_unchanged_and_check_scene_select_parses_the_term():
    D = load_pkg().diffusion
    # rules that do not name the term: today's five-element list, today's errors
    assert D.check_select("shortest") == [0.0, 0.0, 0.0, 1.0, 0.0] and D.check_select("consensus", False, False)[0] == 1.0
    assert D.check_select({"smooth": 2, "bounds": 0.5}) == [0.0, 0.0, 2.0, 0.0, 0.5]
    assert D.check_select({"consensus": 1, "goal": 0.0}, have_goal=False) == [1.0, 0.0, 0.0, 0.0, 0.0]
    for bad in ("clear", {"clearance": 1.0}, {"consensus": 1, "clearance": 1.0}, {}, {"consensus": 0.0}, "best"):
        with pytest.raises(ValueError):
            D.check_select(bad)                                      # check_select itself does not learn the new term
    for rule in ("shortest", {"smooth": 2, "bounds": 0.5}, "goal"):
        assert D.check_scene_select(rule) == (D.check_select(rule), 0.0)
    assert D.check_scene_select("clear") == ([0.0] * 5, 1.0)
    assert D.check_scene_select({"clearance": 2}) == ([0.0] * 5, 2.0)                                 # the only non-zero weight
    assert D.check_scene_select({"consensus": 1, "clearance": 5}) == ([1.0, 0.0, 0.0, 0.0, 0.0], 5.0)
    assert D.check_scene_select({"consensus": 1, "clearance": 0}, have_scene=False) == ([1.0, 0.0, 0.0, 0.0, 0.0], 0.0)
    bad = [dict(select="clear", have_scene=False), dict(select={"consensus": 1, "clearance": 0.5}, have_scene=False),
           dict(select={"clearance": 0}), dict(select={"clearance": 0.0, "consensus": 0.0}), dict(select={"clearance": -1.0}),
           dict(select={"clearance": float("nan")}), dict(select={"clearance": float("inf")}), dict(select={"clearance": "1"}),
           dict(select={"clearance": True}), dict(select={"clearance": 1, "speed": 1}), dict(select={"clearance": 1, "smooth": -1}),
           dict(select={"clearance": 1, "goal": 1}, have_goal=False), dict(select={"clearance": 1, "bounds": 1}, have_bounds=False),
           dict(select="clearance"), dict(select=None), dict(select=3)]
    for kw in bad:
        with pytest.raises(ValueError):
            D.check_scene_select(**kw)


def test_trajectory_clearance_value_errors_before_any_library_call():
    a3d = load_pkg()
    z = torch.zeros
    B, G, L = 2, 3, 5
    P, m, S, sm = z(B, G, L, 8), z(B, L, dtype=torch.bool), z(B, 2, 3, 4, 4), z(B, 2, 4, 4, dtype=torch.bool)
    bad = [dict(trajectories=z(B * G, L, 8)), dict(trajectories=z(B, G, L, 6)), dict(trajectories=z(B, G, L, 9)),
           dict(trajectories=z(B, 0, L, 8)), dict(trajectories=[[0.0]]), dict(trajectories=z(B, 65, L, 8)),
           dict(trajectory_mask=z(B, L + 1, dtype=torch.bool)), dict(trajectory_mask=z(L, dtype=torch.bool)), dict(trajectory_mask=None),
           dict(scene=None), dict(scene=z(B, 2, 4, 4, 4)), dict(scene=z(B + 1, 2, 3, 4, 4)), dict(scene=z(B, 2, 3, 4)),
           dict(scene=z(B, 16, 4)), dict(scene=z(B, 0, 3)), dict(scene=z(B, 2, 3, 0, 4)), dict(scene=z(B, 2, 3, 4, 4, dtype=torch.long)),
           dict(scene_mask=z(B, 2, 4, 5, dtype=torch.bool)), dict(scene_mask=z(B, 32, dtype=torch.bool)),
           dict(scene_mask=z(B, 2, 4, 4)), dict(scene_mask=[0]),
           dict(scene=z(B, 16, 3), scene_mask=sm), dict(scene=z(B, 16, 3), scene_mask=z(B, 15, dtype=torch.bool)),
           dict(margin=0), dict(margin=-0.05), dict(margin=float("nan")), dict(margin=float("inf")), dict(margin="0.05"),
           dict(margin=True),
           dict(skip=1), dict(skip=(1,)), dict(skip=(1, 1, 1)), dict(skip=(-1, 1)), dict(skip=(1, -1)), dict(skip=(1.0, 1)),
           dict(skip=(True, 1)), dict(skip=None)]
    for kw in bad:
        a = dict(trajectories=P, trajectory_mask=m, scene=S, scene_mask=sm, margin=0.05, skip=(1, 1))
        a.update(kw)
        with pytest.raises(ValueError):
            a3d.trajectory_clearance(**a)
    # the same arguments through rank_trajectories, which checks them only when the term is weighed
    for kw in ({}, dict(scene=z(B, 2, 4, 4, 4)), dict(scene_mask=z(B, 2, 4, 5, dtype=torch.bool)), dict(margin=-1.0), dict(skip=(1,))):
        a = dict(scene=S, scene_mask=sm, margin=0.05, skip=(1, 1), select={"consensus": 1, "clearance": 5})
        a.update(kw)
        if not kw:
            a["scene"] = None                                        # a clearance weight without a scene
        with pytest.raises(ValueError):
            a3d.rank_trajectories(P, m, **a)
    with pytest.raises(ValueError):
        a3d.rank_trajectories(P, m, select="clear")
    # valid arguments on CPU tensors get as far as the device check: there is no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a3d.trajectory_clearance(P, m, S, sm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a3d.rank_trajectories(P, m, select="clear", scene=z(B, 16, 3), scene_mask=z(B, 16, dtype=torch.uint8))


def test_compute_trajectory_clearance_raises_before_any_launch():
    a3d = load_pkg()
    m = a3d.DiffusionPlanner(embedding_dim=60, num_attn_heads=4, num_query_cross_attn_layers=6, use_instruction=True, use_goal=True,
                             gripper_loc_bounds=[[-1, -1, -1], [1, 1, 1]], rotation_parametrization="6D", diffusion_timesteps=100)
    B, Ln = 2, 8
    mask = torch.zeros(B, Ln, dtype=torch.bool)
    args = (mask, None, torch.zeros(B, 1, 3, 16, 16), torch.zeros(B, 53, 512), torch.zeros(B, 8), torch.zeros(B, 8))
    rule = {"consensus": 1, "clearance": 5}
    bad = [dict(select="clear"),                                                                     # num_samples is required
           dict(select=rule, num_samples=65), dict(select={"clearance": 0}, num_samples=3), dict(select={"clearance": -1}, num_samples=3),
           dict(select=rule, num_samples=3, scene_mask=torch.zeros(B, 1, 16, 15, dtype=torch.bool)),
           dict(select=rule, num_samples=3, scene_mask=torch.zeros(B, 1, 16, 16)),
           dict(select="clear", num_samples=3, clear_margin=0.0), dict(select="clear", num_samples=3, clear_margin=float("nan")),
           dict(select="clear", num_samples=3, clear_skip=(1,)), dict(select="clear", num_samples=3, clear_skip=(-1, 0)),
           dict(select=rule, num_samples=3, num_inference_steps=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            m.compute_trajectory(*args, **kw)
        with pytest.raises(ValueError):
            m(None, *args, run_inference=True, **kw)
    assert m.last_ranking is None


def test_actioner_predict_clearance_raises_before_any_launch():
    a3d = load_pkg()
    rgbs, pcds, grip = _obs()
    mask = torch.zeros(2, 8, dtype=torch.bool)
    kp, pl = _Keypose(), _Planner()
    act = a3d.Actioner(kp, pl, predict_keypose=True, predict_trajectory=True)
    act.set_instruction(torch.zeros(1, 53, 512))
    B, _, ncam, _, H, W = pcds.shape
    bad = [dict(select="clear"), dict(select="clear", num_samples=0), dict(select={"clearance": -1}, num_samples=3),
           dict(select={"clearance": 0}, num_samples=3),
           dict(select="clear", num_samples=3, scene_mask=torch.zeros(B, ncam, H, W + 1, dtype=torch.bool)),
           dict(select="clear", num_samples=3, scene_mask=torch.zeros(B, ncam, H, W)),
           dict(select="clear", num_samples=3, clear_margin=-0.1), dict(select="clear", num_samples=3, clear_skip=(1, 1, 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            act.predict(rgbs, pcds, grip, None, mask, **kw)
    with pytest.raises(TypeError):
        act.predict(rgbs, pcds, grip, None, mask, select="clear", num_samples=3, margin=0.05)         # the planner's names, not these
    assert kp.calls == 0
