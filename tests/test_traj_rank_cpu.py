"""CPU-only tests of the candidate ranking (a3d_traj_rank, diffusion.rank_trajectories, compute_trajectory(select=...),
Actioner.predict(select=...)): self-checks of the float64 restatement in tests/traj_rank_ref.py on hand-computed cases, the new
C-ABI entry (export, header arity, every argument error without a device) and every host-side ValueError on CPU tensors before any
library call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import traj_rank_ref as R
from conftest import ROOT, load_pkg
from test_actioner_cpu import _Keypose, _Planner, _obs

ID = [1.0, 0.0, 0.0, 0.0]


def row(x, y, z, q=ID):
    return [x, y, z] + list(q)


# ------------------------------------------------------------------------------------------------ the restatement
def test_hand_computed_two_candidates_three_rows():
    """candidate 0 walks along x in steps of 1 with the identity rotation; candidate 1 is 3 higher in y on rows 0, 1, bends on row 2
    and is turned by 90 degrees about z throughout (<q, r> = cos 45 -> rho = 1/2)."""
    s = np.sqrt(0.5)
    qz = [s, 0.0, 0.0, s]
    P = np.array([[[row(0, 0, 0), row(1, 0, 0), row(2, 0, 0)],
                   [row(0, 3, 0, qz), row(1, 3, 0, qz), row(2, 7, 0, qz)]]], dtype=np.float32)         # (1, 2, 3, 7)
    mask = np.zeros((1, 3), dtype=bool)
    goal = np.array([row(2, 0, 4) + [1.0]], dtype=np.float32)                                         # identity rotation
    bounds = np.array([[-1, -1, -1], [5, 5, 5]], dtype=np.float32)
    rw = 2.0
    out = R.rank_ref(P, mask, goal, bounds, {"consensus": 1.0}, rot_weight=rw)
    t = out["terms"][0]
    qd = float(R.rho(R.unit_quat(np.float32(qz)), np.array(ID)))
    assert abs(qd - 0.5) < 1e-7                                                                       # fp32 storage of sqrt(1/2)
    d01 = (3 + 3 + 7) / 3 + rw * qd                                                                   # mean over the three rows
    np.testing.assert_allclose(t[:, 0], [d01, d01], rtol=1e-12)                                       # G - 1 = 1
    np.testing.assert_allclose(t[:, 1], [4.0, np.sqrt(49 + 16) + rw * qd], rtol=1e-12)                # last row vs the goal
    np.testing.assert_allclose(t[:, 2], [0.0, 16.0], atol=1e-12)                                      # one triple: (0, 4, 0)
    np.testing.assert_allclose(t[:, 3], [2.0, 1.0 + np.sqrt(17.0)], rtol=1e-12)
    np.testing.assert_allclose(t[:, 4], [0.0, 1 / 3], rtol=1e-12)                                     # y = 7 is outside
    assert out["best"][0] == 0 and list(out["order"][0]) == [0, 1]                                    # an exact tie: lowest index
    out = R.rank_ref(P, mask, goal, bounds, {"goal": 1.0, "bounds": 3.0}, rot_weight=rw)
    np.testing.assert_allclose(out["scores"][0], [4.0, np.sqrt(65) + rw * qd + 1.0], rtol=1e-12)
    out = R.rank_ref(P[:, ::-1], mask, goal, bounds, "shortest")
    assert out["best"][0] == 1 and np.array_equal(out["selected"][0], P[0, 0])
    # a mask in the middle removes every pair and triple, and the goal row stays the last valid one
    out = R.rank_ref(P, np.array([[False, True, False]]), goal, bounds, "goal", rot_weight=rw)
    assert (out["terms"][0, :, 2:4] == 0).all()
    np.testing.assert_allclose(out["terms"][0, :, 0], [(3 + 7) / 2 + rw * qd] * 2, rtol=1e-12)
    np.testing.assert_allclose(out["terms"][0, 1, 4], 0.5)
    out = R.rank_ref(P, np.array([[False, False, True]]), goal, None, "goal", rot_weight=rw)           # i* = 1, no bounds
    np.testing.assert_allclose(out["terms"][0, :, 1], [np.sqrt(1 + 16), np.sqrt(1 + 9 + 16) + rw * qd], rtol=1e-12)
    assert (out["terms"][0, :, 4] == 0).all()


def test_rho_is_sign_invariant_exact_on_equal_rows_and_equals_one_minus_dot_squared():
    rng = np.random.default_rng(0)
    q, r = R.unit_quat(rng.normal(size=(1000, 4))), R.unit_quat(rng.normal(size=(1000, 4)))
    assert (R.rho(q, q) == 0).all() and (R.rho(q, -q) == 0).all()
    assert np.array_equal(R.rho(q, r), R.rho(q, -r)) and np.array_equal(R.rho(q, r), R.rho(r, q))
    np.testing.assert_allclose(R.rho(q, r), 1 - (q * r).sum(-1) ** 2, atol=1e-15)
    # sin^2 of half the angle between the rotations
    ang = rng.uniform(0, np.pi, 100)
    rz = np.stack([np.cos(ang / 2), 0 * ang, 0 * ang, np.sin(ang / 2)], -1)
    np.testing.assert_allclose(R.rho(rz, np.array(ID)), np.sin(ang / 2) ** 2, atol=1e-15)
    # normalisation: any positive scale, and a zero quaternion stays finite
    assert np.allclose(R.unit_quat(3.0 * q), q) and np.isfinite(R.unit_quat(np.zeros(4))).all()


def test_medoid_of_three_collinear_candidates():
    """candidates at x = 0, 1, 5 (all rows alike): consensus (1 + 5) / 2, (1 + 4) / 2, (5 + 4) / 2 -> the middle one"""
    P = np.zeros((1, 3, 4, 7), dtype=np.float32)
    P[..., 3] = 1.0
    P[0, :, :, 0] = np.array([0.0, 1.0, 5.0])[:, None]
    out = R.rank_ref(P, np.zeros((1, 4), dtype=bool))
    np.testing.assert_allclose(out["terms"][0, :, 0], [3.0, 2.5, 4.5], rtol=1e-12)
    assert out["best"][0] == 1 and list(out["order"][0]) == [1, 0, 2]
    assert np.array_equal(out["selected"][0], P[0, 1])


def test_arbitrary_masks_match_a_dense_call_on_the_valid_rows_where_adjacency_is_kept():
    """a scattered mask equals the unmasked call on the compacted rows for the terms without adjacency (consensus, goal, bounds);
    smooth / length only count neighbours that are adjacent in the ORIGINAL indexing"""
    P, _, goal, bounds = R.make_case(5, 2, 4, 12, 8, "none")
    mask = np.zeros((2, 12), dtype=bool)
    mask[:, [1, 2, 6, 11]] = True                     # valid: 0 | 3 4 5 | 7 8 9 10
    keep = np.nonzero(~mask[0])[0]
    a = R.rank_ref(P, mask, goal, bounds, R.MIXED)["terms"]
    b = R.rank_ref(P[:, :, keep], np.zeros((2, len(keep)), dtype=bool), goal, bounds, R.MIXED)["terms"]
    np.testing.assert_allclose(a[..., [0, 1, 4]], b[..., [0, 1, 4]], rtol=1e-13)
    p = P[..., :3].astype(np.float64)
    seg = lambda i: np.sqrt(((p[:, :, i + 1] - p[:, :, i]) ** 2).sum(-1))
    acc = lambda i: (((p[:, :, i + 1] - p[:, :, i]) - (p[:, :, i] - p[:, :, i - 1])) ** 2).sum(-1)
    np.testing.assert_allclose(a[..., 3], seg(3) + seg(4) + seg(7) + seg(8) + seg(9), rtol=1e-13)
    np.testing.assert_allclose(a[..., 2], (acc(4) + acc(8) + acc(9)) / 3, rtol=1e-13)


def test_empty_scenes_and_short_trajectories():
    P, _, goal, bounds = R.make_case(3, 2, 3, 5, 7, "none")
    mask = np.zeros((2, 5), dtype=bool)
    mask[1] = True                                    # n = 0
    out = R.rank_ref(P, mask, goal, bounds, R.MIXED)
    assert (out["terms"][1] == 0).all() and (out["scores"][1] == 0).all()
    assert out["best"][1] == 0 and list(out["order"][1]) == [0, 1, 2] and np.array_equal(out["selected"][1], P[1, 0])
    for L, zero in ((1, [2, 3]), (2, [2])):
        P, mask, goal, bounds = R.make_case(4, 2, 3, L, 7, "none")
        t = R.rank_ref(P, mask, goal, bounds, R.MIXED)["terms"]
        assert (t[..., zero] == 0).all() and (t[..., 0] > 0).all() and (t[..., 1] > 0).all()
        if L == 2:
            assert (t[..., 3] > 0).all()


def test_non_finite_scores_rank_last_and_stay_visible():
    P, mask, goal, bounds = R.make_case(6, 1, 4, 6, 8, "none")
    P[0, 2] = np.nan
    out = R.rank_ref(P, mask, goal, bounds, "shortest")
    assert out["order"][0, -1] == 2 and out["best"][0] != 2 and np.isinf(out["scores"][0, 2])
    P[:] = np.nan
    out = R.rank_ref(P, mask, goal, bounds, "shortest")
    assert out["best"][0] == 0 and list(out["order"][0]) == [0, 1, 2, 3] and np.isnan(out["selected"]).all()


def test_gap_condition_and_structural_tie():
    assert R.gaps_ok([[1.0, 2.0, 3.0]]) and not R.gaps_ok([[1.0, 1.0 + 1e-4, 3.0]]) and not R.gaps_ok([[1.0, np.inf]])
    assert R.gaps_ok([[0.0, 0.0, 0.0]]) and R.gaps_ok([[5.0]])
    assert not R.gaps_ok([[2.0, 2.0]]) and R.gaps_ok([[2.0, 2.0]], exact_ties=True)
    assert not R.gaps_ok([[2.0, 2.0 + 1e-9]], exact_ties=True)
    # G = 2: the consensus term is one number for both candidates, bit for bit
    for seed in range(5):
        P, mask, goal, bounds = R.make_case(seed, 3, 2, 9, 7, "scattered")
        t = R.rank_ref(P, mask, goal, bounds)["terms"]
        assert np.array_equal(t[:, 0, 0], t[:, 1, 0])
    assert R.structural_tie(2, "consensus") and not R.structural_tie(3, "consensus") and not R.structural_tie(2, "goal")
    assert not R.structural_tie(2, R.MIXED)


# ------------------------------------------------------------------------------------------------ the C entry
def test_rank_entry_is_exported_with_a_signature_of_the_header_arity():
    a3d = load_pkg()
    lib = a3d.lib.load()
    header = open(os.path.join(ROOT, "include", "act3d_hip.h")).read()
    name = "a3d_traj_rank"
    assert name in a3d.lib.exported_symbols() and hasattr(lib, name)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
    assert m, "%s is not declared in include/act3d_hip.h" % name
    n_header = len([p for p in m.group(1).split(",") if p.strip()])
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == n_header == 21
    assert "traj_rank.hip" in a3d.build.__globals__["SOURCES"]


def test_traj_rank_rejects_bad_arguments_without_a_device():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    d = ctypes.c_void_p(64)                                         # aligned, never dereferenced
    call = lib.a3d_traj_rank

    def args(**kw):
        a = dict(poses=d, tmask=d, goal=d, ldg=8, bounds=d, wc=1.0, wg=0.0, ws=0.0, wl=0.0, wb=0.0, rw=1.0, best=d, order=d, scores=d,
                 terms=d, selected=d, B=2, G=3, L=16, Dp=8)
        a.update(kw)
        return list(a.values()) + [None]

    def refused(**kw):
        assert call(*args(**kw)) == -22, kw
        assert b"a3d_traj_rank" in lib.a3d_last_error_string(), kw

    for name in ("poses", "tmask", "best"):                         # the required pointers
        refused(**{name: None})
    for name in ("B", "G", "L"):
        for v in (0, -1):
            refused(**{name: v})
    refused(G=65)
    for v in (6, 9, 0):
        refused(Dp=v)
    refused(ldg=6)
    refused(wg=1.0, goal=None)                                      # a goal weight without a goal
    refused(wb=0.5, bounds=None)                                    # a bounds weight without bounds
    refused(wc=-1.0)
    refused(ws=float("nan"))
    refused(wl=float("inf"))
    refused(rw=float("nan"))


# ------------------------------------------------------------------------------------------------ host-side ValueErrors
def test_rank_trajectories_value_errors_before_any_library_call():
    a3d = load_pkg()
    assert a3d.rank_trajectories is a3d.diffusion.rank_trajectories and a3d.TrajectoryRanking is a3d.diffusion.TrajectoryRanking
    assert a3d.TrajectoryRanking._fields == ("best", "order", "scores", "terms", "selected")
    rank = a3d.rank_trajectories
    z = torch.zeros
    B, G, L = 2, 3, 5
    P, m, goal, bounds = z(B, G, L, 8), z(B, L, dtype=torch.bool), z(B, 8), z(2, 3)
    bad = [dict(select="best"), dict(select="length"), dict(select=None), dict(select=3), dict(select={}),
           dict(select={"consensus": 0.0}), dict(select={"consensus": 1, "speed": 1}), dict(select={"smooth": -1.0}),
           dict(select={"smooth": float("nan")}), dict(select={"length": float("inf")}), dict(select={"goal": "1"}),
           dict(select={"goal": True}),
           dict(trajectories=z(B * G, L, 8)), dict(trajectories=z(B, G, L, 6)), dict(trajectories=z(B, G, L, 9)),
           dict(trajectories=z(B, 0, L, 8)), dict(trajectories=[[0.0]]),
           dict(trajectories=z(B, 65, L, 8)),                                               # G > 64
           dict(trajectory_mask=z(B, L + 1, dtype=torch.bool)), dict(trajectory_mask=z(B * G, L, dtype=torch.bool)),
           dict(trajectory_mask=z(L, dtype=torch.bool)), dict(trajectory_mask=None),
           dict(goal=z(B, 6)), dict(goal=z(B + 1, 8)), dict(goal=z(8)),
           dict(bounds=z(3, 2)), dict(bounds=z(6)),
           dict(select="goal", goal=None), dict(select={"consensus": 1, "goal": 0.1}, goal=None),
           dict(select={"bounds": 1.0}, bounds=None),
           dict(rot_weight=-1.0), dict(rot_weight=float("nan")), dict(rot_weight="1")]
    for kw in bad:
        a = dict(trajectories=P, trajectory_mask=m, goal=goal, bounds=bounds, select="consensus", rot_weight=1.0)
        a.update(kw)
        with pytest.raises(ValueError):
            rank(**a)
    D = a3d.diffusion
    assert D.check_select("shortest") == [0.0, 0.0, 0.0, 1.0, 0.0] and D.check_select("consensus", False, False)[0] == 1.0
    assert D.check_select({"smooth": 2, "bounds": 0.5}) == [0.0, 0.0, 2.0, 0.0, 0.5]
    assert D.check_select({"consensus": 1, "goal": 0.0}, have_goal=False) == [1.0, 0.0, 0.0, 0.0, 0.0]   # a zero weight needs no goal


def test_compute_trajectory_select_raises_before_any_launch():
    a3d = load_pkg()
    T = 100
    m = a3d.DiffusionPlanner(embedding_dim=60, num_attn_heads=4, num_query_cross_attn_layers=6, use_instruction=True, use_goal=True,
                             gripper_loc_bounds=[[-1, -1, -1], [1, 1, 1]], rotation_parametrization="6D", diffusion_timesteps=T)
    assert m.last_ranking is None
    B, Ln = 2, 8
    mask = torch.zeros(B, Ln, dtype=torch.bool)
    args = (mask, None, torch.zeros(B, 1, 3, 16, 16), torch.zeros(B, 53, 512), torch.zeros(B, 8), torch.zeros(B, 8))
    bad = [dict(select="consensus"),                                                        # num_samples is required
           dict(select="consensus", num_samples=None), dict(select="consensus", num_samples=0),
           dict(select="consensus", num_samples=65),
           dict(select="medoid", num_samples=3), dict(select={"consensus": 0}, num_samples=3),
           dict(select={"jerk": 1.0}, num_samples=3), dict(select={"smooth": -0.5}, num_samples=3),
           dict(select="smooth", num_samples=3, rot_weight=-2.0), dict(select="smooth", num_samples=3, rot_weight=float("inf")),
           dict(select="smooth", num_samples=3, num_inference_steps=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            m.compute_trajectory(*args, **kw)
        with pytest.raises(ValueError):                       # and through forward(run_inference=True, ...)
            m(None, *args, run_inference=True, **kw)
    assert m.last_ranking is None


def test_actioner_predict_select_raises_before_any_launch():
    a3d = load_pkg()
    rgbs, pcds, grip = _obs()
    mask = torch.zeros(2, 8, dtype=torch.bool)
    kp, pl = _Keypose(), _Planner()
    act = a3d.Actioner(kp, pl, predict_keypose=True, predict_trajectory=True)
    act.set_instruction(torch.zeros(1, 53, 512))
    assert "select" in a3d.actioner._TRAJ_KW and "rot_weight" in a3d.actioner._TRAJ_KW and act.last_ranking is None
    bad = [dict(select="consensus"), dict(select="consensus", num_samples=0), dict(select="consensus", num_samples=65),
           dict(select="closest", num_samples=3), dict(select={"goal": -1}, num_samples=3), dict(select={}, num_samples=3),
           dict(select="goal", num_samples=3, rot_weight=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            act.predict(rgbs, pcds, grip, None, mask, **kw)
    only_kp = a3d.Actioner(kp, None, predict_keypose=True, predict_trajectory=False)
    only_kp.set_instruction(torch.zeros(1, 53, 512))
    with pytest.raises(ValueError, match="predict_trajectory"):
        only_kp.predict(rgbs, pcds, grip, select="consensus", num_samples=3)
    with pytest.raises(TypeError):
        act.predict(rgbs, pcds, grip, None, mask, selekt="consensus")
    assert kp.calls == 0
