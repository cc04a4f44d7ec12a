"""CPU-only tests of the body-aware swept clearance (a3d_traj_body_clearance, trajectory.body_clearance, rank_trajectories(body=),
compute_trajectory / Actioner.predict with clear_body=): self-checks of the float64 restatement in tests/traj_body_ref.py on
hand-computed cases, the two C-ABI entries (export, header arity, every argument error without a device: the non-NULL pointers are
dummies that are never dereferenced) and every host-side ValueError on CPU tensors before any library call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import traj_body_ref as Bd
import traj_clearance_ref as C
import traj_rank_ref as R
from conftest import ROOT, load_pkg
from test_actioner_cpu import _Keypose, _Planner, _obs

ID = [1.0, 0.0, 0.0, 0.0]
QZ90 = [math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5)]                    # a quarter turn about z


def poses_of(xyz, quat=None):
    """(G, L, 3) -> (1, G, L, 7) fp32; quat: one quaternion for every row, or (G, L, 4); identity by default"""
    xyz = np.asarray(xyz, dtype=np.float32)
    q = np.broadcast_to(np.asarray(ID if quat is None else quat, dtype=np.float32), xyz.shape[:-1] + (4,))
    return np.concatenate([xyz, q], -1)[None]


def cloud_of(points):
    """(N, 3) -> (1, 1, 3, 1, N) fp32, channel-planar"""
    return np.asarray(points, dtype=np.float32).T.reshape(1, 1, 3, 1, -1)


def body(offsets=((0, 0, 0),), radii=(0,)):
    return np.asarray(offsets, dtype=np.float32).reshape(-1, 3), np.asarray(radii, dtype=np.float32)


NOMASK = lambda L: np.zeros((1, L), dtype=bool)  # noqa: E731


# ------------------------------------------------------------------------------------------------ the restatement
def test_a_point_beside_the_middle_beyond_an_end_and_a_degenerate_segment():
    P = poses_of([[[0, 0, 0], [2, 0, 0], [2, 0, 0]]])
    o, r = body()
    # beside the middle of the first segment: interior t = 1/2, distance 0.25; the unswept term sees the ends only
    near, _ = Bd.body_ref(P, NOMASK(3), cloud_of([[1, 0.25, 0]]), o, r, 1, skip=(0, 0))
    assert near[0, 0, 0] == 0.25
    assert near[0, 0, 1] == near[0, 0, 2] == math.sqrt(1 + 0.0625)        # row 1 -> row 2 does not move: a degenerate segment
    point, _ = C.clearance_ref(P, NOMASK(3), cloud_of([[1, 0.25, 0]]), skip=(0, 0))
    assert point[0, 0, 0] == math.sqrt(1 + 0.0625)
    # beyond the far end (t clamped to 1) and before the near end (t clamped to 0)
    near, _ = Bd.body_ref(P, NOMASK(3), cloud_of([[2.5, 0, 0]]), o, r, 1, skip=(0, 0))
    assert near[0, 0, 0] == 0.5
    near, _ = Bd.body_ref(P, NOMASK(3), cloud_of([[-0.5, 0, 0]]), o, r, 1, skip=(0, 0))
    assert near[0, 0, 0] == 0.5 and near[0, 0, 1] == 2.5
    # without sweep every row is its own degenerate segment
    near, _ = Bd.body_ref(P, NOMASK(3), cloud_of([[1, 0.25, 0]]), o, r, 0, skip=(0, 0))
    assert np.array_equal(near, point)
    assert Bd.segment_dist([0, 0, 0], [0, 0, 0], np.array([[0.0, 3.0, 4.0]])) == 5.0


def test_a_quarter_turn_about_z_carries_the_offset():
    Rz = Bd.rotation(np.float32(QZ90))
    np.testing.assert_allclose(Rz @ [1, 0, 0], [0, 1, 0], atol=1e-7)      # fp32 storage of sqrt(1/2)
    np.testing.assert_allclose(Rz @ [0, 1, 0], [-1, 0, 0], atol=1e-7)
    np.testing.assert_allclose(Rz @ [0, 0, 1], [0, 0, 1], atol=1e-7)
    assert np.array_equal(Bd.rotation(ID), np.eye(3)) and np.array_equal(Bd.rotation([-3.0, 0, 0, 0]), np.eye(3))    # any norm, either sign
    q = np.random.default_rng(0).normal(size=(5, 4))
    Rq = Bd.rotation(q)
    np.testing.assert_allclose(Rq @ Rq.transpose(0, 2, 1), np.broadcast_to(np.eye(3), (5, 3, 3)), atol=1e-14)
    np.testing.assert_allclose(np.linalg.det(Rq), 1.0, atol=1e-14)
    # the first two columns are the six numbers pose_to_signal emits (R.unit_quat normalises the same way)
    w, x, y, z = R.unit_quat(q).T
    np.testing.assert_allclose(Rq[:, :, 0], np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)], -1), atol=1e-14)
    np.testing.assert_allclose(Rq[:, :, 1], np.stack([2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)], -1), atol=1e-14)
    # one sphere at (1, 0, 0) of the tool frame, the tool at the origin turned by a quarter: the sphere's centre is (0, 1, 0)
    o, r = body([(1, 0, 0)])
    near, _ = Bd.body_ref(poses_of([[[0, 0, 0]]], QZ90), NOMASK(1), cloud_of([[0, 1.5, 0]]), o, r, 1, skip=(0, 0))
    np.testing.assert_allclose(near[0, 0, 0], 0.5, atol=1e-7)
    near, _ = Bd.body_ref(poses_of([[[0, 0, 0]]]), NOMASK(1), cloud_of([[0, 1.5, 0]]), o, r, 1, skip=(0, 0))
    np.testing.assert_allclose(near[0, 0, 0], math.sqrt(1 + 2.25), rtol=1e-15)


def test_a_radius_larger_than_the_distance_is_negative_and_the_hinge_exceeds_one():
    P = poses_of([[[0, 0, 0], [0, 0, 0]]])
    o, r = body([(0, 0, 0), (0, 0, 1)], [0.75, 0.25])
    near, clear = Bd.body_ref(P, NOMASK(2), cloud_of([[0.5, 0, 0]]), o, r, 1, margin=0.5, skip=(0, 0))
    assert near[0, 0, 0] == -0.25 == near[0, 0, 1]                        # min over the spheres: 0.5 - 0.75 against sqrt(1.25) - 0.25
    assert clear[0, 0] == 1.5 and clear[0, 0] <= 1 + 0.75 / 0.5           # (0.5 + 0.25) / 0.5: not clamped above
    o, r = body([(0, 0, 0)], [0.5])
    near, clear = Bd.body_ref(P, NOMASK(2), cloud_of([[0.5, 0, 0]]), o, r, 0, margin=0.5, skip=(0, 0))
    assert near[0, 0, 0] == 0.0 and clear[0, 0] == 1.0                    # touching


def test_the_end_row_rule_with_skip_tail_0_1_2_and_a_mask_with_gaps():
    mask = np.zeros(5, dtype=bool)
    for st, want_end, want_scored in ((0, [1, 2, 3, 4, 4], [0, 1, 1, 1, 1]), (1, [1, 2, 3, 3, 4], [0, 1, 1, 1, 0]),
                                      (2, [1, 2, 2, 3, 4], [0, 1, 1, 0, 0])):
        idx, end, scored = Bd.end_rows(mask, 1, (1, st))
        assert list(idx) == [0, 1, 2, 3, 4] and list(end) == want_end and list(scored.astype(int)) == want_scored, st
        assert list(Bd.end_rows(mask, 0, (1, st))[1]) == [0, 1, 2, 3, 4]
    # gaps are stepped over: the valid rows 0, 2, 3, 6 have ranks 0 .. 3
    gaps = np.array([0, 1, 0, 0, 1, 1, 0, 1], dtype=bool)
    idx, end, scored = Bd.end_rows(gaps, 1, (1, 1))
    assert list(idx) == [0, 2, 3, 6] and list(end) == [2, 3, 3, 6] and list(scored.astype(int)) == [0, 1, 1, 0]
    assert list(Bd.end_rows(gaps, 1, (0, 0))[1]) == [2, 3, 6, 6]
    assert [len(x) for x in Bd.end_rows(np.ones(3, dtype=bool), 1, (1, 1))] == [0, 0, 0]
    assert list(Bd.end_rows(np.zeros(1, dtype=bool), 1, (0, 0))[1]) == [0]
    # in numbers: rows along x at 0, (padded), 2, 3; a point beside x = 1 is seen by the segment row 0 -> row 2 only
    P = poses_of([[[0, 0, 0], [50, 50, 50], [2, 0, 0], [3, 0, 0]]])
    o, r = body()
    S = cloud_of([[1, 0.25, 0]])
    near, clear = Bd.body_ref(P, np.array([[0, 1, 0, 0]], dtype=bool), S, o, r, 1, margin=0.5, skip=(0, 0))
    assert near[0, 0, 0] == 0.25 and np.isposinf(near[0, 0, 1])
    assert near[0, 0, 2] == math.sqrt(1 + 0.0625) and near[0, 0, 3] == math.sqrt(4 + 0.0625)
    assert clear[0, 0] == (0.5 + 0 + 0) / 3
    # skip_tail = 1: the approach to the last valid row is not swept (n - skip_tail = 2, so only rank 0 steps)
    near1, _ = Bd.body_ref(P, np.array([[0, 1, 0, 0]], dtype=bool), cloud_of([[2.5, 0.25, 0]]), o, r, 1, margin=0.5, skip=(0, 1))
    assert near1[0, 0, 2] == math.sqrt(0.25 + 0.0625)                     # row 2 alone, not the segment to row 3
    near0, _ = Bd.body_ref(P, np.array([[0, 1, 0, 0]], dtype=bool), cloud_of([[2.5, 0.25, 0]]), o, r, 1, margin=0.5, skip=(0, 0))
    assert near0[0, 0, 2] == 0.25


def test_every_point_masked_a_nan_row_and_a_zero_quaternion():
    P = poses_of([[[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]]] * 2)
    o, r = body([(0, 0, 0), (0.1, 0, 0)], [0.0, 0.01])
    S = cloud_of([[1, 0.25, 0], [np.nan, 0, 0], [0, np.inf, 0]])
    sm = np.zeros((1, 1, 1, 3), dtype=bool)
    sm[..., 0] = True
    near, clear = Bd.body_ref(P, NOMASK(5), S, o, r, 1, sm)
    assert np.isposinf(near).all() and (clear == 0).all()                 # no counted point: +inf, the hinge is 0
    # a NaN row poisons itself and, through e(j), the row before it -- and only that one
    Pn = P.copy()
    Pn[0, 0, 3, 1] = np.nan
    near, clear = Bd.body_ref(Pn, NOMASK(5), S, o, r, 1, skip=(0, 0))
    assert list(np.isnan(near[0, 0])) == [False, False, True, True, False] and np.isfinite(near[0, 1]).all()
    assert np.isnan(clear[0, 0]) and np.isfinite(clear[0, 1])
    near, clear = Bd.body_ref(Pn, NOMASK(5), S, o, r, 0, skip=(0, 0))
    assert list(np.isnan(near[0, 0])) == [False, False, False, True, False]
    near, clear = Bd.body_ref(Pn, NOMASK(5), S, o, r, 1, skip=(0, 2))     # ranks 3 and 4 are skipped: 2 -> 3 is not a segment
    assert list(np.isnan(near[0, 0])) == [False, False, False, True, False] and np.isfinite(clear).all()
    # a NaN in the quaternion does the same; the opening (channel 7) is never read
    Pq = np.concatenate([P, np.full(P.shape[:-1] + (1,), np.nan, dtype=np.float32)], -1)
    assert np.isfinite(Bd.body_ref(Pq, NOMASK(5), S, o, r, 1)[0]).all()
    Pq[0, 1, 1, 5] = np.inf
    assert list(np.isnan(Bd.body_ref(Pq, NOMASK(5), S, o, r, 1, skip=(0, 0))[0][0, 1])) == [True, True, False, False, False]
    # a zero quaternion: R is not finite, the row is NaN -- with a zero offset too (0 * NaN)
    Pz = P.copy()
    Pz[0, 1, 2, 3:7] = 0
    assert not np.isfinite(Bd.rotation(np.zeros(4))).any()
    for bd_ in ((o, r), body()):
        near, _ = Bd.body_ref(Pz, NOMASK(5), S, *bd_, 0, skip=(0, 0))
        assert list(np.isnan(near[0, 1])) == [False, False, True, False, False] and np.isfinite(near[0, 0]).all()


@pytest.mark.parametrize("mask_kind", R.MASKS)
def test_the_trivial_body_is_the_point_term_exactly(mask_kind):
    P, mask, goal, bounds, S, sm = C.make_inputs(3, 2, 4, 17, 3, 16, 16, 8, mask_kind)
    for skip in ((1, 1), (0, 0), (2, 3)):
        for m in (None, sm):
            want = C.clearance_ref(P, mask, S, m, skip=skip)
            got = Bd.body_ref(P, mask, S, *Bd.TRIVIAL, m, skip=skip)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (mask_kind, skip)
    ref = Bd.body_rank_ref(P, mask, goal, bounds, C.RULE, S, *Bd.TRIVIAL, sm)
    want = C.scene_rank_ref(P, mask, goal, bounds, C.RULE, S, sm)
    assert np.array_equal(ref["scores"], want["scores"]) and np.array_equal(ref["order"], want["order"])


def test_the_seeded_cases_are_not_trivial_and_the_finder_agrees_with_the_table():
    shape = (2, 4, 17, 3, 3, 16, 16)
    P, mask, goal, bounds, S, sm, o, r = Bd.make_inputs(0, *shape, 8, "scattered")
    assert o.shape == (3, 3) and o.dtype == np.float32 and r.shape == (3,) and (np.abs(o) <= 0.08).all() and (r >= 0).all() and (r <= 0.03).all()
    swept = Bd.body_rank_ref(P, mask, goal, bounds, C.RULE, S, o, r, 1, sm)
    still = Bd.body_rank_ref(P, mask, goal, bounds, C.RULE, S, o, r, 0, sm)
    fin = np.isfinite(swept["nearest"])
    assert (swept["nearest"][fin] <= still["nearest"][fin]).all() and (swept["nearest"][fin] < still["nearest"][fin]).any()
    assert (swept["nearest"][fin] < 0).any() and (swept["clearance"] > 0.01).any()                    # a sphere contains a point somewhere
    np.testing.assert_allclose(swept["scores"], R.rank_ref(P, mask, goal, bounds, {"consensus": 1.0})["scores"] + 5.0 * swept["clearance"],
                               rtol=1e-15)
    assert Bd.find_seed(*shape, 8, "scattered", True, 1, tries=3) == 0
    assert 1e-5 < Bd.nearest_bar(P, S, o) < 1e-4 and Bd.ROUNDINGS == 72


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.mark.parametrize("name,arity", [("a3d_traj_body_clearance_ws_floats", 6), ("a3d_traj_body_clearance", 22)])
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
    assert "traj_body.hip" in a3d.build.__globals__["SOURCES"]
    assert a3d.build.__globals__["EXTRA_FLAGS"]["traj_body.hip"] == ["-Wall", "-Wextra"]
    assert a3d.lib.TRAJ_BODY_MAX_SPHERES == 8 == a3d.trajectory.BODY_MAX_SPHERES and "#define A3D_TRAJ_BODY_MAX_SPHERES 8" in header


def test_workspace_size_without_a_device():
    ws = load_pkg().lib.load().a3d_traj_body_clearance_ws_floats
    B, G, L = 2, 3, 5
    for K in (1, 2, 8):
        for chunks in (1, 3, 7):
            assert ws(B, G, L, K, 1000, chunks) == chunks * B * G * K * L + 8 * B * G * K * L + 3 * B * L
    chosen = ws(1, 16, 50, 4, 4 * 256 * 256, 0) - 8 * 3200 - 150
    assert chosen % 3200 == 0 and 1 <= chosen // 3200 <= 4096
    assert ws(1, 16, 4, 8, 256, 0) > 0                                    # G K = 128 row groups
    for bad in ((0, G, L, 1, 10, 0), (B, 0, L, 1, 10, 0), (B, G, 0, 1, 10, 0), (B, G, L, 0, 10, 0), (B, G, L, 9, 10, 0), (B, G, L, 1, 0, 0),
                (B, G, L, 1, 10, -1), (B, 65, L, 1, 10, 0)):
        assert ws(*bad) == 0, bad


PTR = ctypes.c_void_p(256)                           # 256-byte aligned, never dereferenced
BASE = dict(poses=PTR, tmask=PTR, offsets=PTR, radii=PTR, K=3, sweep=1, scene=PTR, scene_mask=None, n_cam=1, n_pix=21, margin=0.05,
            skip_head=1, skip_tail=1, nearest=None, clearance=PTR, ws=PTR, n_chunks=0, B=1, G=2, L=5, Dp=8)
REFUSED = [
    # the shared checks of the scan plan, under this entry's name
    (dict(B=0), b"B, G and L must be positive"), (dict(G=0), b"B, G and L must be positive"), (dict(L=0), b"B, G and L must be positive"),
    (dict(n_cam=0), b"n_cam and n_pix must be positive"), (dict(n_pix=0), b"n_cam and n_pix must be positive"),
    (dict(G=65), b"G=65 exceeds 64 candidates per scene"),
    (dict(margin=0.0), b"margin must be finite and positive"), (dict(margin=math.nan), b"margin must be finite and positive"),
    (dict(margin=math.inf), b"margin must be finite and positive"), (dict(margin=-0.05), b"margin must be finite and positive"),
    (dict(skip_head=-1), b"negative skip"), (dict(skip_tail=-1), b"negative skip"),
    (dict(n_chunks=-1), b"n_chunks=-1 is negative"),
    (dict(n_cam=65536, n_pix=32768), b"n_cam * n_pix overflows int"),
    (dict(B=65536), b"B=65536 exceeds 65535 scenes per call"),
    (dict(B=65535, n_chunks=1 << 20), b"exceed the grid"),
    # its own
    (dict(K=0), b"K=0, a body has 1 to 8 spheres"), (dict(K=9), b"K=9, a body has 1 to 8 spheres"), (dict(K=-1), b"a body has 1 to 8 spheres"),
    (dict(sweep=2), b"sweep=2 must be 0 or 1"), (dict(sweep=-1), b"sweep=-1 must be 0 or 1"),
    (dict(Dp=6), b"Dp=6, pose rows have 7 or 8 channels"), (dict(Dp=9), b"pose rows have 7 or 8 channels"),
    (dict(G=64, K=8, L=1 << 19), b"G * K * L * 8 overflows int (G=64 K=8 L=524288)"),
    (dict(G=64, K=1, L=1 << 22), b"G * L * 8 overflows int"),
]


def _refused(lib, change, needle):
    a = dict(BASE, **change)
    assert lib.a3d_traj_body_clearance(*a.values(), None) == -22, change
    msg = lib.a3d_last_error_string()
    assert msg.startswith(b"a3d_traj_body_clearance:"), (change, msg)
    assert needle in msg, (change, msg)


def test_bad_arguments_are_refused_before_any_launch():
    lib = load_pkg().lib.load()
    assert list(BASE) == [n for n in load_pkg().lib.PARAM_NAMES["a3d_traj_body_clearance"][:-1]]      # the header's order
    for change, needle in REFUSED:
        _refused(lib, change, needle)
    for k in ("poses", "tmask", "offsets", "radii", "scene", "clearance", "ws"):                      # scene_mask and nearest may be NULL
        _refused(lib, {k: None}, b"null pointer (poses, tmask, offsets, radii, scene, clearance and ws are required)")
    _refused(lib, dict(B=0, poses=None), b"null pointer")                                             # the pointers come first
    # G K = 128 row groups pass the limit on candidates: the call is refused for another reason only
    _refused(lib, dict(G=16, K=8, Dp=6), b"pose rows have 7 or 8 channels")


# ------------------------------------------------------------------------------------------------ host-side ValueErrors
def test_exports():
    a3d = load_pkg()
    T, D = a3d.trajectory, a3d.diffusion
    for n in ("body_clearance", "check_body", "GripperBody"):
        assert getattr(a3d, n) is getattr(T, n) is getattr(D, n), n
    assert T.GripperBody._fields == ("offsets", "radii", "sweep") and T.GripperBody([[0, 0, 0]], [0]).sweep is True
    assert "clear_body" in a3d.actioner._TRAJ_KW
    assert not [n for n in dir(T) if "PRESET" in n and "BODY" in n]                                  # no preset body ships


def test_check_body_accepts_and_refuses():
    T = load_pkg().trajectory
    b = T.check_body(T.GripperBody([[0, 0, 0.1], [0.02, 0, 0]], [0.01, 0]))
    assert b.offsets.dtype == torch.float32 and tuple(b.offsets.shape) == (2, 3) and tuple(b.radii.shape) == (2,) and b.sweep is True
    b = T.check_body({"offsets": torch.zeros(8, 3, dtype=torch.float64), "radii": torch.ones(8), "sweep": False})
    assert b.offsets.dtype == torch.float32 and b.offsets.is_contiguous() and b.sweep is False
    assert T.check_body({"offsets": torch.zeros(4, 3).t().contiguous().t()[:1], "radii": [0.5]}).offsets.is_contiguous()
    assert T.check_body(T.GripperBody(np.zeros((1, 3)), np.zeros(1), 0)).sweep is False
    z = torch.zeros
    bad = [None, 3, ([[0, 0, 0]], [0]), {"offsets": z(1, 3)}, {"radii": z(1)}, {"offsets": z(1, 3), "radii": z(1), "speed": 1},
           T.GripperBody(z(3), z(1)), T.GripperBody(z(1, 4), z(1)), T.GripperBody(z(1, 1, 3), z(1)), T.GripperBody(z(0, 3), z(0)),
           T.GripperBody(z(9, 3), z(9)), T.GripperBody(z(2, 3), z(3)), T.GripperBody(z(2, 3), z(2, 1)), T.GripperBody(z(2, 3), 0.5),
           T.GripperBody(torch.tensor([[0.0, math.nan, 0.0]]), z(1)), T.GripperBody(torch.tensor([[0.0, math.inf, 0.0]]), z(1)),
           T.GripperBody(z(1, 3), torch.tensor([-0.01])), T.GripperBody(z(1, 3), torch.tensor([math.nan])),
           T.GripperBody(z(1, 3), torch.tensor([math.inf])), T.GripperBody(z(1, 3), z(1), 2), T.GripperBody(z(1, 3), z(1), None),
           T.GripperBody(z(1, 3), z(1), 1.0), T.GripperBody("abc", z(1)), T.GripperBody(z(1, 3, dtype=torch.bool), z(1)),
           T.GripperBody(z(1, 3), z(1, dtype=torch.complex64))]
    for x in bad:
        with pytest.raises(ValueError):
            T.check_body(x)


def test_body_clearance_and_rank_trajectories_value_errors_before_any_library_call():
    a3d = load_pkg()
    z = torch.zeros
    B, G, L = 2, 3, 5
    P, m, S, sm = z(B, G, L, 8), z(B, L, dtype=torch.bool), z(B, 2, 3, 4, 4), z(B, 2, 4, 4, dtype=torch.bool)
    ok_body = a3d.GripperBody(z(2, 3), z(2))
    bad = [dict(trajectories=z(B * G, L, 8)), dict(trajectories=z(B, G, L, 6)), dict(trajectories=z(B, 65, L, 8)),
           dict(trajectory_mask=z(B, L + 1, dtype=torch.bool)), dict(scene=None), dict(scene=z(B, 2, 4, 4, 4)),
           dict(scene_mask=z(B, 2, 4, 5, dtype=torch.bool)), dict(margin=0), dict(margin=float("nan")), dict(skip=(1,)), dict(skip=(-1, 1)),
           dict(body=None), dict(body=a3d.GripperBody(z(9, 3), z(9))), dict(body=a3d.GripperBody(z(2, 3), -torch.ones(2))),
           dict(body={"offsets": z(2, 3)})]
    for kw in bad:
        a = dict(trajectories=P, trajectory_mask=m, scene=S, body=ok_body, scene_mask=sm, margin=0.05, skip=(1, 1))
        a.update(kw)
        with pytest.raises(ValueError):
            a3d.body_clearance(**a)
    # rank_trajectories checks a body whatever the rule weighs
    for rule in ("consensus", {"consensus": 1, "clearance": 5}):
        with pytest.raises(ValueError):
            a3d.rank_trajectories(P, m, select=rule, scene=S, body=a3d.GripperBody(z(2, 3), z(3)))
    # valid arguments on CPU tensors get as far as the device check: there is no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a3d.body_clearance(P, m, S, ok_body, sm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a3d.rank_trajectories(P, m, select="clear", scene=S, body=ok_body)


def test_compute_trajectory_and_predict_check_the_body_before_any_launch():
    a3d = load_pkg()
    pl = a3d.DiffusionPlanner(embedding_dim=60, num_attn_heads=4, num_query_cross_attn_layers=6, use_instruction=True, use_goal=True,
                              gripper_loc_bounds=[[-1, -1, -1], [1, 1, 1]], rotation_parametrization="6D", diffusion_timesteps=100)
    B, Ln = 2, 8
    mask = torch.zeros(B, Ln, dtype=torch.bool)
    args = (mask, None, torch.zeros(B, 1, 3, 16, 16), torch.zeros(B, 53, 512), torch.zeros(B, 8), torch.zeros(B, 8))
    z = torch.zeros
    bad_bodies = [a3d.GripperBody(z(9, 3), z(9)), a3d.GripperBody(z(1, 3), torch.tensor([-1.0])), {"offsets": z(1, 3)}, 5]
    for bd_ in bad_bodies:
        for kw in (dict(select="clear", num_samples=3), dict(select="consensus", num_samples=3), dict()):
            with pytest.raises(ValueError):
                pl.compute_trajectory(*args, clear_body=bd_, **kw)
    assert pl.last_ranking is None
    rgbs, pcds, grip = _obs()
    kp, pl2 = _Keypose(), _Planner()
    act = a3d.Actioner(kp, pl2, predict_keypose=True, predict_trajectory=True)
    act.set_instruction(torch.zeros(1, 53, 512))
    for bd_ in bad_bodies:
        with pytest.raises(ValueError):
            act.predict(rgbs, pcds, grip, None, torch.zeros(2, 8, dtype=torch.bool), select="clear", num_samples=3, clear_body=bd_)
    with pytest.raises(TypeError):
        act.predict(rgbs, pcds, grip, None, torch.zeros(2, 8, dtype=torch.bool), select="clear", num_samples=3, body=bad_bodies[0])
    assert kp.calls == 0
