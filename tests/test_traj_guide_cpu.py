"""CPU-only tests of clearance-guided sampling (a3d_traj_guide, diffusion.guide_trajectories, compute_trajectory / Actioner.predict
with guide=...): self-checks of the float64 restatement in tests/traj_guide_ref.py on hand-computed cases, guided_segments, the two
C-ABI entries (export, header arity, every argument error without a device) and every host-side ValueError on CPU tensors before any
library call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import traj_guide_ref as GR
from conftest import ROOT, load_pkg
from test_actioner_cpu import _Keypose, _Planner, _obs

UNIT = np.float32([[-1, -1, -1], [1, 1, 1]])                        # bounds under which world == normalised, exactly


def signals_of(xyz, D=9):
    """(G, L, 3) -> (1, G, L, D) fp32 signals with channels 3.. set to a pattern that must survive"""
    xyz = np.asarray(xyz, dtype=np.float32)
    rest = np.broadcast_to(np.arange(3, D, dtype=np.float32) + 0.5, xyz.shape[:-1] + (D - 3,))
    return np.concatenate([xyz, rest], -1)[None]


def cloud_of(points):
    """(N, 3) -> (1, 1, 3, 1, N) fp32, channel-planar"""
    return np.asarray(points, dtype=np.float32).T.reshape(1, 1, 3, 1, -1)


def step(X, S, mask=None, **kw):
    mask = np.zeros((1, X.shape[2]), dtype=bool) if mask is None else mask
    kw.setdefault("skip", (0, 0))
    return GR.guide_ref(X, mask, kw.pop("cond_mask", None), kw.pop("bounds", UNIT), S, kw.pop("scene_mask", None), **kw)


# ------------------------------------------------------------------------------------------------ the restatement
def test_one_point_push_one_lands_on_the_margin_sphere():
    X = signals_of([[[0.5, 0, 0.03], [0.5, 0.04, 0], [0.9, 0, 0]]])
    S = cloud_of([[0.5, 0, 0]])
    ref = step(X, S, margin=0.05, push=1.0)
    s = np.float64(np.float32([0.5, 0, 0]))
    new_d = np.sqrt(((ref["x"][0, 0, :, :3] - s) ** 2).sum(-1))
    np.testing.assert_allclose(new_d[:2], 0.05, rtol=1e-12)                       # rows 0 and 1 were 3 and 4 cm away
    np.testing.assert_allclose(ref["nearest"][0, 0], [np.float64(np.float32(0.03)), np.float64(np.float32(0.04)), 0.4], rtol=1e-7)
    assert np.array_equal(ref["x"][0, 0, 2], X[0, 0, 2].astype(np.float64))       # 40 cm away: untouched
    assert np.array_equal(ref["x"][..., 3:], X[..., 3:].astype(np.float64))       # channels 3.. are never written
    assert ref["pushed"].tolist() == [[[True, True, False]]] and ref["index"][0, 0].tolist() == [0, 0, 0]
    # the direction is away from the point, along the line through it
    np.testing.assert_allclose(ref["x"][0, 0, 0, :3], [0.5, 0, 0.05], atol=1e-9)
    # push 0.5 goes half of the way, in bounds other than the unit box the update is scaled by 2 / (hi - lo)
    half = step(X, S, margin=0.05, push=0.5)
    np.testing.assert_allclose(half["x"][0, 0, 0, 2], (np.float64(np.float32(0.03)) + 0.05) / 2, rtol=1e-12)
    bounds = np.float32([[-1, -2, 0], [1, 2, 0.5]])                               # world z = (x + 1) / 2 * 0.5
    Xb = signals_of([[[0.5, 0, -0.75]]])                                          # world (0.5, 0, 0.0625)
    rb = step(Xb, cloud_of([[0.5, 0, 0]]), bounds=bounds, margin=0.125, push=1.0)
    assert rb["nearest"][0, 0, 0] == 0.0625 and rb["x"][0, 0, 0, 2] == -0.75 + 0.0625 * 2 / 0.5       # all exact in binary


def test_a_point_exactly_at_the_margin_d_zero_and_no_counted_point_do_not_move():
    X = signals_of([[[0, 0, 0.5], [0, 0, 0], [0, 0, 0.25]]])
    S = cloud_of([[0, 0, 0]])
    ref = step(X, S, margin=0.5, push=1.0)
    assert ref["nearest"][0, 0].tolist() == [0.5, 0.0, 0.25]
    assert np.array_equal(ref["x"][0, 0, :2], X[0, 0, :2].astype(np.float64))     # d == margin: hinge 0; d == 0: no direction
    assert ref["x"][0, 0, 2, 2] == 0.5 and ref["pushed"][0, 0].tolist() == [False, False, True]
    # all points masked, or broken: +inf, nothing moves, smoothing still acts
    sm = np.ones((1, 1, 1, 1), dtype=bool)
    for kw in (dict(scene_mask=sm), dict()):
        S2 = S if kw else cloud_of([[np.nan, 0, 0]])
        r = step(X, S2, margin=0.5, push=1.0, **kw)
        assert np.isposinf(r["nearest"]).all() and np.array_equal(r["x"], X.astype(np.float64)) and not r["pushed"].any()
        assert (r["index"] == -1).all()
    r = step(X, S, margin=0.5, push=1.0, smooth=1.0, scene_mask=sm)
    assert r["x"][0, 0, 1, 2] == 0.375 and np.array_equal(r["x"][0, 0, [0, 2]], X[0, 0, [0, 2]].astype(np.float64))


def test_the_skips_can_eat_every_row_and_padded_rows_keep_their_values():
    X = signals_of([[[0, 0, 0.01], [0, 0, 0.02], [0, 0, 0.03]]])
    S = cloud_of([[0, 0, 0]])
    assert step(X, S, push=1.0)["pushed"].all()
    for skip in ((2, 1), (1, 2), (3, 0), (0, 3), (5, 5)):
        r = step(X, S, push=1.0, smooth=0.5, skip=skip)
        assert np.array_equal(r["x"], X.astype(np.float64)) and not r["free"].any(), skip
        assert np.isfinite(r["nearest"]).all()                                    # nearest is reported for every valid row
    r = step(X, S, push=1.0, skip=(1, 1))
    assert r["free"][0, 0].tolist() == [False, True, False]
    # a scene without a valid row
    r = step(X, S, mask=np.ones((1, 3), dtype=bool), push=1.0)
    assert np.isposinf(r["nearest"]).all() and np.array_equal(r["x"], X.astype(np.float64))
    # pinned rows do not move
    cm = np.zeros((1, 3, 9), dtype=np.uint8)
    cm[0, 1] = 1
    r = step(X, S, push=1.0, cond_mask=cm)
    assert r["free"][0, 0].tolist() == [True, False, True] and r["x"][0, 0, 1, 2] == np.float64(np.float32(0.02))


def test_a_nan_row_stays_and_a_nan_neighbour_switches_the_smoothing_off():
    X = signals_of([[[0, 0, 0.01], [0, 0, 0.2], [np.nan, 0, 0.03], [0, 0, 0.3], [0, 0, 0.5], [0, 0, 0.6]]])
    S = cloud_of([[0, 0, 0]])
    r = step(X, S, margin=0.05, push=1.0, smooth=0.5)
    assert np.isnan(r["nearest"][0, 0, 2]) and not r["free"][0, 0, 2]
    got, was = r["x"][0, 0], X[0, 0].astype(np.float64)
    assert np.isnan(got[2, 0]) and np.array_equal(got[2, 1:], was[2, 1:])         # the NaN row keeps its values
    assert np.array_equal(got[1], was[1]) and np.array_equal(got[3], was[3])      # its neighbours: v = 0 (and they are clear)
    assert got[4, 2] == was[4, 2] + 0.5 * ((was[3, 2] + was[5, 2]) / 2 - was[4, 2])
    np.testing.assert_allclose(got[0, 2], 0.05, rtol=1e-12)                       # row 0: no previous row, pushed only


def test_an_exact_tie_goes_to_the_lower_index_in_both_storage_orders():
    X = signals_of([[[0, 0, 0]]])
    a, b = [0.25, 0, 0], [0, 0.25, 0]                                             # both exactly 0.25 away
    for pts, want in (([a, b], a), ([b, a], b)):
        r = step(X, cloud_of(pts), margin=0.5, push=1.0)
        assert r["index"][0, 0, 0] == 0 and r["nearest"][0, 0, 0] == 0.25
        assert np.array_equal(r["x"][0, 0, 0, :3], -np.float64(want))             # pushed 0.25 away from the FIRST point
        assert len(r["alts"]) == 1 and r["alts"][(0, 0, 0)].shape == (2, 3)       # ... and the tie is reported
    # the index is the kernel's: camera-major, n = c n_pix + pixel, masked points keep their slot
    S = np.zeros((1, 2, 3, 1, 2), dtype=np.float32)
    S[0, 0, :, 0, 0], S[0, 0, :, 0, 1], S[0, 1, :, 0, 0], S[0, 1, :, 0, 1] = [9, 9, 9], a, [9, 9, 9], b
    sm = np.zeros((1, 2, 1, 2), dtype=bool)
    assert step(X, S, margin=0.5, push=1.0)["index"][0, 0, 0] == 1
    sm[0, 0, 0, 1] = True
    assert step(X, S, margin=0.5, push=1.0, scene_mask=sm)["index"][0, 0, 0] == 3


def test_smoothing_a_kink_with_pinned_ends_and_a_scattered_mask():
    X = signals_of([[[0, 0, 0], [0.5, 0.5, 0], [1, 0, 0]]])
    S = cloud_of([[9, 9, 9]])
    cm = np.zeros((1, 3, 9), dtype=np.uint8)
    cm[0, 0] = cm[0, 2] = 1
    for smooth, want in ((1.0, [0.5, 0.0, 0]), (0.5, [0.5, 0.25, 0])):
        r = step(X, S, push=0.0, smooth=smooth, cond_mask=cm)
        assert r["x"][0, 0, 1, :3].tolist() == want                               # towards the midpoint of the pinned anchors
        assert np.array_equal(r["x"][0, 0, [0, 2]], X[0, 0, [0, 2]].astype(np.float64))
    # Jacobi: both inner rows move by the OLD positions of their neighbours
    X4 = signals_of([[[0, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0]]])
    r = step(X4, S, push=0.0, smooth=1.0)
    assert r["x"][0, 0, :, 1].tolist() == [0, -0.5, 0.5, 0]
    # a scattered mask: rows 1 and 3 are padded, the neighbours of row 2 are rows 0 and 4; padded rows keep whatever they hold
    X5 = signals_of([[[0, 0, 0], [7, 7, 7], [0.5, 0.5, 0], [np.nan, 7, 7], [1, 0, 0]]])
    mask = np.array([[False, True, False, True, False]])
    r = step(X5, S, mask=mask, push=0.0, smooth=1.0)
    assert r["x"][0, 0, 2, :3].tolist() == [0.5, 0.0, 0] and r["free"][0, 0].tolist() == [True, False, True, False, True]
    assert np.array_equal(r["x"][0, 0, [0, 4]], X5[0, 0, [0, 4]].astype(np.float64))      # the ends are free and have one neighbour: v = 0
    assert np.array_equal(r["x"][0, 0, 1], X5[0, 0, 1].astype(np.float64)) and np.isnan(r["x"][0, 0, 3, 0])
    assert np.isposinf(r["nearest"][0, 0, [1, 3]]).all()
    # the default skip (1, 1) over ranks: valid rows 0, 2, 4 -> only row 2 is free
    assert step(X5, S, mask=mask, push=0.0, smooth=1.0, skip=(1, 1))["free"][0, 0].tolist() == [False, False, True, False, False]
    assert not step(X5, S, mask=mask, push=0.0, smooth=1.0, skip=(2, 0))["free"][0, 0, 2]


def test_the_seeded_cases_meet_the_conditions_of_the_gpu_test():
    shape = (2, 4, 17, 3, 16, 16)
    P, mask, bounds, S, sm, cm = GR.make_inputs(0, *shape, 10, "scattered")
    assert cm.shape == (8, 17, 10) and cm.dtype == np.uint8 and (cm[:, 0] == 1).all() and 0.1 < cm.mean() < 0.6
    X = GR.signals_of(P, bounds)
    assert X.shape == (2, 4, 17, 10) and X.dtype == np.float32
    np.testing.assert_allclose(GR.world(X[..., :3], bounds), P[..., :3], atol=1e-6)
    ref = GR.guide_ref(X, mask, cm, bounds, S, sm, push=1.0, smooth=0.25)
    ties, n_push, d_min = GR.conditions(ref)
    assert n_push >= 5 and ties <= 0.02 * n_push and d_min >= 1e-4
    moved = (ref["x"] != X.astype(np.float64)).any(-1)
    assert not (moved & ~ref["free"]).any() and (moved & ref["free"]).sum() > n_push       # smoothing moves clear rows too
    bar = GR.row_bar(ref, bounds, GR.MARGIN, 1.0, 0.25)
    assert bar.shape == (2, 4, 17, 3) and 0 < bar[ref["free"]].max() < 1e-3


# ------------------------------------------------------------------------------------------------ guided_segments
def test_guided_segments():
    a3d = load_pkg()
    seg = a3d.guided_segments
    assert seg is a3d.diffusion.guided_segments
    assert seg(4, None) == [(0, 4, False)] and seg(0, None) == [(0, 0, False)]            # unguided: the one launch of before
    assert seg(4, 0) == seg(4, 0.0) == [(0, 1, True), (1, 1, True), (2, 1, True), (3, 1, True)]
    assert seg(4, 0.5) == [(0, 2, False), (2, 1, True), (3, 1, True)]
    assert seg(10, 0.5) == [(0, 5, False)] + [(i, 1, True) for i in range(5, 10)]
    assert seg(5, 0.5) == [(0, 2, False), (2, 1, True), (3, 1, True), (4, 1, True)]         # floor(2.5)
    for K in (2, 3, 4, 7, 10, 49, 100):
        assert seg(K, (K - 1) / K) == [(0, K - 1, False), (K - 1, 1, True)], K             # only the terminal step
        for i in range(K):
            assert seg(K, i / K)[-(K - i):] == [(j, 1, True) for j in range(i, K)] and len(seg(K, i / K)) == K - i + (i > 0)
    for start in (0, 0.5, 0.99):
        assert seg(1, start) == [(0, 1, True)]                                              # the terminal step always is
    assert seg(3, 0.999999) == [(0, 2, False), (2, 1, True)] and seg(0, 0.5) == []


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.mark.parametrize("name,arity", [("a3d_traj_guide_ws_floats", 5), ("a3d_traj_guide", 21)])
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
    assert "traj_guide.hip" in a3d.build.__globals__["SOURCES"]
    assert a3d.build.__globals__["EXTRA_FLAGS"]["traj_guide.hip"] == ["-Wall", "-Wextra"]


def test_workspace_size_without_a_device():
    a3d = load_pkg()
    lib = a3d.lib.load()
    ws, ws_clear = lib.a3d_traj_guide_ws_floats, lib.a3d_traj_clearance_ws_floats
    B, G, L = 2, 3, 5
    for chunks in (1, 3, 7):
        assert ws(B, G, L, 1000, chunks) == 2 * chunks * B * G * L              # a distance and an index per chunk and row
    for shape in ((1, 16, 50, 4 * 256 * 256), (24, 2, 50, 3 * 128 * 128), (1, 1, 1, 1)):
        b, g, l, n = shape
        assert ws(b, g, l, n, 0) == 2 * (ws_clear(b, g, l, n, 0) - b * l)         # the chunk count of the clearance pass
    assert ws(0, G, L, 10, 0) == 0 and ws(B, G, L, 10, -1) == 0


def test_traj_guide_rejects_bad_arguments_without_a_device():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    d = ctypes.c_void_p(64)                                         # aligned, never dereferenced
    call = lib.a3d_traj_guide

    def args(**kw):
        a = dict(traj=d, D=10, tmask=d, cmask=d, bounds=d, scene=d, smask=d, n_cam=2, n_pix=64, margin=0.05, sh=1, st=1, push=1.0,
                 smooth=0.0, nearest=d, ws=d, n_chunks=0, B=2, G=3, L=16)
        a.update(kw)
        return list(a.values()) + [None]

    def refused(**kw):
        assert call(*args(**kw)) == -22, kw
        assert b"a3d_traj_guide" in lib.a3d_last_error_string(), kw

    for name in ("traj", "tmask", "bounds", "scene", "ws"):         # the required pointers (cond_mask, scene_mask, nearest may be NULL)
        refused(**{name: None})
    for name in ("B", "G", "L", "n_cam", "n_pix"):
        for v in (0, -1):
            refused(**{name: v})
    refused(G=65)
    refused(L=257)
    for v in (7, 8, 11, 0):
        refused(D=v)
    for v in (0.0, -0.05, float("nan"), float("inf")):
        refused(margin=v)
    refused(sh=-1)
    refused(st=-1)
    refused(n_chunks=-1)
    for name in ("push", "smooth"):
        for v in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
            refused(**{name: v, "smooth" if name == "push" else "push": 0.5})
    refused(push=0.0, smooth=0.0)
    refused(B=65536)


# ------------------------------------------------------------------------------------------------ host-side ValueErrors
def test_exports_and_unchanged_names():
    a3d = load_pkg()
    D = a3d.diffusion
    assert a3d.guide_trajectories is D.guide_trajectories and a3d.Guidance is D.Guidance
    assert a3d.Guidance._fields == ("steps", "nearest") and D.GUIDE_MAX_ROWS == 256 and D.GUIDE_KEYS == ("push", "smooth", "start")
    assert "guide" in a3d.actioner._TRAJ_KW
    for kw in ("scene_mask", "clear_margin", "clear_skip", "select", "num_samples"):
        assert kw in a3d.actioner._TRAJ_KW
    # check_select / check_scene_select do not learn anything from the guide
    assert D.check_select("shortest") == [0.0, 0.0, 0.0, 1.0, 0.0] and D.check_select({"smooth": 2, "bounds": 0.5}) == [0.0, 0.0, 2.0, 0.0, 0.5]
    assert D.check_scene_select("clear") == ([0.0] * 5, 1.0)
    assert D.check_scene_select({"consensus": 1, "clearance": 5}) == ([1.0, 0.0, 0.0, 0.0, 0.0], 5.0)
    for bad in ("clear", {"clearance": 1.0}, {"push": 1.0}, "guide", {}):
        with pytest.raises(ValueError):
            D.check_select(bad)
    for bad in ({"clearance": 1, "push": 1.0}, "guide", {"guide": 1.0}):
        with pytest.raises(ValueError):
            D.check_scene_select(bad)
    assert D.RANK_TERMS == ("consensus", "goal", "smooth", "length", "bounds")


def test_check_guide_parses_numbers_and_dicts():
    D = load_pkg().diffusion
    assert D.check_guide(None) is None
    assert D.check_guide(1) == (1.0, 0.0, 0.5) and D.check_guide(0.25) == (0.25, 0.0, 0.5)
    assert D.check_guide({}) == (1.0, 0.0, 0.5)
    assert D.check_guide({"push": 0, "smooth": 0.5, "start": 0}) == (0.0, 0.5, 0.0)
    assert D.check_guide({"start": 0.75}) == (1.0, 0.0, 0.75)
    bad = [0, 0.0, -0.5, 1.5, float("nan"), float("inf"), True, "1", (1.0,), [1.0], {"push": 0}, {"push": 0, "smooth": 0},
           {"push": 2}, {"push": -1}, {"smooth": 1.01}, {"smooth": float("nan")}, {"push": "1"}, {"push": True}, {"start": 1},
           {"start": 1.0}, {"start": -0.1}, {"start": float("nan")}, {"start": "0.5"}, {"start": True}, {"margin": 0.05},
           {"push": 1, "steps": 3}]
    for g in bad:
        with pytest.raises(ValueError):
            D.check_guide(g)


def test_guide_trajectories_value_errors_before_any_library_call():
    a3d = load_pkg()
    z = torch.zeros
    B, G, L, Dn = 2, 3, 5, 10
    X, m, S, sm = z(B, G, L, Dn), z(B, L, dtype=torch.bool), z(B, 2, 3, 4, 4), z(B, 2, 4, 4, dtype=torch.bool)
    bounds = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    cm = z(B * G, L, Dn, dtype=torch.uint8)
    bad = [dict(signals=z(B, G, L, 8)), dict(signals=z(B, G, L, 11)), dict(signals=z(L, Dn)), dict(signals=z(1, B, G, L, Dn)),
           dict(signals=[[0.0]]), dict(signals=z(B, 65, L, Dn)), dict(signals=z(B, 0, L, Dn)),
           dict(signals=z(B, G, 257, Dn), trajectory_mask=z(B, 257, dtype=torch.bool)),
           dict(signals=z(B, G, L, Dn, dtype=torch.float64)), dict(signals=z(B, G, L, Dn + 1)[..., :Dn]),
           dict(trajectory_mask=z(B, L + 1, dtype=torch.bool)), dict(trajectory_mask=z(L, dtype=torch.bool)), dict(trajectory_mask=None),
           dict(scene=None), dict(scene=z(B, 2, 4, 4, 4)), dict(scene=z(B + 1, 2, 3, 4, 4)), dict(scene=z(B, 16, 4)),
           dict(scene=z(B, 2, 3, 4, 4, dtype=torch.long)),
           dict(scene_mask=z(B, 2, 4, 5, dtype=torch.bool)), dict(scene_mask=z(B, 2, 4, 4)), dict(scene=z(B, 16, 3), scene_mask=sm),
           dict(cond_mask=z(B * G, L, Dn)), dict(cond_mask=z(B * G, L, dtype=torch.uint8)), dict(cond_mask=z(B, L, Dn, dtype=torch.uint8)),
           dict(cond_mask=[0]),
           dict(bounds=torch.zeros(3, 2)), dict(bounds=[[0.0, 0, 0]]),
           dict(margin=0), dict(margin=-0.05), dict(margin=float("nan")), dict(margin=float("inf")), dict(margin="0.05"),
           dict(skip=1), dict(skip=(1,)), dict(skip=(-1, 1)), dict(skip=(1.0, 1)), dict(skip=None),
           dict(push=-0.1), dict(push=1.1), dict(push=float("nan")), dict(push="1"), dict(push=True), dict(push=0.0),
           dict(smooth=-0.1), dict(smooth=1.1), dict(smooth=float("inf")), dict(smooth=None), dict(push=0, smooth=0)]
    for kw in bad:
        a = dict(signals=X, trajectory_mask=m, scene=S, bounds=bounds, scene_mask=sm, cond_mask=cm, margin=0.05, skip=(1, 1), push=1.0,
                 smooth=0.0)
        a.update(kw)
        sig, tm, sc, bd = a.pop("signals"), a.pop("trajectory_mask"), a.pop("scene"), a.pop("bounds")
        with pytest.raises(ValueError):
            a3d.guide_trajectories(sig, tm, sc, bd, **a)
    with pytest.raises(TypeError):
        a3d.guide_trajectories(X, m, S, bounds, sm)                                # the options are keyword-only
    # valid arguments on CPU tensors get as far as the device check: there is no CPU fallback
    for kw in (dict(), dict(scene_mask=sm, cond_mask=cm, smooth=0.5, want_nearest=True), dict(cond_mask=cm.bool().view(B, G, L, Dn))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            a3d.guide_trajectories(X, m, S, bounds, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a3d.guide_trajectories(z(B, L, 9), m, z(B, 16, 3), [[-1, -1, -1], [1, 1, 1]], scene_mask=z(B, 16, dtype=torch.uint8))
    assert not X.any()


def test_compute_trajectory_guide_raises_before_any_launch():
    a3d = load_pkg()
    m = a3d.DiffusionPlanner(embedding_dim=60, num_attn_heads=4, num_query_cross_attn_layers=6, use_instruction=True, use_goal=True,
                             gripper_loc_bounds=[[-1, -1, -1], [1, 1, 1]], rotation_parametrization="6D", diffusion_timesteps=100)
    assert m.last_guidance is None
    B, Ln = 2, 8
    mask = torch.zeros(B, Ln, dtype=torch.bool)
    args = (mask, None, torch.zeros(B, 1, 3, 16, 16), torch.zeros(B, 53, 512), torch.zeros(B, 8), torch.zeros(B, 8))
    bad = [dict(guide=0), dict(guide=1.5), dict(guide=-1), dict(guide=float("nan")), dict(guide="1"), dict(guide=True),
           dict(guide={"push": 0}), dict(guide={"start": 1.0}), dict(guide={"start": -0.5}), dict(guide={"strength": 1.0}),
           dict(guide={"smooth": 2}), dict(guide=1.0, num_samples=65),
           dict(guide=1.0, scene_mask=torch.zeros(B, 1, 16, 15, dtype=torch.bool)), dict(guide=1.0, scene_mask=torch.zeros(B, 1, 16, 16)),
           dict(guide=1.0, clear_margin=0.0), dict(guide=1.0, clear_margin=float("nan")), dict(guide=1.0, clear_skip=(1,)),
           dict(guide=1.0, clear_skip=(-1, 0)), dict(guide=1.0, num_inference_steps=0), dict(guide=1.0, select="clear")]
    for kw in bad:
        with pytest.raises(ValueError):
            m.compute_trajectory(*args, **kw)
        with pytest.raises(ValueError):
            m(None, *args, run_inference=True, **kw)
    long_mask = torch.zeros(B, 257, dtype=torch.bool)
    with pytest.raises(ValueError, match="256"):
        m.compute_trajectory(long_mask, *args[1:], guide=1.0)
    with pytest.raises(ValueError):
        m.compute_trajectory(mask, None, torch.zeros(B, 1, 4, 16, 16), *args[3:], guide=1.0)         # not a cloud
    assert m.last_guidance is None and m.last_ranking is None


def test_actioner_predict_guide_raises_before_any_launch():
    a3d = load_pkg()
    rgbs, pcds, grip = _obs()
    mask = torch.zeros(2, 8, dtype=torch.bool)
    kp, pl = _Keypose(), _Planner()
    act = a3d.Actioner(kp, pl, predict_keypose=True, predict_trajectory=True)
    act.set_instruction(torch.zeros(1, 53, 512))
    B, _, ncam, _, H, W = pcds.shape
    bad = [dict(guide=0), dict(guide=2.0), dict(guide={"push": 1, "start": 1}), dict(guide={"weight": 1}), dict(guide="on"),
           dict(guide=1.0, num_samples=0), dict(guide=1.0, num_samples=65),
           dict(guide=1.0, scene_mask=torch.zeros(B, ncam, H, W + 1, dtype=torch.bool)), dict(guide=1.0, scene_mask=torch.zeros(B, ncam, H, W)),
           dict(guide=1.0, clear_margin=-0.1), dict(guide=1.0, clear_skip=(1, 1, 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            act.predict(rgbs, pcds, grip, None, mask, **kw)
    with pytest.raises(ValueError):
        act.predict(rgbs, pcds, grip, None, torch.zeros(2, 257, dtype=torch.bool), guide=1.0)
    with pytest.raises(ValueError):
        a3d.Actioner(kp, pl, predict_keypose=True, predict_trajectory=False).predict(rgbs, pcds, grip, None, None, guide=1.0)
    with pytest.raises(TypeError):
        act.predict(rgbs, pcds, grip, None, mask, guide=1.0, push=1.0)                               # the dict's keys, not keywords
    assert kp.calls == 0
