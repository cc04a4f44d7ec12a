"""Host side of the scene-cloud scan that a3d_traj_clearance and a3d_traj_guide share (csrc/traj_points.h: tc_scan_plan, the
workspace plane) and the module split that goes with it (trajectory.py next to diffusion.py).

Every call of an entry in this file is one the host refuses, so nothing is launched on a machine that has a GPU either: the non-NULL
pointers are dummies that are never dereferenced.  Each case changes ONE argument of a call that would otherwise be taken."""
import ctypes
import math

import pytest
import torch

from conftest import load_pkg

PTR = ctypes.c_void_p(256)                           # 256-byte aligned, never dereferenced
BASE = dict(poses=PTR, traj=PTR, tmask=PTR, cond_mask=None, bounds=PTR, scene=PTR, scene_mask=None, nearest=None, clearance=PTR, ws=PTR,
            n_cam=1, n_pix=21, margin=0.05, skip_head=1, skip_tail=1, n_chunks=0, B=1, G=2, L=5, Dp=8, D=10, push=1.0, smooth=0.0)
ORDER = {
    "a3d_traj_clearance": ("poses", "tmask", "scene", "scene_mask", "n_cam", "n_pix", "margin", "skip_head", "skip_tail", "nearest",
                           "clearance", "ws", "n_chunks", "B", "G", "L", "Dp"),
    "a3d_traj_guide": ("traj", "D", "tmask", "cond_mask", "bounds", "scene", "scene_mask", "n_cam", "n_pix", "margin", "skip_head",
                       "skip_tail", "push", "smooth", "nearest", "ws", "n_chunks", "B", "G", "L"),
}
REQUIRED = {"a3d_traj_clearance": ("poses", "tmask", "scene", "clearance", "ws"), "a3d_traj_guide": ("traj", "tmask", "bounds", "scene", "ws")}
names = pytest.mark.parametrize("name", sorted(ORDER))

# the checks of the shared plan: one bad argument -> what the message says
SHARED = [
    (dict(B=0), b"B, G and L must be positive"), (dict(G=0), b"B, G and L must be positive"), (dict(L=0), b"B, G and L must be positive"),
    (dict(n_cam=0), b"n_cam and n_pix must be positive"), (dict(n_pix=0), b"n_cam and n_pix must be positive"),
    (dict(G=65), b"G=65 exceeds 64 candidates per scene"),
    (dict(margin=0.0), b"margin must be finite and positive"), (dict(margin=math.nan), b"margin must be finite and positive"),
    (dict(margin=math.inf), b"margin must be finite and positive"), (dict(margin=-0.05), b"margin must be finite and positive"),
    (dict(skip_head=-1), b"negative skip"), (dict(skip_tail=-1), b"negative skip"),
    (dict(n_chunks=-1), b"n_chunks=-1 is negative"),
    (dict(n_cam=65536, n_pix=32768), b"n_cam * n_pix overflows int"),                 # 2^31
    (dict(B=65536), b"B=65536 exceeds 65535 scenes per call"),
    (dict(B=65535, n_chunks=1 << 20), b"exceed the grid"),
]
OWN = {
    "a3d_traj_clearance": [(dict(Dp=6), b"Dp=6, pose rows have 7 or 8 channels"), (dict(Dp=9), b"pose rows have 7 or 8 channels"),
                           (dict(G=64, L=1 << 22), b"G * L * 8 overflows int")],
    "a3d_traj_guide": [(dict(L=257), b"L=257 exceeds 256 rows per trajectory"), (dict(D=8), b"D=8, signal rows have 9 or 10 channels"),
                       (dict(D=11), b"signal rows have 9 or 10 channels"), (dict(push=1.5), b"push and smooth must lie in [0, 1]"),
                       (dict(smooth=-0.5), b"push and smooth must lie in [0, 1]"), (dict(push=math.nan), b"push and smooth must lie in [0, 1]"),
                       (dict(push=0.0, smooth=0.0), b"push and smooth are both 0: nothing to do")],
}


@pytest.fixture(scope="module")
def lib():
    return load_pkg().lib.load()


def _refused(lib, name, change, needle):
    a = dict(BASE, **change)
    assert getattr(lib, name)(*[a[k] for k in ORDER[name]], None) == -22, (name, change)
    msg = lib.a3d_last_error_string()
    assert msg.startswith(name.encode() + b":"), (name, change, msg)          # the entry that was called
    assert needle in msg, (name, change, msg)


@names
def test_shared_bad_arguments_are_refused_under_the_called_name(lib, name):
    for change, needle in SHARED:
        _refused(lib, name, change, needle)


@names
def test_null_required_pointers_are_refused(lib, name):
    for k in REQUIRED[name]:
        _refused(lib, name, {k: None}, b"null pointer (%s are required)" % (", ".join(REQUIRED[name][:-1]) + " and ws").encode())
    _refused(lib, name, dict(B=0, **{REQUIRED[name][0]: None}), b"null pointer")         # the pointers come first


@names
def test_each_entry_keeps_its_own_checks(lib, name):
    for change, needle in OWN[name]:
        _refused(lib, name, change, needle)


WS_TABLE = [(1, 1, 1, 1, 0), (2, 3, 5, 21, 0), (2, 3, 5, 21, 1), (2, 3, 5, 21, 3), (1, 8, 50, 8192, 0), (1, 64, 17, 21, 0), (1, 64, 17, 21, 7),
            (24, 2, 50, 49152, 0), (1, 16, 50, 262144, 0), (1, 16, 50, 262144, 5000), (65535, 64, 256, 1, 0), (1, 1, 1, 0x7fffffff, 0)]


def test_the_two_workspaces_agree_on_the_chunk_count(lib):
    for B, G, L, N, n_chunks in WS_TABLE:
        clear, guide = lib.a3d_traj_clearance_ws_floats(B, G, L, N, n_chunks), lib.a3d_traj_guide_ws_floats(B, G, L, N, n_chunks)
        c, rest = divmod(clear - B * L, B * G * L)
        assert rest == 0 and c >= 1 and guide == 2 * c * B * G * L, (B, G, L, N, n_chunks, clear, guide)
        if n_chunks > 0:
            assert c == n_chunks
        else:
            assert c <= max(1, -(-N // 512)) and c <= 4096                    # a chunk is at least one staged tile
    for bad in ((0, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 1, 0, 1, 0), (1, 1, 1, 0, 0), (1, 1, 1, 1, -1), (-1, 2, 3, 4, 0)):
        assert lib.a3d_traj_clearance_ws_floats(*bad) == 0 and lib.a3d_traj_guide_ws_floats(*bad) == 0, bad


# ------------------------------------------------------------------------------------------------ the module split
MOVED = ("PINS_MAX", "PIN_CHANNELS", "TrajectoryPins", "Pins", "pin_channel_bits", "check_pins", "traj_pins", "prefix_pins", "RANK_TERMS",
         "RANK_PRESETS", "RANK_MAX_CANDIDATES", "TrajectoryRanking", "PlannerRanking", "CLEARANCE_TERM", "CLEARANCE_PRESET",
         "TrajectoryClearance", "SceneTrajectoryRanking", "ScenePlannerRanking", "check_select", "check_rot_weight", "check_scene_select",
         "check_clearance_args", "check_scene", "trajectory_clearance", "GUIDE_MAX_ROWS", "GUIDE_KEYS", "Guidance", "check_guide_args",
         "check_guide", "check_guide_shape", "guided_segments", "guide_trajectories", "rank_trajectories")
TOP_LEVEL = ("rank_trajectories", "TrajectoryRanking", "trajectory_clearance", "TrajectoryClearance", "SceneTrajectoryRanking",
             "guide_trajectories", "guided_segments", "Guidance", "traj_pins", "prefix_pins", "check_pins", "TrajectoryPins", "Pins")
STAYED = ("DiffusionPlanner", "DiffusionHead", "SamplerSchedule", "DDPMTables", "check_sampler_args", "check_num_samples",
          "check_sampling_call", "traj_condition", "pose_to_signal", "signal_to_pose")


def test_diffusion_exports_the_objects_of_trajectory():
    a3d = load_pkg()
    for n in MOVED:
        assert getattr(a3d.diffusion, n) is getattr(a3d.trajectory, n), n
    for n in TOP_LEVEL:
        assert getattr(a3d, n) is getattr(a3d.trajectory, n), n
    for n in STAYED:
        assert getattr(a3d.diffusion, n).__module__ == a3d.diffusion.__name__ and not hasattr(a3d.trajectory, n), n


def test_number_raises_the_historic_texts():
    a3d = load_pkg()
    T, D = a3d.trajectory, a3d.diffusion
    nan = float("nan")
    cases = [
        (lambda: T.check_select({"goal": -1}), "select['goal'] = -1: a weight is a finite, non-negative number"),
        (lambda: T.check_scene_select({"clearance": True}), "select['clearance'] = True: a weight is a finite, non-negative number"),
        (lambda: T.check_rot_weight(nan), "rot_weight must be a finite, non-negative number, got nan"),
        (lambda: T.check_clearance_args(0, (1, 1)), "margin must be a finite, positive number (metres), got 0"),
        (lambda: T.check_clearance_args(0.05, (1, -1)),
         "skip must be two non-negative integers (rows skipped at the head, at the tail), got (1, -1)"),
        (lambda: T.check_clearance_args(0.05, [1.0, 1]),
         "skip must be two non-negative integers (rows skipped at the head, at the tail), got [1.0, 1]"),
        (lambda: T.check_clearance_args(0.05, 1), "skip must be two non-negative integers (rows skipped at the head, at the tail), got 1"),
        (lambda: T.check_guide_args(1.5, 0), "push must be a number in [0, 1], got 1.5"),
        (lambda: T.check_guide_args(1, "x"), "smooth must be a number in [0, 1], got 'x'"),
        (lambda: T.check_guide({"start": 1}), "guide['start'] must be a number in [0, 1), got 1"),
        (lambda: T.prefix_pins(torch.zeros(1, 5, 8), -1, 1), "executed must be an integer >= 0, got -1"),
        (lambda: T.prefix_pins(torch.zeros(1, 5, 8), 0, 1.0), "keep must be an integer >= 1, got 1.0"),
        (lambda: D.check_num_samples(0), "num_samples must be an integer >= 1 (or None for one trajectory per scene), got 0"),
        (lambda: D.check_sampler_args(100, 0), "num_inference_steps must be an integer in [1, 100], got 0"),
        (lambda: D.check_sampler_args(100, 101), "num_inference_steps must be an integer in [1, 100], got 101"),
        (lambda: D.check_sampler_args(100, True), "num_inference_steps must be an integer in [1, 100], got True"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    # what passes comes back as given
    assert T._number("x", 3, "", lo=0, integer=True) == 3 and T._number("x", 0.5, "", above=0, below=1) == 0.5
    assert T.check_clearance_args(1, [0, 2]) == (1.0, 0, 2) and T.check_guide(0.5) == (0.5, 0.0, 0.5)
    assert D.check_sampler_args(100) == 100 and D.check_sampler_args(100, 10, "ddim") == 10
