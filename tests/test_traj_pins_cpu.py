"""CPU tests of pinned waypoints: the host-side argument checks (check_pins, prefix_pins, the keyword through check_sampling_call and
Actioner.predict), the torch restatement of the kernel's rule (tests/pins_ref.py) on a hand-written case, and the C entry's argument
errors, which return before anything is launched."""
import ctypes
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from conftest import load_pkg  # noqa: E402
import pins_ref as PR  # noqa: E402


def some_pins(B=2, P=3, Dp=7, **kw):
    d = dict(poses=torch.zeros(B, P, Dp), index=torch.ones(B, P, dtype=torch.int64))
    d.update(kw)
    return d


# ------------------------------------------------------------------------------------------------ check_pins
def test_check_pins_accepts():
    D = load_pkg().diffusion
    poses, index, ch = D.check_pins(some_pins(), 2, 7)
    assert ch == 3 and tuple(poses.shape) == (2, 3, 7) and tuple(index.shape) == (2, 3)          # "pose" is the default
    for names, bits in (("position", 1), ("rotation", 2), ("gripper", 4), ("pose", 3), ("all", 7), (("position", "gripper"), 5),
                        (["rotation", "position"], 3), (("pose", "gripper"), 7)):
        assert D.check_pins(some_pins(channels=names), 2, 7)[2] == bits, names
    masks = torch.tensor([[1, 2, 3], [7, 0, 4]], dtype=torch.uint8)
    assert D.check_pins(some_pins(channels=masks), 2, 7)[2] is masks
    # a namedtuple serves as well as a dict; 32 pins are the most a call takes; every integer dtype indexes; Dp = 8 rows
    assert D.check_pins(D.TrajectoryPins(torch.zeros(2, 3, 7), torch.ones(2, 3, dtype=torch.int32)), 2, 7)[2] == 3
    assert D.check_pins(D.TrajectoryPins(torch.zeros(2, 3, 7), torch.ones(2, 3, dtype=torch.int32), "all"), 2, 7)[2] == 7
    assert D.PINS_MAX == 32 and D.check_pins(some_pins(P=32), 2, 7)[0].shape[1] == 32
    assert D.check_pins(some_pins(Dp=8, index=torch.ones(2, 3, dtype=torch.int16)), 2, 8)[0].shape[2] == 8
    assert D.check_pins(some_pins(poses=torch.zeros(2, 3, 7, dtype=torch.float64)), 2, 7)[0].dtype == torch.float64


@pytest.mark.parametrize("name,pins,B,Dp,match", [
    ("wrong B", some_pins(B=3), 2, 7, "poses has shape"),
    ("wrong Dp", some_pins(Dp=8), 2, 7, "poses has shape"),
    ("wrong P", some_pins(index=torch.ones(2, 4, dtype=torch.int64)), 2, 7, "index has shape"),
    ("wrong B of the index", some_pins(index=torch.ones(3, 3, dtype=torch.int64)), 2, 7, "index has shape"),
    ("33 pins", some_pins(P=33), 2, 7, "1 to 32"),
    ("no pin", some_pins(P=0), 2, 7, "1 to 32"),
    ("unknown channel name", some_pins(channels="orientation"), 2, 7, "unknown channel name"),
    ("unknown name in a tuple", some_pins(channels=("position", "open")), 2, 7, "unknown channel name"),
    ("empty tuple", some_pins(channels=()), 2, 7, "channels must be"),
    ("channels of another type", some_pins(channels=3), 2, 7, "channels must be"),
    ("float index", some_pins(index=torch.ones(2, 3)), 2, 7, "integer tensor"),
    ("bool index", some_pins(index=torch.ones(2, 3, dtype=torch.bool)), 2, 7, "integer tensor"),
    ("index is a list", some_pins(index=[[1, 1, 1], [1, 1, 1]]), 2, 7, "integer tensor"),
    ("integer poses", some_pins(poses=torch.zeros(2, 3, 7, dtype=torch.int32)), 2, 7, "floating-point"),
    ("flat poses", some_pins(poses=torch.zeros(6, 7)), 2, 7, "floating-point"),
    ("channel tensor of another dtype", some_pins(channels=torch.ones(2, 3, dtype=torch.int32)), 2, 7, "uint8 bit mask"),
    ("channel tensor of another shape", some_pins(channels=torch.ones(2, 4, dtype=torch.uint8)), 2, 7, "uint8 bit mask"),
    ("unknown key", dict(some_pins(), rows=1), 2, 7, "a dict with the keys"),
    ("missing key", {"poses": torch.zeros(2, 3, 7)}, 2, 7, "a dict with the keys"),
    ("a bare tensor", torch.zeros(2, 3, 7), 2, 7, "dict or a namedtuple"),
], ids=lambda v: v if isinstance(v, str) and " " in v else None)
def test_check_pins_raises(name, pins, B, Dp, match):
    D = load_pkg().diffusion
    with pytest.raises(ValueError, match=match):
        D.check_pins(pins, B, Dp)


def test_the_keyword_is_checked_before_anything_is_launched():
    """check_sampling_call (compute_trajectory's and Actioner.predict's host-side check) validates the pins against the call's B and
    pose width; the Actioner passes the keyword on."""
    a3d = load_pkg()
    D = a3d.diffusion
    pcd = torch.zeros(2, 1, 3, 4, 4)
    assert D.check_sampling_call(2, 8, 9, 100, pcd, True, pins=some_pins()).G is None
    assert D.check_sampling_call(2, 8, 10, None, pcd, True, pins=some_pins(Dp=8), num_samples=3).G == 3      # action_dim = 8
    for D_, pins in ((10, some_pins()), (9, some_pins(Dp=8)), (9, some_pins(B=3)), (9, some_pins(P=33)), (9, some_pins(channels="x"))):
        with pytest.raises(ValueError, match="pins"):
            D.check_sampling_call(2, 8, D_, None, pcd, True, pins=pins)
    assert "pins" in a3d.actioner._TRAJ_KW
    assert a3d.prefix_pins is D.prefix_pins and a3d.traj_pins is D.traj_pins and a3d.Pins._fields == ("index", "applied")
    assert a3d.TrajectoryPins._fields == ("poses", "index", "channels")
    act = a3d.Actioner(predict_keypose=False, predict_trajectory=False)
    assert act.last_pins is None
    act.set_instruction(torch.zeros(53, 512))
    with pytest.raises(ValueError, match="predict_trajectory=True"):
        act.predict(torch.zeros(1, 1, 1, 3, 8, 8), torch.zeros(1, 1, 1, 3, 8, 8), torch.zeros(1, 1, 8), torch.zeros(1, 1, 8),
                    pins=some_pins(B=1))


# ------------------------------------------------------------------------------------------------ prefix_pins
def test_prefix_pins_indices_and_rows():
    D = load_pkg().diffusion
    B, L, Dp = 3, 12, 8
    prev = torch.arange(B * L * Dp, dtype=torch.float32).reshape(B, L, Dp)
    pins = D.prefix_pins(prev, 2, 3)
    assert type(pins) is D.TrajectoryPins and pins.channels == "pose"
    assert pins.index.dtype == torch.int32 and torch.equal(pins.index, torch.tensor([[1, 2, 3]] * B, dtype=torch.int32))
    assert torch.equal(pins.poses, prev[:, 3:6]) and pins.poses.data_ptr() == prev[:, 3:6].data_ptr()          # a view: no copy
    assert D.check_pins(pins, B, Dp)[2] == 3
    # nothing executed: rows 1 .. keep of the old plan stay where they are; the whole remaining plan may be kept
    pins = D.prefix_pins(prev, 0, L - 1, channels=("position", "gripper"))
    assert torch.equal(pins.poses, prev[:, 1:]) and torch.equal(pins.index[0], torch.arange(1, L, dtype=torch.int32))
    assert D.check_pins(pins, B, Dp)[2] == 5
    pins = D.prefix_pins(prev, 10, 1)
    assert torch.equal(pins.poses, prev[:, 11:12]) and pins.index.tolist() == [[1]] * B
    for args, match in (((prev, 10, 2), "do not all exist"), ((prev, 0, L), "do not all exist"), ((prev, -1, 2), "executed"),
                        ((prev, 1, 0), "keep"), ((prev, 1.0, 2), "executed"), ((prev, True, 2), "executed"), ((prev[0], 1, 2), "previous"),
                        ((torch.zeros(1, 64, 7), 0, 33), "at most 32")):
        with pytest.raises(ValueError, match=match):
            D.prefix_pins(*args)
    with pytest.raises(ValueError, match="unknown channel name"):
        D.prefix_pins(prev, 1, 2, channels="orientation")


# ------------------------------------------------------------------------------------------------ the twin's rule
def test_the_twin_on_a_hand_written_case():
    """B = 2 scenes, G = 2 candidates, L = 6, D = 10; scene 1 has two padded rows (last = 3, goal row 3).  Every value is chosen so
    that the expected tensors can be written down."""
    B, G, L, D, P = 2, 2, 6, 10, 5
    tmask = torch.zeros(B, L, dtype=torch.bool)
    tmask[1, 4:] = True
    cond = torch.zeros(B * G, L, D)
    cmask = torch.zeros(B * G, L, D, dtype=torch.uint8)
    cmask[:, 0] = 1
    cmask[:2, 5] = 1
    cmask[2:, 3:] = 1
    noise = torch.full((B * G, L, D), 0.5)
    traj = noise + cond
    sig = torch.arange(1, B * P + 1, dtype=torch.float32).reshape(B, P, 1).expand(B, P, D).contiguous()      # slot p of scene b holds b P + p + 1
    index = torch.tensor([[2, 3, 3, 2, -1],            # scene 0: pose on row 2; position, then rotation on row 3; slot 3 over slot 0; unused
                          [0, 3, 4, 2, 1]])            # scene 1: row 0, the goal row, a padded row: dropped; rows 2 and 1 applied
    channels = torch.tensor([[3, 1, 2, 2, 7], [7, 7, 7, 4, 0]], dtype=torch.uint8)
    channels[1, 4] = 1
    cd, cm, tr, applied = PR.pins_ref(cond, cmask, traj, noise, sig, index, channels, tmask, G, True)
    assert applied.tolist() == [[1, 1, 1, 1, 0], [0, 0, 0, 1, 1]]
    want = torch.zeros(B * G, L, D)
    want[:2, 2, 0:3], want[:2, 2, 3:9] = 1.0, 4.0                    # slot 0's position stays, slot 3's rotation wins
    want[:2, 3, 0:3], want[:2, 3, 3:9] = 2.0, 3.0                    # the position-only and the rotation-only pin merge
    want[2:, 2, 9], want[2:, 1, 0:3] = 9.0, 10.0                     # scene 1: the extras of row 2, the position of row 1
    wmask = cmask.clone()
    wmask[:2, 2, :9], wmask[:2, 3, :9], wmask[2:, 2, 9], wmask[2:, 1, :3] = 1, 1, 1, 1
    assert torch.equal(cd, want) and torch.equal(cm, wmask)
    assert torch.equal(tr, torch.where(want != 0, want + 0.5, traj))
    assert torch.equal(cond, torch.zeros_like(cond)) and torch.equal(traj, noise)                 # the arguments are not written
    # without a goal the last valid row takes a pin: slot 1 of scene 1 (row 3 = last) is applied, the padded row still is not
    cd, cm, tr, applied = PR.pins_ref(cond, cmask, None, None, sig, index, channels, tmask, G, False)
    assert tr is None and applied.tolist() == [[1, 1, 1, 1, 0], [0, 1, 0, 1, 1]] and bool((cd[2:, 3] == 7.0).all())
    # scene 0's row 5 is its last: dropped with a goal, applied without
    index[0, 4] = 5
    assert PR.pins_ref(cond, cmask, None, None, sig, index, channels, tmask, G, True)[3][0].tolist() == [1, 1, 1, 1, 0]
    assert PR.pins_ref(cond, cmask, None, None, sig, index, channels, tmask, G, False)[3][0].tolist() == [1, 1, 1, 1, 1]
    # an all-padding scene takes nothing
    tmask[1] = True
    assert PR.pins_ref(cond, cmask, None, None, sig, index, channels, tmask, G, False)[3][1].tolist() == [0] * P


# ------------------------------------------------------------------------------------------------ the C entry
def test_the_entry_is_exported_with_the_header_signature():
    a3d = load_pkg()
    lib = a3d.lib.load()
    header = open(os.path.join(ROOT, "include", "act3d_hip.h")).read()
    assert "a3d_traj_pins" in a3d.lib.exported_symbols() and hasattr(lib, "a3d_traj_pins")
    m = re.search(r"\ba3d_traj_pins\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m and len([p for p in m.group(1).split(",") if p.strip()]) == len(lib.a3d_traj_pins.argtypes) == 18
    assert a3d.lib.PARAM_NAMES["a3d_traj_pins"][:4] == ["poses", "ldp", "index", "channels"]
    assert a3d.lib.TRAJ_PINS_MAX == 32
    b = a3d.build.__globals__
    assert "traj_pins.hip" in b["SOURCES"] and b["EXTRA_FLAGS"]["traj_pins.hip"] == ["-Wall", "-Wextra"]
    # both users of the row map include the one header, and a change of it rebuilds them
    csrc = os.path.join(ROOT, "act3d-chained-diffuser_amd", "csrc")
    for src in ("diffusion.hip", "traj_pins.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "pose_signal.h"' in text and "void pose_row_to_signal" not in text, src
    assert "pose_signal.h" in open(os.path.join(ROOT, "act3d-chained-diffuser_amd", "build.py")).read()


def test_traj_pins_rejects_bad_arguments_without_a_device():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    d = ctypes.c_void_p(64)                                         # aligned, never dereferenced
    call = lib.a3d_traj_pins

    def args(**kw):
        a = dict(poses=d, ldp=8, index=d, channels=d, bounds=d, tmask=d, init_noise=d, cond_data=d, cond_mask=d, traj=d, applied=d,
                 B=2, G=3, P=5, L=8, Dp=8, use_goal=1)
        a.update(kw)
        return list(a.values()) + [None]

    def refused(**kw):
        assert call(*args(**kw)) == -22, kw
        assert b"a3d_traj_pins" in lib.a3d_last_error_string(), kw

    for name in ("poses", "index", "channels", "bounds", "tmask", "cond_data", "cond_mask", "applied"):
        refused(**{name: None})
    refused(init_noise=None)                                        # traj without init_noise
    for name in ("B", "G", "L"):
        for v in (0, -1):
            refused(**{name: v})
    for v in (0, -1, 33):
        refused(P=v)
    refused(Dp=6, ldp=8)
    refused(Dp=31, ldp=31)                                          # D = 33 signal channels
    refused(ldp=7)
    refused(L=0x7fffffff)                                           # L * D overflows int
