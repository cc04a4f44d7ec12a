"""What happens to the sampler's trajectory candidates besides the denoising itself: pinned waypoints (traj_pins, a3d_traj_pins),
ranking and selection (rank_trajectories, a3d_traj_rank), scene clearance (trajectory_clearance, a3d_traj_clearance; with a gripper
body of swept spheres body_clearance, a3d_traj_body_clearance) and clearance
guidance (guide_trajectories, a3d_traj_guide), with their named tuples and the host-side checks of their arguments.  The reference
has none of these (Actioner.predict, online_evaluation/utils_with_rlbench.py:120-230, executes the one trajectory it samples).
diffusion.py (the planner, compute_trajectory's keywords) re-exports every name of this module."""
import collections
import math

import torch

from . import ops as O


# ------------------------------------------------------------------------------------------------ shared checks and buffers
def _number(name, v, expect, *, lo=None, hi=None, above=None, below=None, integer=False, form="%(name)s %(expect)s, got %(v)r", shown=...):
    """v where it is an int or a float (integer: an int), not a bool, finite and inside lo <= v <= hi, above < v < below (None: no
    such bound); ValueError(form) otherwise -- by default "<name> <expect>, got <v>"; shown: the value the message prints for v."""
    ok = not isinstance(v, bool) and isinstance(v, int if integer else (int, float)) and (isinstance(v, int) or math.isfinite(v))
    ok = ok and (lo is None or v >= lo) and (hi is None or v <= hi) and (above is None or v > above) and (below is None or v < below)
    if not ok:
        raise ValueError(form % {"name": name, "expect": expect, "v": v if shown is ... else shown})
    return v


def _weight(name, v):
    return float(_number(name, v, "a weight is a finite, non-negative number", lo=0, form="%(name)s = %(v)r: %(expect)s"))


def check_trajectory_mask(trajectory_mask, B, Ln=None):
    """the (B, L) padding mask of a call: B scenes and, where the caller already knows it, Ln rows"""
    if Ln is None:
        if trajectory_mask.dim() != 2 or trajectory_mask.shape[0] != B:
            raise ValueError("trajectory_mask must be (B, L) with B = %d, got %s" % (B, tuple(trajectory_mask.shape)))
    elif not torch.is_tensor(trajectory_mask) or tuple(trajectory_mask.shape) != (B, Ln):
        raise ValueError("trajectory_mask must be (B, L) = %s, got %s" % (
            (B, Ln), tuple(trajectory_mask.shape) if torch.is_tensor(trajectory_mask) else type(trajectory_mask).__name__))


def _pose_rows(x, name):
    """(tensor, leading dimension in floats) of fp32 pose rows (B, Dp) the kernel can read in place: unit stride inside a row, any
    row stride >= Dp (a slice of a wider tensor, e.g. action[..., :7] of (B, 8) rows); anything else is copied."""
    if x.dim() != 2:
        raise ValueError("%s must be (B, Dp) pose rows, got shape %s" % (name, tuple(x.shape)))
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1]))


def _mask_bytes(tm):
    """a bool / uint8 / numeric mask as contiguous bytes; a bool tensor stores 0 / 1 bytes: read in place"""
    tm = tm.detach()
    return O._c(tm).view(torch.uint8) if tm.dtype == torch.bool else O._c((tm != 0).view(torch.uint8) if tm.dtype != torch.uint8 else tm)


# a scene as the two scan entries read it: cloud fp32 [B][C][3][n_pix], mask bytes [B][C][n_pix] or None
Scene = collections.namedtuple("Scene", ("cloud", "mask", "n_cam", "n_pix"))


def check_scene(scene, scene_mask, B):
    """shape checks of a scene cloud (B, C, 3, H, W) or (B, N, 3) and its mask -> (n_cam, n_pix)"""
    if not torch.is_tensor(scene) or scene.dim() not in (3, 5) or scene.shape[0] != B:
        raise ValueError("scene must be (B, C, 3, H, W) or (B, N, 3) with B = %d, got %s" % (
            B, tuple(scene.shape) if torch.is_tensor(scene) else type(scene).__name__))
    if scene.dim() == 5:
        if scene.shape[2] != 3 or min(scene.shape[1], scene.shape[3], scene.shape[4]) < 1:
            raise ValueError("scene must be (B, C, 3, H, W) with at least one point, got %s" % (tuple(scene.shape),))
        n_cam, n_pix, mshape = scene.shape[1], scene.shape[3] * scene.shape[4], (B, scene.shape[1], scene.shape[3], scene.shape[4])
    else:
        if scene.shape[2] != 3 or scene.shape[1] < 1:
            raise ValueError("scene must be (B, N, 3) with at least one point, got %s" % (tuple(scene.shape),))
        n_cam, n_pix, mshape = 1, scene.shape[1], (B, scene.shape[1])
    if not scene.is_floating_point():
        raise ValueError("scene must be a floating-point tensor, got %s" % scene.dtype)
    if scene_mask is not None:
        if not torch.is_tensor(scene_mask) or tuple(scene_mask.shape) != mshape:
            raise ValueError("scene_mask must be %s (one entry per point of scene), got %s" % (
                mshape, tuple(scene_mask.shape) if torch.is_tensor(scene_mask) else type(scene_mask).__name__))
        if scene_mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("scene_mask must be bool or uint8, got %s" % scene_mask.dtype)
    if n_cam * n_pix > 0x7fffffff:
        raise ValueError("scene has %d points per scene; the kernel addresses at most 2^31 - 1" % (n_cam * n_pix))
    return n_cam, n_pix


def prepare_scene(scene, scene_mask, B):
    """check_scene, then the scene as a Scene: the cloud read in place when it is contiguous fp32 (B, C, 3, H, W); (B, N, 3) rows are
    transposed ONCE to (B, 3, N) = (B, 1, 3, N), the one copy of the cloud"""
    n_cam, n_pix = check_scene(scene, scene_mask, B)
    S = scene.detach().float()
    S = O._c(S) if S.dim() == 5 else S.transpose(1, 2).contiguous()
    return Scene(S, None if scene_mask is None else _mask_bytes(scene_mask), n_cam, n_pix)


def scan_workspace(entry, B, G, Ln, n_points, device):
    """the workspace of a3d_traj_clearance / a3d_traj_guide (`entry`) for the chunk count the entry chooses itself"""
    n = getattr(O.L.load(), entry + "_ws_floats")(B, G, Ln, n_points, 0)
    return torch.empty((n,), device=device, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ pinned waypoints
PINS_MAX = O.L.TRAJ_PINS_MAX               # pins per scene of one call (a3d_traj_pins keeps them in LDS)
# channel groups of a pin -> the bit a3d_traj_pins reads: position = signal columns 0..2, rotation = 3..8, gripper = the extras 9..D-1
PIN_CHANNELS = {"position": 1, "rotation": 2, "gripper": 4, "pose": 3, "all": 7}
# pins as compute_trajectory(pins=...) takes them (a dict with these keys serves as well; channels may be left out = "pose")
TrajectoryPins = collections.namedtuple("TrajectoryPins", ("poses", "index", "channels"), defaults=("pose",))
# what a call with pins keeps on the planner: the rows asked for and which slots were written, (B, P) device tensors
Pins = collections.namedtuple("Pins", ("index", "applied"))
_PIN_INDEX_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


def pin_channel_bits(channels):
    """"position" | "rotation" | "gripper" | "pose" (= position + rotation) | "all", or a tuple / list of them -> the bit mask"""
    names = (channels,) if isinstance(channels, str) else channels
    if not isinstance(names, (tuple, list)) or not names:
        raise ValueError("pins: channels must be a name, a tuple of names from %s, or a (B, P) uint8 tensor of bit masks, got %r"
                         % (sorted(PIN_CHANNELS), channels))
    bits = 0
    for n in names:
        if not isinstance(n, str) or n not in PIN_CHANNELS:
            raise ValueError("pins: unknown channel name %r (one of %s)" % (n, sorted(PIN_CHANNELS)))
        bits |= PIN_CHANNELS[n]
    return bits


def check_pins(pins, B, Dp):
    """Validates compute_trajectory's `pins` on the host (shapes, dtypes and Python values: nothing is launched or copied) and returns
    (poses, index, channels): poses (B, P, Dp) floating point, index (B, P) integer -- the trajectory row of each pin, < 0 = unused
    slot -- and channels as the bit mask of a3d_traj_pins, an int for every slot or a (B, P) uint8 tensor.  pins: a dict or a
    namedtuple (TrajectoryPins) with "poses", "index" and optionally "channels": a name or a tuple of names from "position",
    "rotation", "gripper" (the channels after the quaternion), "pose" (position + rotation, the default) and "all", or the (B, P)
    uint8 tensor itself.  P <= 32; Dp must be the call's pose width.  Which rows are in range is decided on the device (the
    padding is a device tensor): see traj_pins."""
    if isinstance(pins, dict):
        bad = [k for k in pins if k not in TrajectoryPins._fields]
        if bad or "poses" not in pins or "index" not in pins:
            raise ValueError("pins: a dict with the keys 'poses', 'index' and optionally 'channels', got %s" % sorted(pins))
        poses, index, channels = pins["poses"], pins["index"], pins.get("channels", "pose")
    elif isinstance(pins, tuple) and all(hasattr(pins, k) for k in TrajectoryPins._fields):
        poses, index, channels = pins.poses, pins.index, pins.channels
    else:
        raise ValueError("pins must be a dict or a namedtuple with poses, index and channels, got %s" % type(pins).__name__)
    if not torch.is_tensor(poses) or poses.dim() != 3 or not poses.is_floating_point():
        raise ValueError("pins: poses must be a floating-point (B, P, Dp) tensor, got %s" % (
            (tuple(poses.shape), poses.dtype) if torch.is_tensor(poses) else type(poses).__name__,))
    P = poses.shape[1]
    if poses.shape[0] != B or poses.shape[2] != Dp:
        raise ValueError("pins: poses has shape %s, the call needs (B, P, Dp) = (%d, P, %d)" % (tuple(poses.shape), B, Dp))
    if not 1 <= P <= PINS_MAX:
        raise ValueError("pins: P = %d pins per scene, a call takes 1 to %d" % (P, PINS_MAX))
    if not torch.is_tensor(index) or index.dtype not in _PIN_INDEX_DTYPES:
        raise ValueError("pins: index must be an integer tensor, got %s" % (index.dtype if torch.is_tensor(index) else type(index).__name__,))
    if tuple(index.shape) != (B, P):
        raise ValueError("pins: index has shape %s, poses names (B, P) = %s" % (tuple(index.shape), (B, P)))
    if torch.is_tensor(channels):
        if channels.dtype != torch.uint8 or tuple(channels.shape) != (B, P):
            raise ValueError("pins: a channels tensor holds one uint8 bit mask per slot, (B, P) = %s, got %s %s"
                             % ((B, P), tuple(channels.shape), channels.dtype))
    else:
        channels = pin_channel_bits(channels)
    return poses, index, channels


def traj_pins(cond_data, cond_mask, traj, init_noise, pins, bounds, trajectory_mask, num_samples=1, use_goal=True):
    """Pinned waypoints in ONE launch (a3d_traj_pins, csrc/traj_pins.hip): writes the pins of every scene into the conditioning
    tensors of its G = num_samples trajectories, IN PLACE, and returns applied (B, P) uint8.  cond_data fp32 / cond_mask uint8:
    (B G, L, D) contiguous, as traj_condition returns them; traj / init_noise: (B G, L, D) fp32 or None -- with both,
    traj = init_noise + the pinned signal on the pinned elements (the start the other conditioned rows get); pins: check_pins;
    trajectory_mask: (B, L) per scene, non-zero = padded.
    With last = L - pad - 1, slot p of scene b is applied iff its channels are not empty and 1 <= index <= last - 1 (use_goal) or
    1 <= index <= last: row 0, the goal row and padded rows are never touched, an out-of-range pin is dropped (applied = 0), never an
    error -- the padding lives on the device and nothing is copied back.  The pose goes through pose_to_signal's row map (the same
    bits); where two applied pins select one element the higher slot wins; elements no pin selects keep their bits."""
    if trajectory_mask.dim() != 2:
        raise ValueError("trajectory_mask must be (B, L), got %s" % (tuple(trajectory_mask.shape),))
    B, Ln = trajectory_mask.shape
    G = int(num_samples)
    D = cond_data.shape[-1]
    poses, index, channels = check_pins(pins, B, D - 2)
    P = poses.shape[1]
    for name, x, dt in (("cond_data", cond_data, torch.float32), ("cond_mask", cond_mask, torch.uint8), ("traj", traj, torch.float32)):
        if x is not None and (tuple(x.shape) != (B * G, Ln, D) or x.dtype != dt or not x.is_contiguous()):
            raise ValueError("%s is updated in place: it must be contiguous %s of shape %s, got %s %s" % (
                name, dt, (B * G, Ln, D), tuple(x.shape), x.dtype))
    if traj is not None and init_noise is None:
        raise ValueError("traj needs init_noise (traj = init_noise + the pinned signal)")
    if init_noise is not None and tuple(init_noise.shape) != (B * G, Ln, D):
        raise ValueError("init_noise has shape %s, the call needs %s" % (tuple(init_noise.shape), (B * G, Ln, D)))
    dev = cond_data.device
    O.L.require_gpu(cond_data, cond_mask, traj, init_noise, bounds, trajectory_mask)
    poses = poses.detach().to(device=dev, dtype=torch.float32)
    if poses.stride(2) != 1 or poses.stride(1) < D - 2 or poses.stride(0) != P * poses.stride(1):
        poses = poses.contiguous()
    index = O._c(index.detach().to(device=dev, dtype=torch.int32))
    channels = O._c(channels.to(dev)) if torch.is_tensor(channels) else torch.full((B, P), channels, device=dev, dtype=torch.uint8)
    noise = None if (init_noise is None or traj is None) else O._c(init_noise.detach().float())
    applied = torch.empty((B, P), device=dev, dtype=torch.uint8)
    O.L.call("a3d_traj_pins", poses.data_ptr(), poses.stride(1), index.data_ptr(), channels.data_ptr(), O._c(bounds).data_ptr(),
             _mask_bytes(trajectory_mask).data_ptr(), None if noise is None else noise.data_ptr(), cond_data.data_ptr(),
             cond_mask.data_ptr(), None if traj is None else traj.data_ptr(), applied.data_ptr(), B, G, P, Ln, D - 2,
             1 if use_goal else 0, O.L.stream())
    return applied


def prefix_pins(previous, executed, keep, channels="pose"):
    """The pins of a receding-horizon replan: from the last plan `previous` (B, L, Dp) and the number of its steps `executed` since it
    was made, pins that hold rows executed + 1 .. executed + keep of the old plan on rows 1 .. keep of the new one, so that the new
    trajectory starts with what the robot is already committed to.  The caller passes the pose at row `executed` of the old plan
    (where the robot is now) as curr_gripper: it becomes row 0.  Pure indexing on the device: a view of `previous` and an arange,
    nothing is copied to the host.  Rows the new call cannot hold (its goal row, padding) are dropped there (last_pins.applied)."""
    if not torch.is_tensor(previous) or previous.dim() != 3:
        raise ValueError("previous must be a (B, L, Dp) trajectory, got %s" % (
            tuple(previous.shape) if torch.is_tensor(previous) else type(previous).__name__,))
    for name, v, lo in (("executed", executed, 0), ("keep", keep, 1)):
        _number(name, v, "must be an integer >= %d" % lo, lo=lo, integer=True)
    if keep > PINS_MAX:
        raise ValueError("keep = %d rows; a call takes at most %d pins per scene" % (keep, PINS_MAX))
    B, Ln = previous.shape[:2]
    if executed + keep > Ln - 1:
        raise ValueError("previous has %d rows: rows %d .. %d do not all exist" % (Ln, executed + 1, executed + keep))
    pin_channel_bits(channels)
    index = torch.arange(1, keep + 1, device=previous.device, dtype=torch.int32)[None, :].expand(B, keep)
    return TrajectoryPins(previous[:, executed + 1:executed + keep + 1], index, channels)


# ------------------------------------------------------------------------------------------------ candidate ranking
RANK_TERMS = ("consensus", "goal", "smooth", "length", "bounds")
RANK_PRESETS = {"consensus": "consensus", "goal": "goal", "smooth": "smooth", "shortest": "length"}
RANK_MAX_CANDIDATES = 64
TrajectoryRanking = collections.namedtuple("TrajectoryRanking", ("best", "order", "scores", "terms", "selected"))
# what compute_trajectory(select=...) keeps on the planner: the ranking and all candidates (B, G, L, 8)
PlannerRanking = collections.namedtuple("PlannerRanking", TrajectoryRanking._fields + ("candidates",))
# the scene-aware term (csrc/traj_clearance.hip): weighed by select={"clearance": w} or the preset "clear", never part of RANK_TERMS
CLEARANCE_TERM = "clearance"
CLEARANCE_PRESET = "clear"
TrajectoryClearance = collections.namedtuple("TrajectoryClearance", ("nearest", "clearance"))
# what rank_trajectories returns when the rule weighs the clearance term: the five fields in order, then clearance (B, G), nearest (B, G, L)
SceneTrajectoryRanking = collections.namedtuple("SceneTrajectoryRanking", TrajectoryRanking._fields + ("clearance", "nearest"))
ScenePlannerRanking = collections.namedtuple("ScenePlannerRanking", SceneTrajectoryRanking._fields + ("candidates",))


def check_select(select, have_goal=True, have_bounds=True):
    """Validates a `select` rule on the host and returns its five weights in RANK_TERMS order.  A preset name ("consensus", "goal",
    "smooth", "shortest") puts weight 1 on one term; a dict maps a subset of RANK_TERMS to finite, non-negative weights, not all zero.
    A non-zero goal / bounds weight needs a goal / bounds."""
    return _term_weights(select, have_goal, have_bounds, False)


def _term_weights(select, have_goal, have_bounds, all_zero_ok):
    if isinstance(select, str):
        if select not in RANK_PRESETS:
            raise ValueError("select=%r: the presets are %s (or a dict over %s)" % (select, sorted(RANK_PRESETS), list(RANK_TERMS)))
        select = {RANK_PRESETS[select]: 1.0}
    elif not isinstance(select, dict):
        raise ValueError("select must be a preset name or a dict of term weights, got %r" % (select,))
    bad = [k for k in select if k not in RANK_TERMS]
    if bad:
        raise ValueError("select has unknown terms %s; the terms are %s" % (bad, list(RANK_TERMS)))
    w = [_weight("select[%r]" % (k,), select.get(k, 0.0)) for k in RANK_TERMS]
    if not any(w) and not all_zero_ok:
        raise ValueError("select gives every term weight 0")
    if w[1] != 0.0 and not have_goal:
        raise ValueError("select weighs the goal term, but no goal is given")
    if w[4] != 0.0 and not have_bounds:
        raise ValueError("select weighs the bounds term, but no bounds are given")
    return w


def check_rot_weight(rot_weight):
    return float(_number("rot_weight", rot_weight, "must be a finite, non-negative number", lo=0))


def check_scene_select(select, have_goal=True, have_bounds=True, have_scene=True):
    """check_select for rules that may also weigh the scene term: returns (the five weights in RANK_TERMS order, w_clearance).  The
    preset "clear" puts weight 1 on "clearance"; a dict may map "clearance" to a finite, non-negative weight beside the five terms.
    A rule whose only non-zero weight is the clearance is valid; a non-zero clearance weight needs a scene.  A rule that does not
    name the term goes through check_select unchanged."""
    if isinstance(select, str):
        if select != CLEARANCE_PRESET:
            return check_select(select, have_goal, have_bounds), 0.0
        select = {CLEARANCE_TERM: 1.0}
    if not isinstance(select, dict) or CLEARANCE_TERM not in select:
        return check_select(select, have_goal, have_bounds), 0.0
    wc = _weight("select[%r]" % (CLEARANCE_TERM,), select[CLEARANCE_TERM])
    rest = {k: x for k, x in select.items() if k != CLEARANCE_TERM}
    if wc == 0.0:
        return check_select(rest, have_goal, have_bounds), 0.0
    if not have_scene:
        raise ValueError("select weighs the clearance term, but no scene is given")
    w = _term_weights(rest, have_goal, have_bounds, True)       # the other terms by the same checks; they may all be zero here
    return w, wc


def check_clearance_args(margin, skip):
    """-> (margin, skip_head, skip_tail) of the clearance term, or ValueError"""
    _number("margin", margin, "must be a finite, positive number (metres)", above=0)
    for k in skip if isinstance(skip, (tuple, list)) and len(skip) == 2 else (None,):       # None: not a pair, refused below
        _number("skip", k, "must be two non-negative integers (rows skipped at the head, at the tail)", lo=0, integer=True, shown=skip)
    return float(margin), int(skip[0]), int(skip[1])


def _check_candidates(trajectories, trajectory_mask):
    if not torch.is_tensor(trajectories) or trajectories.dim() != 4:
        raise ValueError("trajectories must be a (B, G, L, Dp) tensor, got %s" % (
            tuple(trajectories.shape) if torch.is_tensor(trajectories) else type(trajectories).__name__,))
    B, G, Ln, Dp = trajectories.shape
    if min(B, G, Ln) < 1:
        raise ValueError("trajectories has an empty dimension: %s" % (tuple(trajectories.shape),))
    if Dp not in (7, 8):
        raise ValueError("trajectories rows have %d channels; pose rows have 7 or 8" % Dp)
    if G > RANK_MAX_CANDIDATES:
        raise ValueError("G = %d candidates per scene; the ranking serves at most %d" % (G, RANK_MAX_CANDIDATES))
    check_trajectory_mask(trajectory_mask, B, Ln)
    return B, G, Ln, Dp


def trajectory_clearance(trajectories, trajectory_mask, scene, scene_mask=None, margin=0.05, skip=(1, 1)):
    """Distance of every waypoint of every candidate to the nearest observed scene point, and a clearance term per candidate, in TWO
    launches (a3d_traj_clearance, csrc/traj_clearance.hip): brute force over the cloud, no (rows x points) matrix, no host copy.
    trajectories: (B, G, L, Dp) fp32 poses in world coordinates as compute_trajectory returns them, Dp = 7 or 8 (only xyz is
    read), G <= 64; trajectory_mask: (B, L), non-zero = padded row (any pattern).  scene: the observed cloud in world coordinates,
    (B, C, 3, H, W) fp32 -- compute_trajectory's pcd_obs -- read in place when contiguous, or (B, N, 3) point rows, which are
    transposed ONCE to (B, 1, 3, N) (one copy of the cloud).  scene_mask: (B, C, H, W) (or (B, N)) bool / uint8, non-zero = ignore
    the point (RLBench's robot mask).  A point counts when it is not masked and its coordinates are finite.
    Returns TrajectoryClearance(nearest (B, G, L), clearance (B, G)).  nearest: min over the counted points of |p - s|_2 (+inf
    without a counted point and on padded rows, NaN where the row's xyz is not finite).  clearance: with j the rank of a valid row
    among the n valid rows of its scene, the mean over the rows skip[0] <= j < n - skip[1] of max(0, margin - nearest) / margin, in
    [0, 1]: 0 = every scored waypoint keeps at least `margin` metres clear, 1 = every one touches a point; 0 without a scored row,
    NaN as soon as a scored row is NaN.  margin = 0.05 and skip = (1, 1) are choices, not derived values: 5 cm is about a finger
    length of the Franka gripper, and row 0 (the in-painted current pose) and the last valid row (the goal) are where contact is
    intended.  Bit-identical from run to run."""
    B, G, Ln, Dp = _check_candidates(trajectories, trajectory_mask)
    sc = prepare_scene(scene, scene_mask, B)
    mg, sh, st = check_clearance_args(margin, skip)
    O.L.require_gpu(trajectories, trajectory_mask, scene, scene_mask)
    P = O._c(trajectories.detach().float())
    tm = _mask_bytes(trajectory_mask)
    dev = P.device
    nearest = torch.empty((B, G, Ln), device=dev, dtype=torch.float32)
    clearance = torch.empty((B, G), device=dev, dtype=torch.float32)
    ws = scan_workspace("a3d_traj_clearance", B, G, Ln, sc.n_cam * sc.n_pix, dev)
    O.L.call("a3d_traj_clearance", P.data_ptr(), tm.data_ptr(), sc.cloud.data_ptr(), None if sc.mask is None else sc.mask.data_ptr(),
             sc.n_cam, sc.n_pix, mg, sh, st, nearest.data_ptr(), clearance.data_ptr(), ws.data_ptr(), 0, B, G, Ln, Dp, O.L.stream())
    return TrajectoryClearance(nearest, clearance)


# ------------------------------------------------------------------------------------------------ body-aware swept clearance
BODY_MAX_SPHERES = O.L.TRAJ_BODY_MAX_SPHERES        # spheres of one body (a3d_traj_body_clearance)
# a gripper body: sphere centres in the TOOL frame (K, 3) and radii (K,), in metres; sweep: score the segment to the next waypoint.
# No preset ships: where the fingers and the palm lie in the tool frame depends on the robot and on the frame convention of the data.
GripperBody = collections.namedtuple("GripperBody", ("offsets", "radii", "sweep"), defaults=(True,))


def check_body(body, device=None):
    """Validates a gripper body and returns GripperBody(offsets (K, 3) fp32, radii (K,) fp32, sweep bool), the tensors on `device`
    (None: where they are).  body: a GripperBody or a dict with "offsets", "radii" and optionally "sweep" (default True); offsets
    and radii are tensors or nested sequences of numbers.  ValueError for wrong ranks or shapes, K outside 1 .. 8, a sweep that is not
    a bool (or 0 / 1), non-finite offsets, negative or non-finite radii.  The values are checked where the tensors live on the
    host; tensors already on a device are NOT copied back for it (no synchronisation): a non-finite offset then gives NaN rows, a
    NaN radius a NaN `nearest`, in the kernel."""
    if isinstance(body, dict):
        bad = [k for k in body if k not in GripperBody._fields]
        if bad or "offsets" not in body or "radii" not in body:
            raise ValueError("body: a dict with the keys 'offsets', 'radii' and optionally 'sweep', got %s" % sorted(body))
        offsets, radii, sweep = body["offsets"], body["radii"], body.get("sweep", True)
    elif isinstance(body, tuple) and all(hasattr(body, k) for k in GripperBody._fields):
        offsets, radii, sweep = body.offsets, body.radii, body.sweep
    else:
        raise ValueError("body must be a GripperBody or a dict with offsets, radii and sweep, got %s" % type(body).__name__)
    if isinstance(sweep, bool) or (isinstance(sweep, int) and sweep in (0, 1)):
        sweep = bool(sweep)
    else:
        raise ValueError("body: sweep must be a bool, got %r" % (sweep,))
    try:
        offsets = offsets.detach() if torch.is_tensor(offsets) else torch.as_tensor(offsets, dtype=torch.float32)
        radii = radii.detach() if torch.is_tensor(radii) else torch.as_tensor(radii, dtype=torch.float32)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError("body: offsets and radii must be tensors or nested sequences of numbers (%s)" % e) from None
    if offsets.dim() != 2 or offsets.shape[1] != 3:
        raise ValueError("body: offsets must be (K, 3) sphere centres in the tool frame, got %s" % (tuple(offsets.shape),))
    K = offsets.shape[0]
    if not 1 <= K <= BODY_MAX_SPHERES:
        raise ValueError("body: K = %d spheres, a body has 1 to %d" % (K, BODY_MAX_SPHERES))
    if tuple(radii.shape) != (K,):
        raise ValueError("body: radii must be (K,) = (%d,), got %s" % (K, tuple(radii.shape)))
    for name, x in (("offsets", offsets), ("radii", radii)):
        if not (x.is_floating_point() or x.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
            raise ValueError("body: %s must hold numbers, got %s" % (name, x.dtype))
    if not offsets.is_cuda and not bool(torch.isfinite(offsets.float()).all()):
        raise ValueError("body: offsets must be finite")
    if not radii.is_cuda and not bool((torch.isfinite(radii.float()) & (radii.float() >= 0)).all()):
        raise ValueError("body: radii must be finite and >= 0")
    offsets = O._c(offsets.to(device=device, dtype=torch.float32))
    radii = O._c(radii.to(device=device, dtype=torch.float32))
    return GripperBody(offsets, radii, sweep)


def body_clearance(trajectories, trajectory_mask, scene, body, scene_mask=None, margin=0.05, skip=(1, 1)):
    """trajectory_clearance for a gripper BODY instead of the tool point, in THREE launches (a3d_traj_body_clearance,
    csrc/traj_body.hip): K <= 8 spheres in the tool frame, rotated with every waypoint's quaternion (the matrix pose_to_signal
    emits, completed by its third column), each swept along the straight segment of its centre to the next valid waypoint.
    trajectories, trajectory_mask, scene, scene_mask, margin, skip: the arguments of trajectory_clearance, except that the
    quaternion (w, x, y, z) of a pose row is read as well.  body: check_body.
    With j the rank of a valid row among the n valid rows of its scene, the end row of row j is the row of rank j + 1 when
    body.sweep is set and j + 1 < n - skip[1], else the row itself: gaps of the mask are stepped over, the approach to the goal row
    is not swept with the default skip (contact is intended there), the last scored row is a degenerate segment.  Sphere k of row j
    moves from a = p_j + R(q_j) o_k to c = p_e + R(q_e) o_k on a straight line (a capsule; the rotation is not interpolated inside
    a segment).  Returns TrajectoryClearance(nearest (B, G, L), clearance (B, G)): nearest = min_k (distance of the segment to the
    nearest counted point - r_k), SIGNED (negative: a sphere contains a scene point), +inf without a counted point and on padded
    rows, NaN where a sphere centre of the row or of its end row is not finite (a zero quaternion included); clearance = the mean
    over the scored rows of max(0, margin - nearest) / margin, NOT clamped above (in [0, 1 + max r / margin]: penetration costs
    more than touching), 0 without a scored row, NaN as soon as a scored row is NaN.  offsets and radii are read by the kernels at
    launch time: a captured call replayed after they were changed in place sees the new values (give device tensors to a call that
    is captured: host values are copied to the device first).  With one sphere of radius 0 at the
    tool point and sweep=False this is trajectory_clearance, bit for bit.  Bit-identical from run to run.
    No preset body ships: sphere positions in the tool frame depend on the robot and on the data's frame convention, and neither
    has been verified here.  A worked example with MADE-UP numbers (a palm sphere and two finger-tip spheres of a parallel gripper
    whose fingers point along the tool frame's +z and open along its y):
        body = GripperBody(offsets=[[0.0, 0.0, -0.06], [0.0, 0.04, 0.0], [0.0, -0.04, 0.0]], radii=[0.04, 0.015, 0.015])"""
    B, G, Ln, Dp = _check_candidates(trajectories, trajectory_mask)
    sc = prepare_scene(scene, scene_mask, B)
    mg, sh, st = check_clearance_args(margin, skip)
    body = check_body(body)
    O.L.require_gpu(trajectories, trajectory_mask, scene, scene_mask)
    P = O._c(trajectories.detach().float())
    body = check_body(body, P.device)                        # already on the device: nothing is copied, nothing is read back
    K = body.offsets.shape[0]
    tm = _mask_bytes(trajectory_mask)
    dev = P.device
    nearest = torch.empty((B, G, Ln), device=dev, dtype=torch.float32)
    clearance = torch.empty((B, G), device=dev, dtype=torch.float32)
    n = O.L.load().a3d_traj_body_clearance_ws_floats(B, G, Ln, K, sc.n_cam * sc.n_pix, 0)
    ws = torch.empty((n,), device=dev, dtype=torch.float32)
    O.L.call("a3d_traj_body_clearance", P.data_ptr(), tm.data_ptr(), body.offsets.data_ptr(), body.radii.data_ptr(), K,
             1 if body.sweep else 0, sc.cloud.data_ptr(), None if sc.mask is None else sc.mask.data_ptr(), sc.n_cam, sc.n_pix, mg, sh, st,
             nearest.data_ptr(), clearance.data_ptr(), ws.data_ptr(), 0, B, G, Ln, Dp, O.L.stream())
    return TrajectoryClearance(nearest, clearance)


# ------------------------------------------------------------------------------------------------ clearance guidance
GUIDE_MAX_ROWS = 256                    # a3d_traj_guide: one thread per row of a trajectory
GUIDE_KEYS = ("push", "smooth", "start")
Guidance = collections.namedtuple("Guidance", ("steps", "nearest"))


def check_guide_args(push, smooth):
    """-> (push, smooth) of a guide step as floats, or ValueError: both in [0, 1], not both 0"""
    for name, v in (("push", push), ("smooth", smooth)):
        _number(name, v, "must be a number in [0, 1]", lo=0, hi=1)
    if push == 0 and smooth == 0:
        raise ValueError("push and smooth are both 0: the guide step would do nothing")
    return float(push), float(smooth)


def check_guide(guide):
    """compute_trajectory's `guide` -> None, or (push, smooth, start): a number is the push; a dict maps a subset of "push" (default
    1.0), "smooth" (0.0) and "start" (0.5, in [0, 1)) to numbers, unknown keys raise"""
    if guide is None:
        return None
    if isinstance(guide, dict):
        bad = [k for k in guide if k not in GUIDE_KEYS]
        if bad:
            raise ValueError("guide has unknown keys %s; the keys are %s" % (bad, list(GUIDE_KEYS)))
        push, smooth, start = guide.get("push", 1.0), guide.get("smooth", 0.0), guide.get("start", 0.5)
    elif isinstance(guide, (int, float)) and not isinstance(guide, bool):
        push, smooth, start = guide, 0.0, 0.5
    else:
        raise ValueError("guide must be None, a number (the push) or a dict over %s, got %r" % (list(GUIDE_KEYS), guide))
    push, smooth = check_guide_args(push, smooth)
    return push, smooth, float(_number("guide['start']", start, "must be a number in [0, 1)", lo=0, below=1))


def check_guide_shape(G, Ln, D):
    """what a3d_traj_guide serves: G candidates per scene, Ln rows, D signal channels"""
    if G > RANK_MAX_CANDIDATES:
        raise ValueError("the guide step serves at most %d candidates per scene, got %d" % (RANK_MAX_CANDIDATES, G))
    if Ln > GUIDE_MAX_ROWS:
        raise ValueError("the guide step serves at most %d rows per trajectory, got L = %d" % (GUIDE_MAX_ROWS, Ln))
    if D not in (9, 10):
        raise ValueError("the guide step reads signal rows of 9 or 10 channels, got %d" % D)


def guided_segments(n, start):
    """The launch list of a sampling loop of n executed steps guided from `start` on: [(first, count, guided)] over step POSITIONS.
    Step position i is guided iff i >= floor(start n) (so the terminal step always is; 1e-9 is added before the floor, so that a
    start written as i / n means position i whatever its rounding).  Each maximal run of unguided steps is ONE entry (one sampler
    launch where the path runs several steps per launch); each guided step is an entry of its own: a one-step sampler launch, then
    the guide pair.  start None: the whole loop, unguided."""
    n = int(n)
    if start is None:
        return [(0, n, False)]
    if n < 1:
        return []
    g0 = min(n - 1, max(0, int(math.floor(start * n + 1e-9))))
    return ([(0, g0, False)] if g0 > 0 else []) + [(i, 1, True) for i in range(g0, n)]


def _guide_launch(x, tm, cm, bounds, sc, margin, sh, st, push, smooth, nearest, ws, B, G, Ln):
    """a3d_traj_guide on prepared buffers: x (B G, L, D) contiguous fp32 signals, updated in place; sc: a Scene"""
    O.L.call("a3d_traj_guide", x.data_ptr(), x.shape[-1], tm.data_ptr(), None if cm is None else cm.data_ptr(), bounds.data_ptr(),
             sc.cloud.data_ptr(), None if sc.mask is None else sc.mask.data_ptr(), sc.n_cam, sc.n_pix, margin, sh, st, push, smooth,
             None if nearest is None else nearest.data_ptr(), ws.data_ptr(), 0, B, G, Ln, O.L.stream())


def guide_trajectories(signals, trajectory_mask, scene, bounds, *, scene_mask=None, cond_mask=None, margin=0.05, skip=(1, 1),
                       push=1.0, smooth=0.0, want_nearest=False):
    """One clearance-guidance step on trajectory signals, IN PLACE, in two launches (a3d_traj_guide, csrc/traj_guide.hip): every
    free waypoint closer than `margin` to its nearest counted scene point is moved `push` of the way out to the margin sphere of that
    point, and `smooth` of the way to the midpoint of its two neighbouring valid rows (all positions read before any update).
    signals: (B, G, L, D) or (B, L, D) contiguous fp32, D = 9 or 10, as the sampler holds them (trace entries of compute_trajectory):
    channels 0..2 are positions normalised to `bounds` (2, 3); nothing else is read or written.  trajectory_mask (B, L), non-zero =
    padded row; scene / scene_mask / margin / skip: the arguments of trajectory_clearance, `scene` in world coordinates.
    cond_mask: None or the sampler's in-painting mask, B G L D bytes (bool or uint8): a row whose first byte is set is pinned.
    A row is free when it is valid, scored by the skip rule (skip[0] <= j < n - skip[1] over its rank j among the n valid rows), not
    pinned and finite; every other row keeps its bits, pinned rows still anchor the smoothing of their neighbours.
    Returns nearest (the shape of signals without D: the distance to the nearest counted point BEFORE the push, +inf on padded rows
    and without a counted point, NaN where the row is not finite) with want_nearest, else None.  Bit-identical from run to run."""
    if not torch.is_tensor(signals) or signals.dim() not in (3, 4):
        raise ValueError("signals must be a (B, G, L, D) or (B, L, D) tensor, got %s" % (
            tuple(signals.shape) if torch.is_tensor(signals) else type(signals).__name__,))
    if signals.dtype != torch.float32 or not signals.is_contiguous():
        raise ValueError("signals are updated in place: they must be contiguous fp32, got %s%s" % (
            signals.dtype, "" if signals.is_contiguous() else " (not contiguous)"))
    B, G, Ln, D = signals.shape if signals.dim() == 4 else (signals.shape[0], 1) + tuple(signals.shape[1:])
    if min(B, G, Ln) < 1:
        raise ValueError("signals has an empty dimension: %s" % (tuple(signals.shape),))
    check_guide_shape(G, Ln, D)
    check_trajectory_mask(trajectory_mask, B, Ln)
    sc = prepare_scene(scene, scene_mask, B)
    mg, sh, st = check_clearance_args(margin, skip)
    push, smooth = check_guide_args(push, smooth)
    if cond_mask is not None:
        if not torch.is_tensor(cond_mask) or cond_mask.numel() != signals.numel() or cond_mask.shape[-1] != D:
            raise ValueError("cond_mask must hold one byte per signal element, (B G, L, D) = %s, got %s" % (
                (B * G, Ln, D), tuple(cond_mask.shape) if torch.is_tensor(cond_mask) else type(cond_mask).__name__))
        if cond_mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError("cond_mask must be bool or uint8, got %s" % cond_mask.dtype)
    if not torch.is_tensor(bounds):
        bounds = torch.as_tensor(bounds, dtype=torch.float32)
    if tuple(bounds.shape) != (2, 3):
        raise ValueError("bounds must be (2, 3), got %s" % (tuple(bounds.shape),))
    bounds = bounds.to(device=signals.device, dtype=torch.float32)
    O.L.require_gpu(signals, trajectory_mask, scene, scene_mask, cond_mask)
    dev = signals.device
    nearest = torch.empty(signals.shape[:-1], device=dev, dtype=torch.float32) if want_nearest else None
    ws = scan_workspace("a3d_traj_guide", B, G, Ln, sc.n_cam * sc.n_pix, dev)
    _guide_launch(signals, _mask_bytes(trajectory_mask), None if cond_mask is None else _mask_bytes(cond_mask), O._c(bounds), sc, mg, sh,
                  st, push, smooth, nearest, ws, B, G, Ln)
    return nearest


def rank_trajectories(trajectories, trajectory_mask, goal=None, bounds=None, select="consensus", rot_weight=1.0, scene=None,
                      scene_mask=None, margin=0.05, skip=(1, 1), body=None):
    """Ranks the G candidate trajectories of every scene and selects one, in ONE launch (a3d_traj_rank, csrc/traj_rank.hip); nothing
    is copied to the host.  trajectories: (B, G, L, Dp) fp32 poses [xyz | quaternion | opening], Dp = 7 or 8, scene-major as
    compute_trajectory(num_samples=G) returns them, G <= 64; trajectory_mask: (B, L), non-zero = padded row (any pattern); goal:
    (B, >= 7) pose rows, read in place where they are row slices of a wider tensor; bounds: (2, 3).
    Terms per candidate over the valid rows: "consensus" (mean pose distance to all candidates of the scene: its argmin is the
    medoid), "goal" (pose distance of the last valid row to the goal), "smooth" (mean squared second difference of the positions),
    "length" (path length), "bounds" (share of rows outside the bounds); pose distance = position L2 + rot_weight (1 - <q, r>^2).
    rot_weight = 1.0 is a choice, not a derived value: it prices a half turn (rho = 1) like one metre.  select: a preset name or a
    dict of term weights (check_select).  Returns TrajectoryRanking(best (B,) int32, order (B, G) int32 ascending and stable,
    scores (B, G), terms (B, G, 5), selected (B, L, Dp) = trajectories[b, best[b]]); a non-finite score counts as +inf.
    scene / scene_mask / margin / skip: the arguments of trajectory_clearance.  A rule that weighs "clearance" (a dict entry, or the
    preset "clear") needs `scene`; the score is then the five-term sum plus w_clearance * clearance, added last, the call runs
    trajectory_clearance's two launches before the ranking launch (a3d_traj_rank_extra, the same kernel) and returns
    SceneTrajectoryRanking: the five fields above in order, then clearance (B, G) and nearest (B, G, L).  A rule that does not weigh
    the term runs the one launch above and returns TrajectoryRanking, whatever `scene` is.
    body: None or a gripper body (check_body).  With a rule that weighs "clearance" the term and `nearest` then come from
    body_clearance (three launches instead of two); with any other rule the body is checked and otherwise ignored, as `scene` is."""
    B, G, Ln, Dp = _check_candidates(trajectories, trajectory_mask)
    if goal is not None and (not torch.is_tensor(goal) or goal.dim() != 2 or goal.shape[0] != B or goal.shape[1] < 7):
        raise ValueError("goal must be (B, >= 7) pose rows with B = %d, got %s" % (
            B, tuple(goal.shape) if torch.is_tensor(goal) else type(goal).__name__))
    if bounds is not None:
        bounds = torch.as_tensor(bounds, dtype=torch.float32, device=trajectories.device)
        if tuple(bounds.shape) != (2, 3):
            raise ValueError("bounds must be (2, 3), got %s" % (tuple(bounds.shape),))
    w, wc = check_scene_select(select, goal is not None, bounds is not None, scene is not None)
    rw = check_rot_weight(rot_weight)
    if body is not None:
        body = check_body(body)
    if wc != 0.0:
        check_scene(scene, scene_mask, B)
        check_clearance_args(margin, skip)
    O.L.require_gpu(trajectories, trajectory_mask, goal, bounds)
    P = O._c(trajectories.detach().float())
    tm = _mask_bytes(trajectory_mask)
    gl, ldg = (None, 0) if goal is None else _pose_rows(goal, "goal")
    dev = P.device
    best = torch.empty((B,), device=dev, dtype=torch.int32)
    order = torch.empty((B, G), device=dev, dtype=torch.int32)
    scores = torch.empty((B, G), device=dev, dtype=torch.float32)
    terms = torch.empty((B, G, 5), device=dev, dtype=torch.float32)
    selected = torch.empty((B, Ln, Dp), device=dev, dtype=torch.float32)
    args = (P.data_ptr(), tm.data_ptr(), None if gl is None else gl.data_ptr(), ldg, None if bounds is None else O._c(bounds).data_ptr(),
            w[0], w[1], w[2], w[3], w[4], rw, best.data_ptr(), order.data_ptr(), scores.data_ptr(), terms.data_ptr(), selected.data_ptr(),
            B, G, Ln, Dp)
    if wc != 0.0:
        cl = trajectory_clearance(P, tm, scene, scene_mask, margin, skip) if body is None else \
            body_clearance(P, tm, scene, body, scene_mask, margin, skip)
        O.L.call("a3d_traj_rank_extra", *args, cl.clearance.data_ptr(), wc, O.L.stream())
        return SceneTrajectoryRanking(best, order, scores, terms, selected, cl.clearance, cl.nearest)
    O.L.call("a3d_traj_rank", *args, O.L.stream())
    return TrajectoryRanking(best, order, scores, terms, selected)
