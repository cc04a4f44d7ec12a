"""Chained keypose-to-trajectory inference: the reference's `Actioner.predict`
(online_evaluation/utils_with_rlbench.py:120-230) as one call on the MI355X hot path.

`predict` runs the Act3D keypose forward on the last observation, concatenates position | rotation | gripper into an action and
hands action[..., :action_dim] to `DiffusionPlanner.compute_trajectory` as the goal pose.  Same constructor keywords, same
`load_episode` / `predict` semantics and the same output dictionary as the reference.  What the chained call saves over the two
calls written out by hand, with identical results:
  * ONE pass of the frozen backbone when both models hold the same backbone (`share_backbone`): its maps feed both FPNs;
  * the conditioning seam of the sampler (pose conversions, in-painting data / mask, key mask, noisy start trajectory) in ONE
    launch (`fused_conditioning`, a3d_traj_condition) instead of ~25 small ones;
  * `predict(use_graph=True)`: one captured graph for the keypose half, followed by the sampler's own captured loop.
Additive: constructor keywords `share_backbone`, `fused_conditioning`; `set_instruction` (RLBench's TASK_TO_ID table is not
needed: `load_episode` only picks the instruction); keyword-only arguments of `predict` (`use_graph`, `ghost_points` and the
sampling options of compute_trajectory, `select` / `rot_weight` for the on-device choice among `num_samples` candidates included).
Nothing in `predict` copies from the device to the host.
"""
import random

import torch

from .diffusion import check_sampling_call, _graph_replay
from .trajectory import check_trajectory_mask

_TRAJ_KW = ("num_samples", "num_inference_steps", "scheduler", "eta", "init_noise", "step_noise", "n_steps", "select", "rot_weight",
            "scene_mask", "clear_margin", "clear_skip", "guide", "solver_order", "lower_order_final", "pins", "clear_body")


def _same_tensors(a, b):
    """the two state dicts hold the same names with identical tensors.  run_frozen_backbone converts a backbone's convolution
    weights to its reduced dtype at the first pass: a tensor one side has already converted is compared in that dtype"""
    if a.keys() != b.keys():
        return False
    for k, x in a.items():
        y = b[k]
        if x.shape != y.shape or x.device != y.device:
            return False
        if x.dtype != y.dtype:
            narrow = x.dtype if x.element_size() < y.element_size() else y.dtype
            x, y = x.to(narrow), y.to(narrow)
        if not torch.equal(x, y):
            return False
    return True


def backbones_identical(keypose_model, traj_model):
    """Both models carry a frozen backbone (and its input normalisation) with identical tensors."""
    head = getattr(traj_model, "prediction_head", None)
    a, b = getattr(keypose_model, "backbone", None), getattr(head, "backbone", None)
    if a is None or b is None:
        return False
    if a is b:
        return True
    if type(a) is not type(b) or not _same_tensors(a.state_dict(), b.state_dict()):
        return False
    na, nb = getattr(keypose_model, "normalize", None), getattr(head, "normalize", None)
    if (na is None) != (nb is None):
        return False
    return na is None or (type(na) is type(nb) and _same_tensors(dict(na.named_buffers()), dict(nb.named_buffers())))


class Actioner:

    def __init__(self, keypose_model=None, traj_model=None, instructions=None,
                 apply_cameras=("left_shoulder", "right_shoulder", "wrist"), action_dim=7, predict_keypose=True,
                 predict_trajectory=False, *, share_backbone="auto", fused_conditioning=True):
        if action_dim not in (7, 8):
            raise ValueError("action_dim must be 7 (pose) or 8 (pose + gripper opening), got %r" % (action_dim,))
        if not (share_backbone == "auto" or share_backbone is True or share_backbone is False):
            raise ValueError("share_backbone must be 'auto', True or False, got %r" % (share_backbone,))
        if predict_keypose and keypose_model is None:
            raise ValueError("predict_keypose=True needs a keypose_model")
        if predict_trajectory and traj_model is None:
            raise ValueError("predict_trajectory=True needs a traj_model")
        if predict_keypose and str(getattr(keypose_model, "rotation_parametrization", "")).startswith("6D"):
            # the chained goal is action[..., :7] = position | quaternion: a 6D head's action rows do not hold one
            raise ValueError("the keypose model has a 6D rotation head (%s): action[..., :%d] is a goal pose only for quaternion "
                             "heads" % (keypose_model.rotation_parametrization, action_dim))
        self._keypose_model, self._traj_model = keypose_model, traj_model
        self._instructions = instructions
        self._apply_cameras = apply_cameras
        self._action_dim = action_dim
        self._predict_keypose, self._predict_trajectory = predict_keypose, predict_trajectory
        self._fused_conditioning = bool(fused_conditioning)
        self._share_backbone = share_backbone
        self._actions = {}
        self._instr = None
        self._task_str = None
        self._instr_cache = None
        self._graph = None
        self.last_backbone_passes = 0
        self.last_ranking = None
        self.last_pins = None
        if predict_keypose:
            keypose_model.eval()
        if predict_trajectory:
            traj_model.eval()
        # the weights are compared once, here (after eval(): nothing updates the frozen backbone's buffers from now on); the dtype
        # attributes of the two models may still be set afterwards and are compared at every call
        self._same_backbone = bool(predict_keypose and predict_trajectory and share_backbone is not False and
                                   backbones_identical(keypose_model, traj_model))
        if share_backbone is True:
            self._sharing(check=True)

    # ------------------------------------------------------------------------------------------------ sharing rule
    def _sharing(self, check=False):
        """One backbone pass serves both models: identical backbone tensors, the same backbone_dtype, and both FPNs asking for the
        same kind of maps (run_frozen_backbone's keep_dtype = a reduced fpn_dtype).  check: raise where that does not hold."""
        why = None
        if not (self._predict_keypose and self._predict_trajectory):
            why = "it takes both predict_keypose and predict_trajectory"
        elif self._share_backbone is False:
            return False
        elif not self._same_backbone:
            why = "the two models' backbones do not hold identical tensors"
        else:
            kp, head = self._keypose_model, self._traj_model.prediction_head
            if kp.backbone_dtype != head.backbone_dtype:
                why = "backbone_dtype differs (%s, %s)" % (kp.backbone_dtype, head.backbone_dtype)
            elif (kp.fpn_dtype != torch.float32) != (head.fpn_dtype != torch.float32):
                why = "the FPNs ask for different maps (fpn_dtype %s, %s)" % (kp.fpn_dtype, head.fpn_dtype)
        if why is not None and (check or self._share_backbone is True):
            raise ValueError("share_backbone=True, but the backbone pass cannot be shared: " + why)
        return why is None

    @property
    def shares_backbone(self):
        return self._sharing()

    # ------------------------------------------------------------------------------------------------ instruction
    def load_episode(self, task_str, variation):
        self._task_str = task_str
        instructions = list(self._instructions[task_str][variation])
        self.set_instruction(random.choice(instructions))
        self._actions = {}

    def set_instruction(self, instr):
        """The instruction embedding of the episode: (53, 512), (1, 53, 512) or one per scene (B, 53, 512)."""
        if not torch.is_tensor(instr) or instr.dim() not in (2, 3):
            raise ValueError("an instruction is a (n_words, 512) tensor, optionally with a leading batch dimension")
        self._instr = instr if instr.dim() == 3 else instr.unsqueeze(0)
        self._instr_cache = None

    def _instruction(self, B, device):
        c = self._instr_cache
        if c is None or c[0] != (B, device):
            x = self._instr.to(device)
            if x.shape[0] != B:
                x = x.expand(B, -1, -1)
            self._instr_cache = ((B, device), x.contiguous())
        return self._instr_cache[1]

    @property
    def device(self):
        for m in (self._keypose_model, self._traj_model):
            if m is not None:
                return next(m.parameters()).device

    # ------------------------------------------------------------------------------------------------ host-side checks
    def _check(self, rgbs, pcds, gripper, gt_action, trajectory_mask, use_graph, ghost_points):
        if self._instr is None:
            raise ValueError("no instruction is set: call load_episode or set_instruction first")
        for name, x, rank in (("rgbs", rgbs, 6), ("pcds", pcds, 6), ("gripper", gripper, 3)):
            if not torch.is_tensor(x) or x.dim() != rank:
                raise ValueError("%s must have %d dimensions %s, got %s" % (
                    name, rank, "(B, history, cameras, 3, H, W)" if rank == 6 else "(B, history, >= action_dim)",
                    tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if rgbs.shape[0] != pcds.shape[0] or rgbs.shape[0] != gripper.shape[0]:
            raise ValueError("rgbs, pcds and gripper disagree on the batch size: %d, %d, %d" % (
                rgbs.shape[0], pcds.shape[0], gripper.shape[0]))
        if rgbs.shape[2] != pcds.shape[2]:
            raise ValueError("rgbs and pcds disagree on the number of cameras: %d, %d" % (rgbs.shape[2], pcds.shape[2]))
        if gripper.shape[-1] < self._action_dim:
            raise ValueError("gripper rows have %d channels, action_dim is %d" % (gripper.shape[-1], self._action_dim))
        B = rgbs.shape[0]
        if self._instr.shape[0] not in (1, B):
            raise ValueError("the instruction has %d rows for a batch of %d" % (self._instr.shape[0], B))
        if not self._predict_keypose:
            if gt_action is None:
                raise ValueError("predict_keypose=False needs gt_action (B, history, >= action_dim)")
            if gt_action.dim() != 3 or gt_action.shape[0] != B or gt_action.shape[-1] < self._action_dim:
                raise ValueError("gt_action must be (B, history, >= action_dim), got %s" % (tuple(gt_action.shape),))
        if self._predict_trajectory:
            if trajectory_mask is None:
                raise ValueError("predict_trajectory=True needs a trajectory_mask (B, L)")
            check_trajectory_mask(trajectory_mask, B)
        if use_graph and self._predict_keypose and ghost_points is None and \
                getattr(self._keypose_model, "ghost_sampler", "philox") != "philox":
            raise ValueError("use_graph=True needs the device ghost-point sampler (ghost_sampler='philox'): the host sampler copies "
                             "the anchor to the host at every level")

    # ------------------------------------------------------------------------------------------------ the keypose half
    def _keypose_half(self, rgb_raw, pcd, instr, curr, ghost_points, share):
        """rescale -> (one backbone pass) -> Act3D's FPN and evaluation forward -> the action cat; with `share` also the planner's
        FPN tokens on the same maps.  Every launch is stream-ordered and nothing touches the host: capturable."""
        kp = self._keypose_model
        rgb = rgb_raw / 2 + 0.5                                          # in [0, 1]
        tokens = None
        if share:
            maps = kp.backbone_maps(rgb)
            feats = kp.compute_visual_tokens(rgb, maps=maps)
            pred = kp(rgb, pcd, instr, curr, ghost_points=ghost_points, visual_features=feats)
            # encode_images reads the images' shape and the maps only (its coordinate argument is not used by the FPN)
            tokens = self._traj_model.prediction_head.encode_images(rgb, None, maps=maps)
        else:
            pred = kp(rgb, pcd, instr, curr, ghost_points=ghost_points)
        action = torch.cat([pred["position"], pred["rotation"], pred["gripper"]], dim=1)
        return {"rgb": rgb, "action": action, "tokens": tokens, "pred": pred}

    def _keypose_graphed(self, rgb_raw, pcd, instr, curr, ghost_points, share):
        kp = self._keypose_model
        ins = [rgb_raw, pcd, instr, curr] + list(ghost_points or [])
        key = (tuple((tuple(t.shape), t.dtype, t.device) for t in ins), ghost_points is not None, share,
               kp.backbone_dtype, kp.fpn_dtype,
               None if not share else (self._traj_model.prediction_head.backbone_dtype, self._traj_model.prediction_head.fpn_dtype))

        def capture():
            # "static" and "out" keep every buffer the captured launches address alive
            static = [t.clone() for t in ins]
            run = lambda: self._keypose_half(static[0], static[1], static[2], static[3], static[4:] if ghost_points is not None else None,
                                             share)
            # the warm-up (allocator, lazy module state, the convolution library's algorithm choice) must not consume ghost-point
            # draws: the sampler state is put back, so a replay draws what an eager call would
            rng = kp._rng_state.clone() if hasattr(kp, "_rng_state") else None
            return run, {"static": static}, None if rng is None else (lambda: kp._rng_state.copy_(rng))

        self._graph = _graph_replay(self._graph, key, capture, ins)
        return self._graph["out"]

    # ------------------------------------------------------------------------------------------------ predict
    @torch.no_grad()
    def predict(self, rgbs, pcds, gripper, gt_action=None, trajectory_mask=None, *, use_graph=False, ghost_points=None,
                **sample_kw):
        """rgbs (B, history, cameras, 3, H, W) in [-1, 1]; pcds alike; gripper (B, history, >= action_dim); gt_action
        (B, history, >= action_dim), read only with predict_keypose=False; trajectory_mask (B, L), needed with
        predict_trajectory=True.  Returns {"action": (B, 8) or gt_action[:, -1], "trajectory": compute_trajectory's result or None,
        "attention": {}}.  sample_kw (num_samples, num_inference_steps, scheduler, eta, init_noise, step_noise, n_steps, select,
        rot_weight, scene_mask, clear_margin, clear_skip, guide, solver_order, lower_order_final, pins, clear_body) go to compute_trajectory unchanged (a rule that weighs "clearance"
        scores the candidates against pcds[:, -1] -- with clear_body, a gripper body of swept spheres (trajectory.body_clearance), instead of the tool point -- and `guide` steers the waypoints off that cloud while they are drawn); with select the candidates are ranked on the device, "trajectory" is the
        selected one (B, L, 8) and self.last_ranking mirrors the planner's; with pins (trajectory.check_pins, pose rows of action_dim
        channels; trajectory.prefix_pins for a replan that keeps what the robot is executing) self.last_pins mirrors the planner's; ghost_points to Act3D; use_graph replays the keypose half
        and the sampling loop as graphs."""
        bad = [k for k in sample_kw if k not in _TRAJ_KW]
        if bad:
            raise TypeError("predict() got unexpected keyword arguments %s" % bad)
        if not self._predict_trajectory:
            if sample_kw.get("select") is not None:
                raise ValueError("select ranks sampled trajectories: it needs predict_trajectory=True")
            if sample_kw.get("guide") is not None:
                raise ValueError("guide steers sampled trajectories: it needs predict_trajectory=True")
            if sample_kw.get("pins") is not None:
                raise ValueError("pins are waypoints of sampled trajectories: they need predict_trajectory=True")
        self._check(rgbs, pcds, gripper, gt_action, trajectory_mask, use_graph, ghost_points)
        if self._predict_trajectory:
            # the sampling call's own argument errors, before the keypose half launches anything (the schedule and the noise
            # tables stay compute_trajectory's: it knows the chain length)
            check_sampling_call(pcds.shape[0], trajectory_mask.shape[1], self._action_dim + 2, None, pcds[:, -1], True, **sample_kw)
        share = self._sharing()
        output = {"action": None, "attention": {}}
        B = rgbs.shape[0]
        instr = self._instruction(B, rgbs.device)
        pcd = pcds[:, -1].contiguous()
        curr = gripper[:, -1, :self._action_dim]
        passes, tokens, rgb = 0, None, None
        if self._predict_keypose:
            rgb_raw = rgbs[:, -1]
            if use_graph:
                half = self._keypose_graphed(rgb_raw.contiguous(), pcd, instr, curr.contiguous(), ghost_points, share)
            else:
                half = self._keypose_half(rgb_raw, pcd, instr, curr, ghost_points, share)
            rgb, tokens = half["rgb"], half["tokens"]
            # a replay writes the graph's own buffers: the caller gets a copy the next call does not overwrite
            output["action"] = half["action"].clone() if use_graph else half["action"]
            self.last_keypose_output = half["pred"]
            passes += 1
        else:
            output["action"] = gt_action[:, -1]
        if self._predict_trajectory:
            if rgb is None:
                rgb = rgbs[:, -1] / 2 + 0.5
            output["trajectory"] = self._traj_model.compute_trajectory(
                trajectory_mask, rgb, pcd, instr, curr, output["action"][..., :self._action_dim], visual_tokens=tokens,
                use_graph=use_graph, fused_conditioning=self._fused_conditioning, **sample_kw)
            passes += 0 if tokens is not None else 1
            if sample_kw.get("select") is not None:
                self.last_ranking = self._traj_model.last_ranking
            self.last_pins = self._traj_model.last_pins
        else:
            output["trajectory"] = None
        self.last_backbone_passes = passes
        return output
