"""ChainedDiffuser trajectory DDPM on the MI355X hot path.

Drop-in for `model.DiffusionPlanner` (model/trajectory_optimization/diffusion_model.py:15-324) and its
`DiffusionHead` (diffusion_head.py:10-363, on top of model/utils/encoder.py): same constructor keywords, same
`forward(gt_trajectory, trajectory_mask, rgb_obs, pcd_obs, instruction, curr_gripper, goal_gripper, run_inference)`
and `compute_trajectory(...)`, same parameter names (checkpoints interchange).

What is restructured, with identical results:
  * everything that does not depend on the denoising step -- image encoding, instruction encoding, vision->language
    attention, gripper tokens and the K/V projections (+RoPE) of all cross-attention layers -- is computed ONCE per
    trajectory batch (`encode_context`, `build_kv_cache`) instead of once per step;
  * one denoise step is a fixed sequence of stream-ordered launches (no host sync: the boolean-mask scatter becomes a
    masked select in the fused DDPM-step kernel, timestep tables live on the device), so the whole 100-step loop is
    captured in a hipGraph and replayed (`compute_trajectory(..., use_graph=True)`).
The DDPM schedules restate diffusers' DDPMScheduler (third-party, un-pinned -> parity unpinned).
Additive keyword arguments: `noise`, `timesteps` (training) and `init_noise`, `step_noise` (sampling) inject the random
draws; `visual_tokens` bypasses the backbone + FPN; `num_inference_steps` / `scheduler` / `eta` select a few-step sampler
schedule (`scheduler="dpm++"` with `solver_order` / `lower_order_final`: the DPM-Solver++ 2M multistep solver); `num_samples=G` samples G candidate trajectories per scene from one shared context K/V cache -> (B, G, L, 8);
`fused_conditioning=True` builds the sampler's conditioning tensors in one launch (a3d_traj_condition); `select` / `rot_weight`
rank the candidates on the device and return the selected trajectory (rank_trajectories, a3d_traj_rank), optionally against the
observed point cloud (trajectory_clearance, a3d_traj_clearance: the "clearance" term of a select rule); `guide` steers the waypoints
off that cloud while they are drawn (guide_trajectories, a3d_traj_guide, between sampler steps); `pins` keeps a committed prefix or
via-points of the trajectory while the rest is sampled (traj_pins, a3d_traj_pins; prefix_pins for a receding-horizon replan).
Training-mode dropout (p = 0.1 in every ParallelAttentionLayer --
attention weights, residual branches, FFN -- and in the traj_encoder / regressor MLPs: layers.py:10,
diffusion_head.py:46,183,193) runs on a device-resident Philox stream (csrc/dropout.hip, attention kernels): same
distribution as the reference's torch generator, not the same draws.  The additive constructor keyword `dropout`
(default 0.1 = the reference) sets that probability; 0.0 disables it.
"""
import collections
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops as O
from .act3d import broadcast_row
from .nn import FeaturePyramidNetwork, ParallelAttention, load_synthetic_clip, run_frozen_backbone
# the candidates' post-processing (pins, ranking, clearance, guidance) lives in trajectory.py; every name stays importable from here
from .trajectory import (  # noqa: F401
    PINS_MAX, PIN_CHANNELS, TrajectoryPins, Pins, pin_channel_bits, check_pins, traj_pins, prefix_pins, RANK_TERMS, RANK_PRESETS,
    RANK_MAX_CANDIDATES, TrajectoryRanking, PlannerRanking, check_select, check_rot_weight, rank_trajectories, CLEARANCE_TERM,
    CLEARANCE_PRESET, TrajectoryClearance, SceneTrajectoryRanking, ScenePlannerRanking, check_scene_select, check_clearance_args,
    check_scene, prepare_scene, scan_workspace, check_trajectory_mask, trajectory_clearance, GUIDE_MAX_ROWS, GUIDE_KEYS, Guidance,
    check_guide_args, check_guide, check_guide_shape, guided_segments, guide_trajectories, _number, _pose_rows, _mask_bytes, _guide_launch,
    BODY_MAX_SPHERES, GripperBody, check_body, body_clearance)


# ------------------------------------------------------------------------------------------------ DDPM tables
class DDPMTables:
    """alphas_cumprod and per-step posterior coefficients of the two schedulers the reference builds
    (diffusion_model.py:51-60), as device tables.  Follows Ho et al. 2020 eq. 6-7 with diffusers' defaults
    (beta_start 1e-4, beta_end 0.02, variance "fixed_small", clip_sample, prediction_type "sample")."""

    def __init__(self, T, device):
        self.T = T
        betas_pos = torch.linspace(0.0001 ** 0.5, 0.02 ** 0.5, T, dtype=torch.float32) ** 2

        def alpha_bar(s):
            return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2

        betas_rot = torch.tensor([min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), 0.999) for i in range(T)],
                                 dtype=torch.float32)
        acp_pos, acp_rot = torch.cumprod(1.0 - betas_pos, 0), torch.cumprod(1.0 - betas_rot, 0)
        self.acp_pos, self.acp_rot = acp_pos.to(device), acp_rot.to(device)
        self.coef_pos, self.coef_rot = self._coef(acp_pos).to(device), self._coef(acp_rot).to(device)

    def _coef(self, acp):
        return sampler_coefficients(acp, range(self.T), 1).float().contiguous()


# ------------------------------------------------------------------------------------------------ sampler schedules
SCHEDULERS = ("ddpm", "ddim", "dpm++")


def check_sampler_args(T, num_inference_steps=None, scheduler="ddpm", eta=0.0, solver_order=2, lower_order_final=True):
    """Validates the sampler-schedule arguments of compute_trajectory on the host; returns K (None -> T).  solver_order (1 or 2) and
    lower_order_final (a bool) belong to scheduler "dpm++": any other scheduler takes only their defaults; "dpm++" takes eta = 0."""
    if scheduler not in SCHEDULERS:
        raise ValueError("unknown scheduler %r (one of %s)" % (scheduler, ", ".join(SCHEDULERS)))
    K = _number("num_inference_steps", T if num_inference_steps is None else num_inference_steps, "must be an integer in [1, %d]" % T,
                lo=1, hi=T, integer=True, shown=num_inference_steps)
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError("eta must lie in [0, 1], got %r" % (eta,))
    if scheduler == "ddpm" and float(eta) != 0.0:
        raise ValueError("eta = %r needs scheduler='ddim' (the ancestral DDPM sampler has no eta)" % (eta,))
    check_solver_args(scheduler, eta, solver_order, lower_order_final)
    return K


def check_solver_args(scheduler, eta, solver_order, lower_order_final):
    """The part of check_sampler_args that needs no chain length: what "dpm++" takes and what only "dpm++" takes."""
    if isinstance(solver_order, bool) or solver_order not in (1, 2):
        raise ValueError("solver_order must be 1 or 2, got %r" % (solver_order,))
    if not isinstance(lower_order_final, bool):
        raise ValueError("lower_order_final must be True or False, got %r" % (lower_order_final,))
    if scheduler == "dpm++":
        if float(eta) != 0.0:
            raise ValueError("eta = %r: scheduler='dpm++' is deterministic (eta must be 0)" % (eta,))
    elif solver_order != 2 or lower_order_final is not True:
        raise ValueError("solver_order / lower_order_final belong to scheduler='dpm++', got solver_order=%r, lower_order_final=%r "
                         "with scheduler=%r" % (solver_order, lower_order_final, scheduler))


def check_num_samples(num_samples):
    """Validates compute_trajectory's num_samples (candidates per scene) on the host; returns it as an int."""
    return int(_number("num_samples", num_samples, "must be an integer >= 1 (or None for one trajectory per scene)", lo=1, integer=True))


def check_candidate_noise(init_noise, step_noise, B, G, Ln, D, rows):
    """Shapes of the injected draws of a multi-candidate call: init_noise (B, G, L, D), step_noise (rows, B, G, L, D)."""
    for name, x, want in (("init_noise", init_noise, (B, G, Ln, D)), ("step_noise", step_noise, (rows, B, G, Ln, D))):
        if x is not None and tuple(x.shape) != want:
            raise ValueError("%s has shape %s; num_samples=%d needs %s (%s)" % (
                name, tuple(x.shape), G, want, "B, G, L, D" if len(want) == 4 else "steps, B, G, L, D"))


def sampler_timesteps(T, K):
    """'Leading' spacing: stride r = T // K, t_i = (K - 1 - i) r for i = 0 .. K - 1; the last one is always 0.  Returns (list, r)."""
    r = T // K
    return [(K - 1 - i) * r for i in range(K)], r


def sampler_coefficients(acp, timesteps, stride, scheduler="ddpm", eta=0.0):
    """Rows (c0, c1, c2) of the update  x_prev = c0 clip(x0, -1, 1) + c1 x_t + c2 z  at the given timesteps, in acp's dtype;
    the step from t lands on prev = t - stride with a_prev = acp[prev], or 1 when prev < 0 (c2 = 0 there: no noise at the end).
    "ddpm": the posterior of Ho et al. 2020 eq. 6-7 between t and prev, variance "fixed_small" clamped at 1e-20, in acp's own
    arithmetic (with every timestep and stride 1 these are DDPMTables.coef_*, bit for bit).
    "ddim": Song et al. 2021 eq. 12 with eps DERIVED FROM THE CLIPPED x0, eps = (x_t - sqrt(a_t) clip(x0)) / sqrt(1 - a_t) -- the
    choice that keeps the update a three-coefficient form:  sigma = eta sqrt((1 - a_prev) / (1 - a_t)) sqrt(1 - a_t / a_prev),
    c1 = sqrt(1 - a_prev - sigma^2) / sqrt(1 - a_t),  c0 = sqrt(a_prev) - c1 sqrt(a_t),  c2 = sigma; evaluated in float64.
    "dpm++": the "ddim" rows at eta = 0 by the same code (the first-order part of DPM-Solver++; the rest is sampler_kappa)."""
    rows = []
    for t in timesteps:
        prev = t - stride
        if scheduler == "ddpm":
            a_t, a_prev = acp[t], (acp[prev] if prev >= 0 else torch.ones((), dtype=acp.dtype))
            b_t, b_prev = 1 - a_t, 1 - a_prev
            cur_a = a_t / a_prev
            cur_b = 1 - cur_a
            var = torch.clamp(b_prev / b_t * cur_b, min=1e-20)
            rows.append(torch.stack([(a_prev ** 0.5 * cur_b) / b_t, cur_a ** 0.5 * b_prev / b_t,
                                     var ** 0.5 if prev >= 0 else torch.zeros((), dtype=acp.dtype)]))
        else:
            a_t = acp[t].double()
            a_prev = acp[prev].double() if prev >= 0 else torch.ones((), dtype=torch.float64)
            sigma = float(eta) * ((1 - a_prev) / (1 - a_t)) ** 0.5 * (1 - a_t / a_prev) ** 0.5
            c1 = torch.clamp(1 - a_prev - sigma ** 2, min=0.0) ** 0.5 / (1 - a_t) ** 0.5
            rows.append(torch.stack([a_prev ** 0.5 - c1 * a_t ** 0.5, c1, sigma]).to(acp.dtype))
    return torch.stack(rows)


def _log_snr_half(a):
    """lambda(a) = 1/2 ln(a / (1 - a)) = ln(alpha / sigma) of a cumulative alpha product a (a Python float, evaluated in float64)"""
    return 0.5 * math.log(a / (1.0 - a))


def sampler_kappa(acp, timesteps, stride, solver_order=2, lower_order_final=True):
    """[K] float64 coefficients of the history term of DPM-Solver++ (2M) (Lu et al. 2022, Algorithm 2) in its data-prediction form.
    With D_i = clip(in-painted network output at step position i), lambda(a) = 1/2 ln(a / (1 - a)), the step at position i from
    t = timesteps[i] to prev = t - stride and h_i = lambda(a_prev) - lambda(a_t), the multistep update
        x_prev = (sigma_prev / sigma_t) x_t - alpha_prev (e^{-h_i} - 1) [(1 + 1 / (2 rho)) D_i - 1 / (2 rho) D_{i-1}],  rho = h_{i-1} / h_i
    is the "ddim", eta = 0 row of sampler_coefficients plus one term on the previous prediction:
        x_prev = c0 D_i + c1 x_t + kappa_i (D_i - D_{i-1}),    kappa_i = sqrt(a_prev) (1 - e^{-h_i}) h_i / (2 h_{i-1}).
    kappa_i = 0 (a first-order step) at position 0 (no history yet), everywhere for solver_order 1, at the terminal position (prev < 0:
    the step returns the network output) and, with lower_order_final, at the last update, position K - 2: it lands on timestep 0,
    where h is several times the steps before it and the extrapolation overshoots (kappa up to 1.6; diffusers' lower_order_final)."""
    K = len(timesteps)
    lam = lambda t: _log_snr_half(float(acp[t].double()))
    out = torch.zeros(K, dtype=torch.float64)
    if solver_order == 1:
        return out
    for i in range(1, K):
        t, prev = timesteps[i], timesteps[i] - stride
        if prev < 0 or (lower_order_final and i == K - 2):
            continue
        h, h_last = lam(prev) - lam(t), lam(t) - lam(timesteps[i - 1])
        out[i] = math.sqrt(float(acp[prev].double())) * (1.0 - math.exp(-h)) * h / (2.0 * h_last)
    return out


class SamplerSchedule:
    """A K-step sampler over the T training timesteps of a DDPMTables (its position and rotation schedules): the timestep list and
    the per-step coefficient tables coef_pos / coef_rot [K][3], indexed by step POSITION i (the i-th executed step), see
    sampler_timesteps / sampler_coefficients.  The step at timestep 0 (position K - 1) is terminal for both schedulers: it returns
    the in-painted network output and adds no noise, as the full chain does.  noise_free: no step reads a noise draw (DDIM, eta = 0,
    and "dpm++").  "dpm++" (DPM-Solver++ 2M): coef_* are the "ddim", eta = 0 rows, bit for bit, and kappa_pos / kappa_rot [K] weigh
    the history term (sampler_kappa); they are None for the other schedulers, whose key is unchanged."""

    def __init__(self, tables, num_inference_steps=None, scheduler="ddpm", eta=0.0, solver_order=2, lower_order_final=True):
        self.T = tables.T
        self.K = check_sampler_args(tables.T, num_inference_steps, scheduler, eta, solver_order, lower_order_final)
        self.scheduler, self.eta = scheduler, float(eta)
        self.solver_order, self.lower_order_final = solver_order, lower_order_final
        self.timesteps, self.stride = sampler_timesteps(self.T, self.K)
        dev = tables.acp_pos.device
        self.coef_pos, self.coef_rot = (
            sampler_coefficients(acp.cpu(), self.timesteps, self.stride, scheduler, eta).float().contiguous().to(dev)
            for acp in (tables.acp_pos, tables.acp_rot))
        self.noise_free = scheduler in ("ddim", "dpm++") and self.eta == 0.0
        self.key = (self.K, scheduler, self.eta)
        self.kappa_pos = self.kappa_rot = None
        if scheduler == "dpm++":
            self.kappa_pos, self.kappa_rot = (
                sampler_kappa(acp.cpu(), self.timesteps, self.stride, solver_order, lower_order_final).float().contiguous().to(dev)
                for acp in (tables.acp_pos, tables.acp_rot))
            self.key = self.key + (solver_order, lower_order_final)


# ------------------------------------------------------------------------------------------------ pose <-> signal
def pose_to_signal(pose, bounds=None):
    """[xyz | quaternion (w, x, y, z) | extra] -> [normalised xyz | 6D rotation | extra] in one launch
    (diffusion_model.py:187-212; csrc/diffusion.hip).  bounds: (2, 3) device tensor or None (xyz untouched).  No grad."""
    x = O._c(pose.detach().float())
    n, D = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty(x.shape[:-1] + (D + 2,), device=x.device, dtype=torch.float32)
    O.L.call("a3d_pose_to_signal", x.data_ptr(), None if bounds is None else bounds.data_ptr(), out.data_ptr(), n, D - 7,
             O.L.stream())
    return out


def signal_to_pose(signal, bounds=None):
    """inverse map (diffusion_model.py:192-195,214-230)"""
    x = O._c(signal.detach().float())
    n, D = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty(x.shape[:-1] + (D - 2,), device=x.device, dtype=torch.float32)
    O.L.call("a3d_signal_to_pose", x.data_ptr(), None if bounds is None else bounds.data_ptr(), out.data_ptr(), n, D - 9,
             O.L.stream())
    return out


def traj_condition(curr_gripper, goal_gripper, bounds, trajectory_mask, init_noise=None, num_samples=1, use_goal=True):
    """The conditioning of a sampling call in ONE launch (a3d_traj_condition, csrc/diffusion.hip; diffusion_model.py:131-168):
    returns (cg, gg, cond_data, cond_mask_u8, kmask, traj) -- the two poses as signals (B, D) (bit-equal to pose_to_signal), the
    in-painting data / mask (B G, L, D) and the key mask (B G, L) of G = num_samples trajectories per scene (scene-major), and
    traj = init_noise + cond_data when init_noise (B G, L, D) is given (None otherwise).  curr_gripper / goal_gripper: (B, Dp)
    rows, read in place where they are row slices of a wider tensor; trajectory_mask: (B, L), non-zero = padded step."""
    cur, ldc = _pose_rows(curr_gripper, "curr_gripper")
    goal, ldg = _pose_rows(goal_gripper, "goal_gripper")
    B, Dp = cur.shape
    G = int(num_samples)
    if tuple(goal.shape) != (B, Dp):
        raise ValueError("goal_gripper has shape %s, curr_gripper %s" % (tuple(goal.shape), (B, Dp)))
    check_trajectory_mask(trajectory_mask, B)
    Ln, D = trajectory_mask.shape[1], Dp + 2
    if init_noise is not None and tuple(init_noise.shape) != (B * G, Ln, D):
        raise ValueError("init_noise has shape %s, the call needs %s" % (tuple(init_noise.shape), (B * G, Ln, D)))
    O.L.require_gpu(cur, goal, bounds, trajectory_mask, init_noise)
    tm = _mask_bytes(trajectory_mask)
    dev = cur.device
    noise = None if init_noise is None else O._c(init_noise.detach().float())
    cg = torch.empty((B, D), device=dev, dtype=torch.float32)
    gg = torch.empty((B, D), device=dev, dtype=torch.float32)
    cond_data = torch.empty((B * G, Ln, D), device=dev, dtype=torch.float32)
    cond_mask = torch.empty((B * G, Ln, D), device=dev, dtype=torch.uint8)
    kmask = torch.empty((B * G, Ln), device=dev, dtype=torch.uint8)
    traj = None if noise is None else torch.empty((B * G, Ln, D), device=dev, dtype=torch.float32)
    O.L.call("a3d_traj_condition", cur.data_ptr(), ldc, goal.data_ptr(), ldg, O._c(bounds).data_ptr(), tm.data_ptr(),
             None if noise is None else noise.data_ptr(), cg.data_ptr(), gg.data_ptr(), cond_data.data_ptr(), cond_mask.data_ptr(),
             kmask.data_ptr(), None if traj is None else traj.data_ptr(), B, G, Ln, Dp, 1 if use_goal else 0, O.L.stream())
    return cg, gg, cond_data, cond_mask, kmask, traj


# ------------------------------------------------------------------------------------------------ prediction head
class DiffusionHead(nn.Module):

    def __init__(self, backbone="clip", image_size=(256, 256), embedding_dim=60, output_dim=7, num_attn_heads=8,
                 num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6, use_instruction=False, use_goal=False,
                 use_sigma=False, feat_scales_to_use=1, attn_rounds=1, weight_tying=False,
                 rotation_parametrization='quat', dropout=0.1, dropout_seed=0):
        super().__init__()
        if use_sigma:
            # DiffusionPlanner never forwards use_sigma (diffusion_model.py:37-50): unreachable through the model API
            raise NotImplementedError("use_sigma=True (a learned time embedding, encoder.py:68-76) is not implemented")
        assert feat_scales_to_use in (1, 2, 3, 4) and attn_rounds >= 1
        self.attn_rounds, self.feat_scales = attn_rounds, feat_scales_to_use
        R = attn_rounds * feat_scales_to_use        # one module set per (round, scale) iteration, diffusion_head.py:53-199
        self.image_size = tuple(image_size)
        self.use_instruction, self.use_goal = use_instruction, use_goal
        self.rotation_parametrization = rotation_parametrization
        self.num_attn_heads = num_attn_heads
        self.dropout_p = dropout
        if rotation_parametrization == '6D':
            output_dim += 2
        E = embedding_dim
        # --- Encoder base (model/utils/encoder.py:14-73)
        self.backbone, self.normalize = load_synthetic_clip()
        for p in self.backbone.parameters():
            p.requires_grad = False
        self.backbone_dtype = torch.float32
        self.fpn_dtype = torch.float32           # set to torch.bfloat16 to run the FPN convolutions under autocast (as Act3D.fpn_dtype)
        self.feature_pyramid = FeaturePyramidNetwork([64, 256, 512, 1024, 2048], E)
        self.feature_map_pyramid = ['res3', 'res1', 'res1', 'res1'] if self.image_size == (256, 256) else ['res2', 'res1', 'res1', 'res1']
        self.downscaling_factor_pyramid = [8, 2, 2, 2] if self.image_size == (256, 256) else [4, 2, 2, 2]
        self.curr_gripper_embed = nn.Embedding(1, E)
        self.goal_gripper_embed = nn.Embedding(1, E)
        self.instruction_encoder = nn.Linear(512, E)
        # --- DiffusionHead (diffusion_head.py:41-199)
        self.traj_encoder = nn.Sequential(nn.Linear(9, E), nn.ReLU(), nn.Dropout(dropout), nn.Linear(E, E))
        self.curr_gripper_encoder = nn.Linear(output_dim, E)
        if use_goal:
            self.goal_gripper_encoder = nn.Linear(output_dim, E)
        common = dict(d_model=E, n_heads=num_attn_heads, dropout=dropout, self_attention2=False, cross_attention1=True,
                      cross_attention2=False)
        def stack(make):                      # the reference shares ONE module across all iterations iff weight_tying
            if weight_tying:
                m = make()
                return nn.ModuleList([m for _ in range(R)])
            return nn.ModuleList([make() for _ in range(R)])

        if use_instruction:
            self.vl_attention = stack(lambda: ParallelAttention(num_layers=num_vis_ins_attn_layers, self_attention1=False, **common))
        self.traj_lang_attention = stack(lambda: ParallelAttention(num_layers=1, self_attention1=False, rotary_pe=False,
                                                                   apply_ffn=False, **common))
        self.traj_attention = stack(lambda: ParallelAttention(num_layers=num_query_cross_attn_layers - 2, self_attention1=True,
                                                              rotary_pe=True, use_adaln=True, **common))
        self.pos_attention = stack(lambda: ParallelAttention(num_layers=2, self_attention1=True, rotary_pe=True,
                                                             use_adaln=True, **common))
        self.rot_attention = stack(lambda: ParallelAttention(num_layers=2, self_attention1=True, rotary_pe=True,
                                                             use_adaln=True, **common))
        self.pos_regressor = nn.ModuleList([nn.Sequential(nn.Linear(E, E), nn.ReLU(), nn.Dropout(dropout), nn.Linear(E, 3))
                                            for _ in range(R)])
        self.rot_regressor = nn.ModuleList([nn.Sequential(nn.Linear(E, E), nn.ReLU(), nn.Dropout(dropout),
                                                          nn.Linear(E, output_dim - 3)) for _ in range(R)])
        self._sem_cache = {}
        # dropout sites are named after the modules (ops.site_id); generator state {seed, forward-pass counter} on the device
        for name, mod in self.named_modules():
            if hasattr(mod, "site_base"):
                mod.site_base = O.site_id(name)
        self._mlp_sites = {n: O.site_id(n, 4) for n in ["traj_encoder"] + [f"{k}_regressor.{l}" for k in ("pos", "rot")
                                                                          for l in range(R)]}
        self.register_buffer("_drop_state", torch.tensor([dropout_seed, 0], dtype=torch.int64), persistent=False)

    def begin_dropout(self):
        """DropCtx of one training forward pass (None in eval mode or with dropout=0): snapshots the device generator
        state and advances it by one, both as stream-ordered kernels (capturable)."""
        if not self.training or self.dropout_p <= 0:
            return None
        snap = self._drop_state.clone()
        O.L.call("a3d_rng_advance", self._drop_state.data_ptr(), 1, O.L.stream())
        return O.DropCtx(snap, self.dropout_p)

    # ---- vision (adjacent): one scale
    def encode_images(self, rgb, pcd_norm, maps=None):
        """encoder.py:115-167: FPN tokens (B, ncam*h*w, E) of the scales the head uses -- one tensor for
        feat_scales_to_use = 1 (the res3 map at 1/8), a list [res3 @ 1/8, res1 @ 1/2, ...] otherwise."""
        B, ncam = rgb.shape[:2]
        return self.tokens_from_backbone_maps(maps if maps is not None else self.backbone_maps(rgb), B, ncam)

    def backbone_maps(self, rgb, out=None):
        """The frozen half of encode_images (normalize -> backbone under no_grad): {res1..res5} of the B * ncam views; `out`:
        preallocated maps to write into.  No gradient flows through it and its weights never change, so a training loop may compute
        the maps of batch k + 1 while step k runs (engine.GraphedStep(prefetch=...)) and pass them to encode_images(maps=...)."""
        x = rgb.flatten(0, 1)
        low = self.fpn_dtype != torch.float32 and x.is_cuda
        with torch.no_grad():
            return run_frozen_backbone(self.backbone, x, self.backbone_dtype, keep_dtype=low, normalize=self.normalize, out=out)

    def tokens_from_backbone_maps(self, feats, B, ncam):
        """The FPN + token layout half of encode_images on the backbone's maps {res1..res5} of the B * ncam views (bf16 maps when
        fpn_dtype is bf16, fp32 maps otherwise)."""
        low = self.fpn_dtype != torch.float32 and next(iter(feats.values())).is_cuda
        names = self.feature_map_pyramid[:self.feat_scales]
        E_ = self.curr_gripper_embed.weight.shape[1]
        if low:
            # round 6: the FPN in bf16 on the backbone's bf16 maps (channels padded to a multiple of 64 for MIOpen, the lateral biases
            # folded into the top-down kernel) -- the fp32 path converted all five backbone maps to fp32 (277 MB for res1 alone at the
            # script shape) and ran the FPN's convolutions, forward and backward, on MIOpen's fp32 kernels; only the map(s) the head
            # reads are converted now
            with torch.autocast("cuda", dtype=self.fpn_dtype):
                pyr = self.feature_pyramid(feats, needed=sorted(set(names)), pad_to=(E_ + 63) // 64 * 64)
        else:
            pyr = self.feature_pyramid(feats, needed=sorted(set(names)))
        toks = {}
        for name in set(names):
            fm = pyr[name]
            n, E, h, w = fm.shape
            tk = fm.permute(0, 2, 3, 1).reshape(B, ncam * h * w, E)
            toks[name] = tk[..., :E_].float() if low else tk
        out = [toks[n] for n in names]
        return out[0] if self.feat_scales == 1 else out

    def _sem(self, Ln, E, device):
        key = (Ln, E, str(device))
        if key not in self._sem_cache:
            self._sem_cache[key] = O.sinusoidal_emb(torch.arange(Ln, device=device, dtype=torch.float32), E)
        return self._sem_cache[key]

    def _gripper_tokens(self, curr_gripper, goal_gripper):
        """The gripper tokens every context ends with: (rows (B, 1 | 2, E), the list of their xyz rows (B, 1, 3) each) -- the
        current gripper and, with use_goal, the goal."""
        B = curr_gripper.shape[0]
        cg = O.linear(curr_gripper, self.curr_gripper_encoder)[:, None] + broadcast_row(self.curr_gripper_embed.weight, B, 1)
        extra, extra_xyz = [cg], [curr_gripper[:, None, :3]]
        if self.use_goal:
            gg = O.linear(goal_gripper, self.goal_gripper_encoder)[:, None] + broadcast_row(self.goal_gripper_embed.weight, B, 1)
            extra.append(gg)
            extra_xyz.append(goal_gripper[:, None, :3])
        return torch.cat(extra, dim=1), extra_xyz

    def encode_context(self, visual_tokens, ctx_xyz, instruction, curr_gripper, goal_gripper, drop=None):
        """Step-invariant context (diffusion_head.py:222-247, 290-323): returns (ctx (B,S,E), ctx_xyz (B,S,3), instr)."""
        instr = O.linear(instruction.float(), self.instruction_encoder) if self.use_instruction else None
        ctx = visual_tokens
        if self.use_instruction:
            ctx = self.vl_attention[0](ctx, None, instr, drop=drop)
        extra, extra_xyz = self._gripper_tokens(curr_gripper, goal_gripper)
        ctx = O.BuildContextFn.apply(ctx, None, extra)
        ctx_xyz = torch.cat([ctx_xyz] + extra_xyz, dim=1).contiguous()
        return ctx, ctx_xyz, instr

    def _iteration(self, l, prev, trajectory_mask, traj_feats, traj_xyz, sem, silu_t, ctx, ctx_xyz, instr, drop=None, sinks=None,
                   cache=None):
        """Iteration l of the head (diffusion_head.py:325-363) on module set l: the optional language layer, the trajectory,
        position and rotation stacks, the two regressors; returns `prev` updated by the prediction (xyz accumulates, the rotation
        is replaced).  traj_feats / traj_xyz / sem / silu_t: the trajectory encoding, its positions, the step embedding rows and
        SiLU(time embedding), all the caller's.  What differs between the callers comes in:
          drop   the DropCtx of this iteration (None: no dropout);
          sinks  the registry of the context's shared gradient sink (ops.GradSink: the k | v projections' input and weight
                 gradients of all 8 cross-attention layers run as ONE GEMM each when the last layer's backward has parked its
                 rows), attached after the language layer; None: no sink -- it would change the summation order of the gradients;
          cache  build_kv_cache's K/V operands: every cross-attention block reads them, ctx / ctx_xyz / instr are unused."""
        ms = self._mlp_sites
        stacks = (self.traj_attention[l], self.pos_attention[l], self.rot_attention[l])
        lang_c, stack_c = None, (None, None, None)
        if cache is not None:
            per_layer = iter(cache["ctx"])                  # in _cross_layers order
            lang_c, stack_c = [cache.get("lang")], [[next(per_layer) for _ in st.layers] for st in stacks]
        if self.use_instruction:
            traj_feats = self.traj_lang_attention[l](traj_feats, trajectory_mask, instr, seq1_sem_pos=sem, drop=drop,
                                                     cross_caches=lang_c)
        if sinks is not None:
            ctx = O.attach_grad_sink(ctx, sinks)
        kw = dict(seq1_xyz=traj_xyz, seq2_xyz=ctx_xyz, seq1_sem_pos=sem, silu_t=silu_t, drop=drop)
        traj_feats = stacks[0](traj_feats, trajectory_mask, ctx, cross_caches=stack_c[0], **kw)
        pos_feats = stacks[1](traj_feats, trajectory_mask, ctx, cross_caches=stack_c[1], **kw)
        rot_feats = stacks[2](traj_feats, trajectory_mask, ctx, cross_caches=stack_c[2], **kw)
        upd = torch.cat([O.mlp(pos_feats, self.pos_regressor[l][0], self.pos_regressor[l][3], drop=drop,
                               site_hidden=ms[f"pos_regressor.{l}"]),
                         O.mlp(rot_feats, self.rot_regressor[l][0], self.rot_regressor[l][3], drop=drop,
                               site_hidden=ms[f"rot_regressor.{l}"])], dim=-1)
        return O.TrajUpdateFn.apply(prev, upd)

    def forward_tokens(self, trajectory, trajectory_mask, timestep, ctx, ctx_xyz, instr, drop=None):
        """The step-dependent part of DiffusionHead.forward (diffusion_head.py:214-219, 325-363) with autograd."""
        B, Ln, _ = trajectory.shape
        E = ctx.shape[-1]
        trajectory = trajectory.contiguous()
        traj_feats = O.mlp(trajectory, self.traj_encoder[0], self.traj_encoder[3], drop=drop,
                           site_hidden=self._mlp_sites["traj_encoder"])
        traj_xyz = trajectory[..., :3].contiguous()
        time_feats = O.sinusoidal_emb(timestep.float(), E)
        silu_t = O.SiLUFn.apply(time_feats)
        sem = self._sem(Ln, E, trajectory.device)
        self._ctx_sinks = []
        return self._iteration(0, trajectory, trajectory_mask, traj_feats, traj_xyz, sem, silu_t, ctx, ctx_xyz, instr, drop=drop,
                               sinks=self._ctx_sinks)

    def forward_multi(self, trajectory, trajectory_mask, timestep, tokens, xyzs, instruction, curr_gripper, goal_gripper,
                      new_drop=None):
        """DiffusionHead.forward for attn_rounds x feat_scales_to_use > 1 (diffusion_head.py:249-275).  Iteration
        l = round * feat_scales + scale runs module set l on the SAME trajectory encoding / positions (the reference never
        carries traj_feats over, :286-288); only the prediction chains (xyz accumulates, rotation is replaced).  With a goal,
        scales > 0 attend to the (64 | 16) * L fine tokens nearest to the previous prediction (find_traj_nn ->
        a3d_traj_nn_topk).  tokens / xyzs: per-scale visual tokens (B, N_s, E) and normalised coordinates (B, N_s, 3).
        new_drop: callable returning a fresh DropCtx per iteration (None: no dropout).  Returns the list of predictions."""
        B, Ln, _ = trajectory.shape
        E = self.curr_gripper_embed.weight.shape[1]
        trajectory = trajectory.contiguous()
        drop = new_drop() if new_drop is not None else None
        traj_feats0 = O.mlp(trajectory, self.traj_encoder[0], self.traj_encoder[3], drop=drop,
                            site_hidden=self._mlp_sites["traj_encoder"])
        traj_xyz = trajectory[..., :3].contiguous()
        silu_t = O.SiLUFn.apply(O.sinusoidal_emb(timestep.float(), E))
        sem = self._sem(Ln, E, trajectory.device)
        instr = O.linear(instruction.float(), self.instruction_encoder) if self.use_instruction else None
        extra, extra_xyz = self._gripper_tokens(curr_gripper, goal_gripper)
        extra_xyz = torch.cat(extra_xyz, dim=1).contiguous()
        none = torch.empty((B, 0, E), device=trajectory.device, dtype=torch.float32)
        outs, prev = [], trajectory
        for rnd in range(self.attn_rounds):
            for scale in range(self.feat_scales):
                l = rnd * self.feat_scales + scale
                if l > 0 and new_drop is not None:
                    drop = new_drop()
                feats, xyz = tokens[scale], xyzs[scale]
                idx = None
                if self.use_goal and scale > 0:
                    idx = O.traj_nn_topk(outs[-1][..., :3], xyz, (64 if scale == 1 else 16) * Ln)
                if self.use_instruction:
                    ctx = O.BuildContextFn.apply(feats, idx, none) if idx is not None else feats
                    ctx = self.vl_attention[l](ctx, None, instr, drop=drop)
                    ctx = O.BuildContextFn.apply(ctx, None, extra)
                else:
                    ctx = O.BuildContextFn.apply(feats, idx, extra)
                ctx_xyz = O.gather_rows(xyz, idx, extra_xyz)
                prev = self._iteration(l, prev, trajectory_mask, traj_feats0, traj_xyz, sem, silu_t, ctx, ctx_xyz, instr, drop=drop)
                outs.append(prev)
        return outs

    # ---- inference with cached K/V
    def _cross_layers(self):
        out = []
        for stack in (self.traj_attention[0], self.pos_attention[0], self.rot_attention[0]):
            out.extend(stack.layers)
        return out

    @torch.no_grad()
    def build_kv_cache(self, ctx, ctx_xyz, instr):
        cache = {"ctx": [O.kv_cache_build(ctx, ctx_xyz, lay.cross_12, self.num_attn_heads) for lay in self._cross_layers()]}
        if self.use_instruction:
            cache["lang"] = O.kv_cache_build(instr, None, self.traj_lang_attention[0].layers[0].cross_12, self.num_attn_heads)
        return cache

    @torch.no_grad()
    def denoise_tokens_cached(self, trajectory, trajectory_mask, t, cache, time_tables):
        """One network evaluation at integer step t against the prebuilt K/V cache (no autograd, no host sync): iteration 0 of the
        head with SiLU(time embedding) read from the time table."""
        B, Ln, _ = trajectory.shape
        E = self.curr_gripper_embed.weight.shape[1]
        traj_feats = O.mlp(trajectory, self.traj_encoder[0], self.traj_encoder[3])
        traj_xyz = trajectory[..., :3].contiguous()
        silu_t = time_tables["silu"][t:t + 1].expand(B, E).contiguous()
        sem = self._sem(Ln, E, trajectory.device)
        return self._iteration(0, trajectory, trajectory_mask, traj_feats, traj_xyz, sem, silu_t, None, None, None, cache=cache)

    # ---- inference, fused: 18 launches per network evaluation (csrc/denoise.hip)
    @torch.no_grad()
    def build_fused(self, ctx, ctx_xyz, instr, kmask, time_sin, Ln, n_cand=1):
        """Step-invariant state of the fused sampling path for one trajectory batch: the context K (fp16 hi | lo rows) / V (fp16
        hi / lo planes) of every cross-attention layer, the instruction tokens through traj_lang_attention's k | v projection, and
        the AdaLN modulation of every layer at every row of time_sin (Linear(SiLU(sinusoidal(t))), layers.py:273-290): all T timesteps
        for the full chain, only the K scheduled ones -- in step order -- under a SamplerSchedule.  Returns
        {"tensors": [...]} -- the list is what a captured graph must refresh in place -- plus per-layer pointer tables.
        n_cand > 1 (compute_trajectory(num_samples=...)): ctx / ctx_xyz / instr hold one sample per SCENE and every cache tensor keeps
        that leading dimension B; kmask and the persistent sampler's workspaces are per trajectory, B * n_cand of them
        (a3d_dn_persist_group); the per-phase workspaces (ws) are not for such a state."""
        B, S, E = ctx.shape
        H = self.num_attn_heads
        dev = ctx.device
        Sp = O.ceil_to(S, 64)
        freq = O.rope_freq(E, dev)
        silu = F.silu(time_sin)                                         # (T, E)
        st = {"S": S, "Sp": Sp, "layers": [], "tensors": [], "freq": freq, "sem": self._sem(Ln, E, dev), "kmask": kmask, "n_cand": n_cand}
        ctx = O._c(ctx)
        xyz = O._c(ctx_xyz.float())
        for lay in self._cross_layers():
            # the split-fp16 operand formats (csrc/denoise.hip header): K rows16, V planes16 with the ones channel, in ONE launch per
            # layer (E % 4 != 0 -- E = 30 / 90 -- which the fused writer's float4 reads refuse: one linear launch, two formatting ones)
            Kf, Vt = O.ctx_kv_cache16(ctx, xyz, lay.cross_12, H)
            mods = [O.linear2d(silu, a.modulation[1].weight, a.modulation[1].bias) for a in (lay.adaln_12, lay.adaln_1, lay.adaln_ff1)]
            st["layers"].append({"lay": lay, "Kf": Kf, "Vt": Vt, "mods": mods})
            st["tensors"] += [Kf, Vt] + mods
        st["lang_kv"] = None
        if self.use_instruction:
            mha = self.traj_lang_attention[0].layers[0].cross_12
            ip = O.InProj(mha.in_proj_weight, mha.in_proj_bias, E)
            instr = O._c(instr)
            st["S_lang"] = instr.shape[1]
            st["lang_kv"] = O.linear_raw(instr.data_ptr(), E, ip.wk, E, ip.bk, B * instr.shape[1], 2 * E, E, dev)
            st["tensors"].append(st["lang_kv"])
        st["nsplit"] = max(1, min(8, Sp // 128, -(-DN_TARGET_WGS // (B * H))))
        nws = O.L.load().a3d_dn_cross_ws_floats(B, H, st["nsplit"])
        st["ws"] = torch.empty((nws,), device=dev, dtype=torch.float32)
        st["ws_side"] = torch.empty((nws,), device=dev, dtype=torch.float32)      # rotation branch, concurrent
        st["persist"] = None                                # the persistent sampler's own state: _build_persist, for the calls planned on it
        return st

    # ---- the parameter blocks of the fused kernels (lib.Dn*Params), each built in ONE place
    def _dn_head_params(self, st):
        enc = self.traj_encoder
        hp = O.L.DnHeadParams(enc_w0=enc[0].weight.data_ptr(), enc_b0=enc[0].bias.data_ptr(), enc_w1=enc[3].weight.data_ptr(),
                              enc_b1=enc[3].bias.data_ptr(), sem=st["sem"].data_ptr(),
                              lang_kv=None if st["lang_kv"] is None else st["lang_kv"].data_ptr(), S_lang=st.get("S_lang", 0))
        if st["lang_kv"] is not None:
            ll = self.traj_lang_attention[0].layers[0]
            hp.q_w, hp.q_b = ll.cross_12.in_proj_weight.data_ptr(), ll.cross_12.in_proj_bias.data_ptr()
            hp.out_w, hp.out_b = ll.cross_12.out_proj.weight.data_ptr(), ll.cross_12.out_proj.bias.data_ptr()
            hp.ln_g, hp.ln_b = ll.norm_12.weight.data_ptr(), ll.norm_12.bias.data_ptr()
        return hp

    def _dn_tail_params(self, noise, cond_data, cond_mask_u8, tables, hist=None):
        """noise: what the launch reads -- the whole table (persistent sampler), one step's row (per-phase tail) or None.
        hist: the history buffer of a multistep schedule (tables.kappa_*), else None: the three fields stay NULL."""
        pr, rr = self.pos_regressor[0], self.rot_regressor[0]
        tp = O.L.DnTailParams(pos_w0=pr[0].weight.data_ptr(), pos_b0=pr[0].bias.data_ptr(), pos_w1=pr[3].weight.data_ptr(),
                              pos_b1=pr[3].bias.data_ptr(), rot_w0=rr[0].weight.data_ptr(), rot_b0=rr[0].bias.data_ptr(),
                              rot_w1=rr[3].weight.data_ptr(), rot_b1=rr[3].bias.data_ptr(),
                              noise=None if noise is None else noise.data_ptr(), cond_data=cond_data.data_ptr(),
                              cond_mask=cond_mask_u8.data_ptr(), coef_pos=tables.coef_pos.data_ptr(),
                              coef_rot=tables.coef_rot.data_ptr())
        if hist is not None:
            assert tuple(hist.shape) == tuple(cond_data.shape) and hist.is_contiguous() and hist.dtype == torch.float32
            tp.hist, tp.kappa_pos, tp.kappa_rot = hist.data_ptr(), tables.kappa_pos.data_ptr(), tables.kappa_rot.data_ptr()
        return tp

    @staticmethod
    def _dn_mod(rec, k, row):
        """AdaLN table k ([rows][2E] fp32) of a layer: its base for row=None (the persistent sampler indexes it with the step), else
        the pointer to `row`."""
        m = rec["mods"][k]
        return m.data_ptr() + (0 if row is None else row * m.stride(0) * m.element_size())

    def _dn_cross_params(self, st, rec, row=None):
        mha = rec["lay"].cross_12
        return O.L.DnCrossParams(sem=st["sem"].data_ptr(), mod=self._dn_mod(rec, 0, row), q_w=mha.in_proj_weight.data_ptr(),
                                 q_b=mha.in_proj_bias.data_ptr(), freq=st["freq"].data_ptr(), Kf=rec["Kf"].data_ptr(),
                                 Vt=rec["Vt"].data_ptr())

    def _dn_rest_params(self, st, rec, row=None):
        lay, ff = rec["lay"], rec["lay"].ffn_12
        return O.L.DnRestParams(
            c_out_w=lay.cross_12.out_proj.weight.data_ptr(), c_out_b=lay.cross_12.out_proj.bias.data_ptr(),
            c_ln_g=lay.norm_12.weight.data_ptr(), c_ln_b=lay.norm_12.bias.data_ptr(), sem=st["sem"].data_ptr(),
            s_mod=self._dn_mod(rec, 1, row), s_in_w=lay.sa1.in_proj_weight.data_ptr(), s_in_b=lay.sa1.in_proj_bias.data_ptr(),
            s_out_w=lay.sa1.out_proj.weight.data_ptr(), s_out_b=lay.sa1.out_proj.bias.data_ptr(),
            s_ln_g=lay.norm_1.weight.data_ptr(), s_ln_b=lay.norm_1.bias.data_ptr(), freq=st["freq"].data_ptr(),
            kmask=None if st["kmask"] is None else st["kmask"].data_ptr(), f_mod=self._dn_mod(rec, 2, row),
            f_w1=ff[0].weight.data_ptr(), f_b1=ff[0].bias.data_ptr(), f_w2=ff[3].weight.data_ptr(), f_b2=ff[3].bias.data_ptr(),
            f_ln_g=lay.norm_122.weight.data_ptr(), f_ln_b=lay.norm_122.bias.data_ptr(), F=ff[0].weight.shape[0])

    def _build_persist(self, st, B, Ln, T, group=False):
        """State of the persistent sampler (a3d_dn_persist: the whole denoise loop as one launch, csrc/denoise.hip): the device
        table of per-layer parameter blocks (AdaLN tables by their base: the kernel indexes them with the step), the query /
        partial exchange buffers and the synchronisation words.  Whether the launch fits the device is sampler_plan's question
        (persist_fits), answered before this state is built.
        B: TRAJECTORIES (scenes x st["n_cand"] candidates: the workspaces are per trajectory, the K / V tables of st per scene).
        T: rows of the AdaLN tables -- the training timesteps, or the K steps of a sampler schedule (a3d_dn_persist_sched).
        group: the launches go through a3d_dn_persist_group (compute_trajectory(num_samples=...))."""
        Lb = O.L
        lib = Lb.load()
        H, E, Sp, dev = self.num_attn_heads, st["sem"].shape[-1], st["Sp"], st["sem"].device
        NT = -(-Ln // 16)                                   # 16-step row tiles per trajectory: one sample-role workgroup each
        recs = st["layers"]
        table = (Lb.DnLayerParams * len(recs))()
        for i, rec in enumerate(recs):
            table[i].cross, table[i].rest = self._dn_cross_params(st, rec), self._dn_rest_params(st, rec)
        raw = bytes(memoryview(table))
        nsplit = max(1, min(DN_PERSIST_SPLIT, Sp // 64, 16 // lib.a3d_dn_persist_splits(H, 1)))      # at most 16 partials per (sample, head)
        nse = lib.a3d_dn_persist_splits(H, nsplit)
        n_layers = len(recs)
        return {
            "table": torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev),
            "nsplit": nsplit,
            "qbuf": torch.zeros((2 * B * NT * 16 * 128,), device=dev, dtype=torch.float32),
            "part": torch.empty((lib.a3d_dn_cross_ws_floats(2 * B * NT, H, nse),), device=dev, dtype=torch.float32),
            "xbuf": torch.zeros((lib.a3d_dn_persist_xbuf_floats(B, Ln),), device=dev, dtype=torch.float32),
            "kvx": torch.empty((lib.a3d_dn_persist_kvx_floats(B, Ln, E),), device=dev, dtype=torch.float32) if NT > 1 else None,
            "sync": torch.zeros((lib.a3d_dn_persist_sync_ints(B, Ln, n_layers, T),), device=dev, dtype=torch.int32),
            "stacks": (len(self.traj_attention[0].layers), len(self.pos_attention[0].layers), len(self.rot_attention[0].layers)),
            "rows": T,                                          # rows of the AdaLN tables = the most steps one launch may run
            "n_cand": st.get("n_cand", 1),                      # candidates per scene of a num_samples call
            "group": group,
        }

    @torch.no_grad()
    def fused_persist(self, st, traj, first, nsteps, step_noise, cond_data, cond_mask_u8, tables):
        """nsteps consecutive denoise steps (network evaluation + DDPM reverse step each) as ONE launch of the persistent sampler;
        returns the trajectory after the last of them (a new tensor).  tables is what st was built on:
        a DDPMTables -- the timesteps first, first - 1, ... of the full chain (a3d_dn_persist), step_noise the (T, B, L, D) table;
        a SamplerSchedule -- the steps at POSITIONS first, first + 1, ... of the schedule (a3d_dn_persist_sched), step_noise
        (K, B, L, D) by position, or None for a noise-free schedule.  st["hist"] (a "dpm++" schedule): the history buffer (B, L, D) the
        launch starts from and leaves its last prediction in.
        A state marked for candidate groups (ps["group"]: compute_trajectory(num_samples=G), always on a schedule) goes through
        a3d_dn_persist_group: traj holds scenes x n_cand trajectories, scene-major, against the per-scene cache of st."""
        Lb = O.L
        ps = st["persist"]
        B, Ln, D = traj.shape
        hp, tp = self._dn_head_params(st), self._dn_tail_params(step_noise, cond_data, cond_mask_u8, tables, st.get("hist"))
        out = traj.clone()
        self._last_persist = ps                      # tests read the abort word (sync[2]) after synchronising
        nt, npos, nrot = ps["stacks"]
        common = (ps["table"].data_ptr(), nt, npos, nrot, Lb.byref(hp), Lb.byref(tp), out.data_ptr(), ps["qbuf"].data_ptr(),
                  ps["part"].data_ptr(), None if ps["kvx"] is None else ps["kvx"].data_ptr(), ps["xbuf"].data_ptr(), ps["sync"].data_ptr(),
                  B, Ln, D, st["sem"].shape[-1], self.num_attn_heads, st["S"], st["Sp"], ps["nsplit"], int(first), int(nsteps))
        if not isinstance(tables, SamplerSchedule):
            entry = "a3d_dn_persist"
            assert not ps["group"]
            Lb.call(entry, *common, Lb.stream())
        else:
            K = tables.K
            assert ps["rows"] == K and (step_noise is None) == tables.noise_free
            if ps["group"]:
                entry = "a3d_dn_persist_group"
                assert B % ps["n_cand"] == 0 and st["layers"][0]["Kf"].shape[0] * ps["n_cand"] == B
                Lb.call(entry, *common, K, int(first + nsteps == K), ps["n_cand"], Lb.stream())
            else:
                entry = "a3d_dn_persist_sched"
                Lb.call(entry, *common, K, int(first + nsteps == K), Lb.stream())
        if DN_PERSIST_CHECK:
            if int(ps["sync"][2].item()) != 0:
                raise RuntimeError(entry + " gave up waiting (sync[2] != 0): the trajectory is invalid")
        return out

    @torch.no_grad()
    def fused_step(self, st, traj, row, noise, cond_data, cond_mask_u8, tables):
        """One denoise step: network evaluation + DDPM reverse step -> the next trajectory (B, L, D).  tables is what st was built
        on: a DDPMTables -- row is the timestep (a3d_dn_tail); a SamplerSchedule -- row is the step's POSITION, and the step at
        position K - 1 returns the in-painted network output (a3d_dn_tail_sched).  noise: this step's (B, L, D) draw or None."""
        Lb = O.L
        out = torch.empty_like(traj)
        B, Ln, D = traj.shape
        H = self.num_attn_heads
        E = st["sem"].shape[-1]
        dev = traj.device
        new = lambda: torch.empty((B, Ln, E), device=dev, dtype=torch.float32)
        hp = self._dn_head_params(st)
        x = new()
        Lb.call("a3d_dn_head", traj.data_ptr(), D, Lb.byref(hp), x.data_ptr(), B, Ln, E, H, Lb.stream())

        def run_layer(xin, rec, ws):
            stream = Lb.stream()
            cp, rp = self._dn_cross_params(st, rec, row), self._dn_rest_params(st, rec, row)
            Lb.call("a3d_dn_cross", xin.data_ptr(), traj.data_ptr(), D, Lb.byref(cp), ws.data_ptr(), B, Ln, E, H, st["S"],
                    st["Sp"], st["nsplit"], stream)
            xout = new()
            Lb.call("a3d_dn_rest", xin.data_ptr(), traj.data_ptr(), D, ws.data_ptr(), Lb.byref(rp), xout.data_ptr(), B, Ln,
                    E, H, st["nsplit"], stream)
            return xout

        recs = st["layers"]
        n_traj = len(self.traj_attention[0].layers)
        n_pos = len(self.pos_attention[0].layers)
        for rec in recs[:n_traj]:
            x = run_layer(x, rec, st["ws"])
        # the position and rotation stacks (diffusion_head.py:343-357) both start from x and are independent: the rotation
        # stack runs on a side stream (fork / join on events: capturable), its 64-workgroup per-sample kernels filling CUs
        # the position stack leaves idle
        cur = torch.cuda.current_stream(dev)
        side = _dn_side_stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            rf = x
            for rec in recs[n_traj + n_pos:]:
                rf = run_layer(rf, rec, st["ws_side"])
        pf = x
        for rec in recs[n_traj:n_traj + n_pos]:
            pf = run_layer(pf, rec, st["ws"])
        cur.wait_stream(side)
        rf.record_stream(cur)
        tp = self._dn_tail_params(noise, cond_data, cond_mask_u8, tables, st.get("hist"))
        tail = (pf.data_ptr(), rf.data_ptr(), traj.data_ptr(), D, Lb.byref(tp), out.data_ptr(), B, Ln, E, int(row))
        if not isinstance(tables, SamplerSchedule):
            Lb.call("a3d_dn_tail", *tail, Lb.stream())
        else:
            Lb.call("a3d_dn_tail_sched", *tail, int(row == tables.K - 1), Lb.stream())
        return out


# workgroups the cached cross-attention kernel aims for (key splits x samples x heads).  Every split repeats the query
# projection and adds a combine term, so splits only pay while the grid is smaller than the chip: measured at cfg-3
# (B x H = 512) 1 split 0.924 ms per denoise step, 2 splits 0.955, 4 splits 1.04, 8 splits 1.20
DN_TARGET_WGS = int(os.environ.get("A3D_DN_TARGET_WGS", "512"))
FUSED_DENOISE = os.environ.get("A3D_DN_FUSED", "1") == "1"
# the sampling loop as ONE launch of the persistent two-role kernel (a3d_dn_persist); A3D_DN_PERSIST=0: one launch per phase
# (head, per layer cross + rest, tail: 18 per step).  A3D_DN_PERSIST_SPLIT: key splits per (sample, layer) = items of the ready queue.
DN_PERSIST = os.environ.get("A3D_DN_PERSIST", "1") == "1"
# (round 6: 6 -- 0.730 ms per denoise step at cfg-3 against 0.755 with 8 and 0.749 with 4, profiles/r06_sampler_split.json: fewer,
# longer items amortise the ~9 us of per-item overhead until the sample role starts to wait for its last item)
DN_PERSIST_SPLIT = int(os.environ.get("A3D_DN_PERSIST_SPLIT", "6"))
# An aborted persistent launch (a co-resident workgroup never arrived) poisons the whole trajectory batch with NaN inside the launch
# sequence itself (dn_persist_poison_kernel), so the failure is visible in the result without a host synchronisation, eager or
# replayed.  A3D_DN_PERSIST_CHECK=1 additionally synchronises after every launch and raises on the abort word.
DN_PERSIST_CHECK = os.environ.get("A3D_DN_PERSIST_CHECK", "0") == "1"
_DN_SIDE = {}


def _as_list(x):
    """Per-scale tensors as a list: a single-scale head passes the bare tensor."""
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _dn_side_stream(dev):
    key = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    if key not in _DN_SIDE:
        _DN_SIDE[key] = torch.cuda.Stream(device=dev)
    return _DN_SIDE[key]


def persist_fits(n_traj, Ln, H, cus):
    """Whether the persistent sampler can serve n_traj trajectories of Ln steps on a device of `cus` compute units: two sample-role
    workgroups per (trajectory, 16-step row tile) -- primary + rotation-stack helper -- and >= 16 streamers, all co-resident; at most
    four row tiles and eight heads."""
    NT = -(-Ln // 16)
    return 2 * n_traj * NT + 16 <= cus and H <= 8 and NT <= 4


# path: "multi-round" | "persistent" | "per-phase" | "op-by-op"; group: candidate groups on the per-scene cache (a3d_dn_persist_group);
# scheduled / K: tables by step position, K rows (else by timestep, K None); flip_noise: the by-timestep noise of a full chain is read
# in step order; steps: the timesteps to run; label: what last_sampler_path reports
SamplerPlan = collections.namedtuple("SamplerPlan", ("path", "group", "scheduled", "K", "flip_noise", "steps", "label"))


def sampler_plan(B, G, Ln, D, E, H, T, cus, multi=False, fused=None, num_inference_steps=None, scheduler="ddpm", eta=0.0,
                 n_steps=None):
    """Which launches serve a compute_trajectory call, from host values alone: B scenes x G candidates (G None: one trajectory per
    scene, no candidate axis) of Ln steps and D signal channels, embedding E, H heads, T training timesteps, a device of `cus`
    compute units; multi: a multi-round / multi-scale head; the other arguments are compute_trajectory's.

      multi-round   a multi-round head: nothing but the image encoding is step-invariant, every step evaluates the full head
      persistent    the fused kernels serve the shape (`fused` below: E, D and the L x D tile they stage), A3D_DN_PERSIST and persist_fits:
                    the whole loop is one launch -- a3d_dn_persist (full chain), a3d_dn_persist_sched (schedule) or, with G,
                    a3d_dn_persist_group on the per-scene cache (the full chain then runs as the K = T "ddpm" schedule: the same
                    coefficients and AdaLN rows, bit for bit, with the noise of timestep t at row T - 1 - t)
      per-phase     the fused kernels serve the shape and L <= 16 (one row tile): 2 + 2 * layers launches per step
      op-by-op      everything else: the K/V cache and one launch per operation

    With G and any path but the persistent one the context is expanded along the batch axis (group False).  The module switches
    are read here, at call time."""
    scheduled = num_inference_steps is not None or scheduler != "ddpm" or eta != 0.0
    K = check_sampler_args(T, num_inference_steps, scheduler, eta) if scheduled else None
    fused = (FUSED_DENOISE if fused is None else fused) and E <= 128 and D <= 16 and min(Ln, 16) * D <= 160
    if multi:
        path = "multi-round"
    elif fused and DN_PERSIST and persist_fits(B * (G or 1), Ln, H, cus):
        path = "persistent"
    elif fused and Ln <= 16:
        path = "per-phase"
    else:
        path = "op-by-op"
    group = G is not None and path == "persistent"
    flip_noise = group and not scheduled
    if flip_noise:
        scheduled, K = True, T
    steps = sampler_timesteps(T, K)[0] if scheduled else list(range(T - 1, -1, -1))
    if n_steps is not None:
        steps = steps[:n_steps]
    label = {"multi-round": "multi-round", "per-phase": "per-phase fused launches", "op-by-op": "op-by-op",
             "persistent": "persistent (a3d_dn_persist%s)" % ("_group" if group else "_sched" if scheduled else "")}[path]
    return SamplerPlan(path, group, scheduled, K, flip_noise, tuple(steps), label)


# what check_sampling_call derives from the keywords of a sampling call: G candidates per scene (None: no candidate axis); K steps of
# the sampler schedule (None: the full chain); the normalised guide (push, smooth, start) or None; the ranking rule's clearance
# weight (0.0 without one); margin, skip = (head, tail) of the clearance term and cams, pix of the cloud -- None where neither the
# guide nor the ranking reads the cloud
_SamplingCall = collections.namedtuple("_SamplingCall", ("G", "K", "guide", "w_clear", "margin", "skip", "cams", "pix"))


def check_sampling_call(B, Ln, D, T, pcd_obs, have_goal=True, *, num_samples=None, num_inference_steps=None, scheduler="ddpm", eta=0.0,
                        init_noise=None, step_noise=None, n_steps=None, select=None, rot_weight=1.0, scene_mask=None,
                        clear_margin=0.05, clear_skip=(1, 1), guide=None, solver_order=2, lower_order_final=True, pins=None,
                        clear_body=None):
    """Every host-side check of a sampling call (compute_trajectory, Actioner.predict), on shapes and Python values alone: nothing
    is launched, so a bad argument raises before any kernel runs.  B scenes of Ln steps and D = pose width + 2 signal channels; T:
    the chain length, or None where the caller leaves the schedule and the noise tables to the sampler (Actioner.predict, whose
    keypose half these never held up); pcd_obs: the cloud the ranking / the guide would read; the keywords are compute_trajectory's
    (_TRAJ_KW; n_steps only truncates the step list: nothing to check).  Returns a _SamplingCall."""
    G = None if num_samples is None else check_num_samples(num_samples)
    w_clear, scene = 0.0, (None,) * 5
    if select is not None:
        if G is None:
            raise ValueError("select ranks the candidates of a num_samples=G call: give num_samples")
        if G > RANK_MAX_CANDIDATES:
            raise ValueError("select serves at most %d candidates per scene, num_samples is %d" % (RANK_MAX_CANDIDATES, G))
        if D - 2 not in (7, 8):
            raise ValueError("select ranks pose rows of 7 or 8 channels, curr_gripper has %d" % (D - 2))
        _, w_clear = check_scene_select(select, have_goal, True, True)
        check_rot_weight(rot_weight)
        if w_clear != 0.0:
            scene = check_scene(pcd_obs, scene_mask, B) + check_clearance_args(clear_margin, clear_skip)
    K = None
    if T is not None and (num_inference_steps is not None or scheduler != "ddpm" or eta != 0.0 or solver_order != 2
                          or lower_order_final is not True):
        K = check_sampler_args(T, num_inference_steps, scheduler, eta, solver_order, lower_order_final)
        if step_noise is not None and step_noise.shape[0] != K:
            raise ValueError("step_noise has %d leading rows for a schedule of %d steps (one row per step position)"
                             % (step_noise.shape[0], K))
    if T is None:
        check_solver_args(scheduler, eta, solver_order, lower_order_final)
    if pins is not None:
        check_pins(pins, B, D - 2)
    if clear_body is not None:
        check_body(clear_body)                              # whatever the rule weighs; nothing is copied to a device here
    guide = check_guide(guide)
    if guide is not None:
        check_guide_shape(G or 1, Ln, D)
        scene = check_scene(pcd_obs, scene_mask, B) + check_clearance_args(clear_margin, clear_skip)
    if G is not None and T is not None:
        check_candidate_noise(init_noise, step_noise, B, G, Ln, D, K or T)
    cams, pix, margin, sh, st = scene
    return _SamplingCall(G, K, guide, w_clear, margin, None if sh is None else (sh, st), cams, pix)


def _graph_replay(gr, key, capture, srcs, dsts=lambda gr: gr["static"]):
    """One captured graph per owner (DiffusionPlanner._graph, Actioner._graph): replays the owner's record `gr` (None before the
    first capture) after refreshing its static inputs from `srcs`, capturing first where gr was taken under another key (shapes,
    steps, path, schedule, ...).  Returns the record, which the owner keeps: {"key", <what capture() retains>, "out", "g"}.
    capture() -- called only by a call that captures -- returns (run, keep, after_warmup): run() issues the launches and returns
    their result; keep is the dict of EVERY buffer the captured launches address (they must stay alive as long as the graph:
    workspaces, the persistent sampler's tables, the static inputs as keep["static"]); after_warmup (or None) runs on the warm-up
    stream once the warm-up has been issued, to undo what it must not leave behind.  dsts(gr): the captured tensors srcs go to."""
    if gr is None or gr["key"] != key:
        run, keep, after_warmup = capture()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()                                           # warm-up (allocator, lazy module state) outside capture
            if after_warmup is not None:
                after_warmup()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        gr = dict(key=key, **keep)
        with torch.cuda.graph(g):
            gr["out"] = run()
        gr["g"] = g
    # refresh the captured buffers in place (same addresses; the key pins every shape and dtype)
    for dst, src in zip(dsts(gr), srcs):
        if dst is not src:
            dst.copy_(src)
    gr["g"].replay()
    return gr


# the conditioning of a sampling call, the only record that knows both batches: B_scene scenes and B = B_scene x candidates
# trajectories.  tokens / ctx_xyz (one entry per scale), instruction, cg, gg and trajectory_mask are per scene on the candidate-group
# path and per trajectory (expanded) on every other; cond_data, cond_mask_u8, kmask, step_noise and traj are per trajectory
_Conditioned = collections.namedtuple("_Conditioned", ("B_scene", "B", "tokens", "ctx_xyz", "instruction", "cg", "gg", "trajectory_mask",
                                                       "cond_data", "cond_mask_u8", "kmask", "step_noise", "traj"))


class DiffusionPlanner(nn.Module):

    def __init__(self, backbone="clip", image_size=(256, 256), embedding_dim=60, output_dim=7,
                 num_vis_ins_attn_layers=2, num_query_cross_attn_layers=8, use_instruction=False, use_goal=False,
                 use_goal_at_test=True, feat_scales_to_use=1, attn_rounds=1, weight_tying=False,
                 gripper_loc_bounds=None, rotation_parametrization='quat', diffusion_timesteps=100, num_attn_heads=8,
                 dropout=0.1, dropout_seed=0):
        super().__init__()
        if rotation_parametrization != '6D':
            raise NotImplementedError("only rotation_parametrization='6D' (scripts/train_trajectory.sh) is implemented")
        self._use_goal, self._use_goal_at_test = use_goal, use_goal_at_test
        self._rotation_parametrization = rotation_parametrization
        self.prediction_head = DiffusionHead(
            backbone=backbone, image_size=image_size, embedding_dim=embedding_dim, output_dim=output_dim,
            num_attn_heads=num_attn_heads, num_vis_ins_attn_layers=num_vis_ins_attn_layers,
            num_query_cross_attn_layers=num_query_cross_attn_layers, use_instruction=use_instruction, use_goal=use_goal,
            feat_scales_to_use=feat_scales_to_use, attn_rounds=attn_rounds, weight_tying=weight_tying,
            rotation_parametrization=rotation_parametrization, dropout=dropout, dropout_seed=dropout_seed)
        self.n_steps = diffusion_timesteps
        self.register_buffer("gripper_loc_bounds", torch.tensor(gripper_loc_bounds, dtype=torch.float32), persistent=False)
        self._tables = None
        self._graph = None
        self.last_ranking = None
        self.last_guidance = None
        self.last_pins = None

    # ---- helpers (diffusion_model.py:187-230)
    def tables(self, device):
        if self._tables is None or self._tables.acp_pos.device != device:
            self._tables = DDPMTables(self.n_steps, device)
            E = self.prediction_head.curr_gripper_embed.weight.shape[1]
            sin = O.sinusoidal_emb(torch.arange(self.n_steps, device=device, dtype=torch.float32), E)
            self._time_tables = {"sin": sin, "silu": F.silu(sin)}
            self._schedules = {}
        return self._tables

    def schedule(self, device, num_inference_steps=None, scheduler="ddpm", eta=0.0, solver_order=2, lower_order_final=True):
        """The SamplerSchedule of (K, scheduler, eta[, solver_order, lower_order_final]) on `device` (built once and kept: a captured
        graph addresses its tables), with time_sin = the sinusoidal embedding rows of its K timesteps in step order."""
        tb = self.tables(device)
        key = (check_sampler_args(self.n_steps, num_inference_steps, scheduler, eta, solver_order, lower_order_final), scheduler,
               float(eta), solver_order, lower_order_final)
        if key not in self._schedules:
            sc = SamplerSchedule(tb, *key)
            sc.time_sin = self._time_tables["sin"][torch.tensor(sc.timesteps, device=device)].contiguous()
            self._schedules[key] = sc
        return self._schedules[key]

    def normalize_pos(self, pos):
        lo, hi = self.gripper_loc_bounds[0], self.gripper_loc_bounds[1]
        return (pos - lo) / (hi - lo) * 2.0 - 1.0

    def unnormalize_pos(self, pos):
        lo, hi = self.gripper_loc_bounds[0], self.gripper_loc_bounds[1]
        return (pos + 1.0) / 2.0 * (hi - lo) + lo

    def convert_rot(self, signal):
        return pose_to_signal(signal)

    def unconvert_rot(self, signal):
        return signal_to_pose(signal)

    def _prepare(self, rgb_obs, pcd_obs, curr_gripper, goal_gripper, visual_tokens, signals=True):
        """Normalised, converted conditioning + visual tokens and their (normalised, down-sampled) coordinates
        (one tensor each, or one per scale for a multi-scale head).  signals=False: the caller converts the two poses itself
        (traj_condition) -- cg and gg come back as None."""
        head = self.prediction_head
        with torch.no_grad():
            pcd_n = self.normalize_pos(pcd_obs.float().permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3).contiguous()
            by_factor = {}
            for f in head.downscaling_factor_pyramid[:head.feat_scales]:
                if f not in by_factor:
                    by_factor[f] = O.pcd_downsample(pcd_n, f)
            ctx_xyz = [by_factor[f] for f in head.downscaling_factor_pyramid[:head.feat_scales]]
            cg = pose_to_signal(curr_gripper, self.gripper_loc_bounds) if signals else None
            gg = pose_to_signal(goal_gripper, self.gripper_loc_bounds) if signals else None
        tokens = visual_tokens if visual_tokens is not None else head.encode_images(rgb_obs, pcd_n)
        if head.feat_scales == 1:
            ctx_xyz = ctx_xyz[0]
        return tokens, ctx_xyz, cg, gg

    # ---- training (diffusion_model.py:253-324)
    def forward(self, gt_trajectory, trajectory_mask, rgb_obs, pcd_obs, instruction, curr_gripper, goal_gripper,
                run_inference=False, *, noise=None, timesteps=None, visual_tokens=None, return_pred=False, **sample_kw):
        if run_inference:
            return self.compute_trajectory(trajectory_mask, rgb_obs, pcd_obs, instruction, curr_gripper, goal_gripper,
                                           visual_tokens=visual_tokens, **sample_kw)
        head = self.prediction_head
        dev = pcd_obs.device
        tb = self.tables(dev)
        tokens, ctx_xyz, cg, gg = self._prepare(rgb_obs, pcd_obs, curr_gripper, goal_gripper, visual_tokens)
        with torch.no_grad():
            gt = pose_to_signal(gt_trajectory, self.gripper_loc_bounds)
            if noise is None:
                noise = torch.randn(gt.shape, device=dev)
            if timesteps is None:
                timesteps = torch.randint(0, self.n_steps, (gt.shape[0],), device=dev).long()
            gt = gt[..., :9].contiguous()               # the reference rebuilds the 9 pose channels (diffusion_model.py:296-305)
            noisy = O.ddpm_add_noise(gt, noise.to(dev).float()[..., :9].contiguous(), timesteps.to(dev), tb.acp_pos, tb.acp_rot)
        if head.attn_rounds * head.feat_scales > 1:
            # every iteration's prediction is supervised (diffusion_model.py:313-323)
            preds = head.forward_multi(noisy, trajectory_mask, timesteps.to(dev), _as_list(tokens), _as_list(ctx_xyz), instruction, cg, gg,
                                       head.begin_dropout if (head.training and head.dropout_p > 0) else None)
            loss = sum(O.ElemLossFn.apply(p_[..., :3], gt[..., :3], 1, 100.0) + O.ElemLossFn.apply(p_[..., 3:9], gt[..., 3:9], 1, 10.0)
                       for p_ in preds)
            return (loss, preds, gt) if return_pred else loss
        drop = head.begin_dropout()
        ctx, ctx_xyz, instr = head.encode_context(tokens, ctx_xyz, instruction, cg, gg, drop=drop)
        pred = head.forward_tokens(noisy, trajectory_mask, timesteps.to(dev), ctx, ctx_xyz, instr, drop=drop)
        loss = O.ElemLossFn.apply(pred[..., :3], gt[..., :3], 1, 100.0) + O.ElemLossFn.apply(pred[..., 3:9], gt[..., 3:9], 1, 10.0)
        return (loss, pred, gt) if return_pred else loss

    # ---- sampling (diffusion_model.py:86-185)
    @torch.no_grad()
    def compute_trajectory(self, trajectory_mask, rgb_obs, pcd_obs, instruction, curr_gripper, goal_gripper, *,
                           init_noise=None, step_noise=None, visual_tokens=None, use_graph=False, n_steps=None,
                           return_trace=False, fused=None, num_inference_steps=None, scheduler="ddpm", eta=0.0, num_samples=None,
                           fused_conditioning=False, select=None, rot_weight=1.0, scene_mask=None, clear_margin=0.05,
                           clear_skip=(1, 1), guide=None, solver_order=2, lower_order_final=True, pins=None, clear_body=None):
        """Samples a trajectory batch.  By default the full chain of diffusion_timesteps ancestral DDPM steps, as the reference.
        num_inference_steps = K / scheduler / eta select a few-step sampler schedule instead (SamplerSchedule: K evenly strided
        timesteps, scheduler "ddpm" = strided ancestral sampling, "ddim" with 0 <= eta <= 1); step_noise is then (K, B, L, D) with row
        i used by the i-th executed step, and is neither drawn nor read for "ddim" with eta = 0.  n_steps truncates the (scheduled)
        step list for fixtures; a truncated run has no terminal step.
        scheduler = "dpm++": DPM-Solver++ (2M), the second-order multistep solver for a 5 - 20 step budget (sampler_kappa): the
        "ddim", eta = 0 update plus one term on the previous step's prediction -- no further network evaluation, noise table or launch.
        solver_order = 1 is "ddim" with eta = 0, bit for bit; lower_order_final = True (default) makes the last update, the one that
        lands on timestep 0, first-order.  eta must be 0, no step noise is drawn or read (a given step_noise is ignored), and the two
        keywords are accepted only with this scheduler.
        num_samples = G (an integer >= 1) draws G candidate trajectories per scene and returns (B, G, L, 8) (trace entries
        (B, G, L, D)): init_noise is then (B, G, L, D) and step_noise (steps, B, G, L, D); every other input stays per scene.  The
        step-invariant setup (encoding, K / V cache, instruction rows) runs once per scene and the persistent sampler streams a
        scene's cache once for a chunk of candidates (a3d_dn_persist_group); trajectory b G + g belongs to scene b.  Where that
        kernel cannot serve the call (A3D_DN_PERSIST=0, too many trajectories for the CU count, multi-round heads, fused=False)
        the context is expanded along the batch axis and the call runs on the single-candidate paths.
        fused_conditioning=True: the two pose conversions, the in-painting data / mask, the key mask and the noisy start trajectory
        come from ONE launch (traj_condition) instead of ~25 small ones, per trajectory of a multi-candidate call included; the
        result is the same, bit for bit.
        select (needs num_samples): a rule of rank_trajectories (a preset name or a dict of term weights).  The G candidates are
        ranked on the device in one launch after signal_to_pose (with use_graph: after the replay) and the call returns the
        selected trajectory (B, L, 8), the single-trajectory shape; the goal and the workspace bounds of the ranking are this call's
        goal_gripper and gripper_loc_bounds, rot_weight its rotation weight.  self.last_ranking keeps best / order / scores / terms /
        selected and all candidates (B, G, L, 8).  Trace entries stay (B, G, L, D).  None (default): today's path and result.
        A rule that weighs "clearance" (or the preset "clear") scores the candidates against THIS call's pcd_obs, the caller's
        tensor in world coordinates, read in place (trajectory_clearance); scene_mask (B, C, H, W) drops points (the robot's own),
        clear_margin / clear_skip are its margin and skip.  self.last_ranking then also carries clearance (B, G) and nearest
        (B, G, L), before candidates.
        clear_body: None or a gripper body (trajectory.check_body: sphere centres in the tool frame, radii, sweep).  With a rule that
        weighs "clearance" the term and last_ranking.nearest then come from body_clearance: the spheres turn with every waypoint and
        are swept along the segments between waypoints.  With any other rule the body is checked and otherwise ignored.  No preset
        body ships (body_clearance says why).  `guide` keeps pushing the tool point.  None (default): today's launches and bits.
        guide: clearance guidance WHILE the trajectory is drawn (guide_trajectories, a3d_traj_guide).  A number is the push; a dict
        maps "push" (default 1.0), "smooth" (0.0) and "start" (0.5, in [0, 1)) to numbers.  With n executed steps, the step at
        position i >= floor(start n) is followed by one guide step on the signal it produced (the terminal step always is), on
        every sampler path: guided_segments is the launch list, each run of unguided steps stays one launch where the path has
        one.  The cloud is THIS call's pcd_obs in world coordinates, read in place when eager (a replayed graph reads a copy the
        planner owns and refreshes); the margin, the skip and the point mask are clear_margin, clear_skip and scene_mask; the
        pinned rows are the in-painted ones.  It composes with num_samples / select unchanged.  self.last_guidance =
        Guidance(steps = the guided positions, nearest = the distances the LAST guide step found before its push, (B, G, L) or
        (B, L)).  None (default): today's launches and today's bits.
        pins: pinned waypoints (check_pins: poses (B, P, Dp), index (B, P), channels; P <= 32), per scene.  The sampler in-paints
        them exactly as it in-paints the start and the goal: one more launch (traj_pins, a3d_traj_pins) fills the in-painting data /
        mask and the noisy start trajectory of every candidate of the scene, on either conditioning path with the same bits, and
        every step of every sampler path and scheduler then returns the pinned elements unchanged.  A pin is applied iff its row lies
        strictly between row 0 and the goal row (up to the last valid row without a goal) -- start and goal keep priority, padded
        rows are never touched; out-of-range pins are dropped on the device and self.last_pins = Pins(index, applied) (device
        tensors, nothing is synchronised) reports them.  prefix_pins builds the pins of a receding-horizon replan.  With use_graph
        the launch stays outside the captured loop, whose in-painting tensors and start trajectory every replay refreshes: other
        pins, another P or none replay the same graph.  With guide, a row whose POSITION is pinned is never pushed (the guide reads
        the first mask byte of a row); a rotation-only pin leaves the row free.  None (default): today's launches and today's bits,
        last_pins = None."""
        head = self.prediction_head
        dev = pcd_obs.device
        B_scene, Ln = trajectory_mask.shape
        D = curr_gripper.shape[-1] + 2
        # host-side checks first: bad arguments raise before anything is launched
        call = check_sampling_call(B_scene, Ln, D, self.n_steps, pcd_obs, goal_gripper is not None, num_samples=num_samples,
                                   num_inference_steps=num_inference_steps, scheduler=scheduler, eta=eta, init_noise=init_noise,
                                   step_noise=step_noise, n_steps=n_steps, select=select, rot_weight=rot_weight, scene_mask=scene_mask,
                                   clear_margin=clear_margin, clear_skip=clear_skip, guide=guide, solver_order=solver_order,
                                   lower_order_final=lower_order_final, pins=pins, clear_body=clear_body)
        # ---- the plan: which launches serve the call, from the shapes and the CU count alone
        multi = head.attn_rounds * head.feat_scales > 1
        plan = sampler_plan(B_scene, call.G, Ln, D, head.curr_gripper_embed.weight.shape[1], head.num_attn_heads, self.n_steps,
                            torch.cuda.get_device_properties(dev).multi_processor_count, multi, fused, num_inference_steps, scheduler,
                            eta, n_steps)
        tb = self.tables(dev)
        sched = self.schedule(dev, plan.K, scheduler, eta, solver_order, lower_order_final) if plan.scheduled else None
        c = self._condition(plan, sched, call.G, trajectory_mask, rgb_obs, pcd_obs, instruction, curr_gripper, goal_gripper,
                            init_noise, step_noise, visual_tokens, fused_conditioning, pins)
        replay = use_graph and not return_trace
        state, static, key, gd = self._sampler_state(plan, sched, call, c, pcd_obs, trajectory_mask, scene_mask, fused_conditioning,
                                                     replay)
        if call.G is not None:
            self._last_state = state                        # tests read the leading dimensions of the cache
        self.last_sampler_path = plan.label                 # which sampler serves this call (read by the bench line and the tests)
        segments = guided_segments(len(plan.steps), None if call.guide is None else call.guide[2])
        trace = [] if return_trace else None
        run = lambda x: self._run_steps(x, plan, tb if sched is None else sched, call, c, state, gd, segments, trace)
        traj = self._replay(key, run, c.traj, static, state) if replay else run(c.traj)
        return self._finish(call, c, traj, trace, gd, segments, replay, trajectory_mask, pcd_obs, goal_gripper, select, rot_weight,
                            scene_mask, clear_margin, clear_skip, clear_body)

    def _condition(self, plan, sched, G, trajectory_mask, rgb_obs, pcd_obs, instruction, curr_gripper, goal_gripper, init_noise,
                   step_noise, visual_tokens, fused_conditioning, pins=None):
        """The conditioning of a sampling call -> _Conditioned: visual tokens, the two poses as signals, the in-painting data / mask,
        the key mask, the candidate reshaping / expansion, the noise defaults and the noisy start trajectory.  pins: one more launch
        (traj_pins) on the per-trajectory in-painting tensors, with the call's own per-scene mask; self.last_pins keeps its record."""
        dev = pcd_obs.device
        scene_mask_rows = trajectory_mask                   # per scene, whatever the candidate expansion below does
        self.last_pins = None
        B_scene, Ln = trajectory_mask.shape
        D = curr_gripper.shape[-1] + 2
        B = B_scene * (G or 1)
        tokens, ctx_xyz, cg, gg = self._prepare(rgb_obs, pcd_obs, curr_gripper, goal_gripper, visual_tokens,
                                                signals=not fused_conditioning)
        tokens, ctx_xyz = _as_list(tokens), _as_list(ctx_xyz)      # one entry per scale
        if fused_conditioning:
            # every per-trajectory conditioning tensor at once, before the candidate expansion below (the kernel expands itself)
            if init_noise is None:
                init_noise = torch.randn((B, Ln, D), device=dev)
            else:
                init_noise = init_noise.to(dev).float().reshape(B, Ln, -1)
            cg, gg, cond_data, cond_mask_u8, kmask, traj = traj_condition(
                curr_gripper, goal_gripper, self.gripper_loc_bounds, trajectory_mask, init_noise, G or 1, self._use_goal_at_test)
            if pins is not None:
                self._pin(pins, cond_data, cond_mask_u8, traj, init_noise, scene_mask_rows, G or 1)
        if G is not None:
            if init_noise is not None:
                init_noise = init_noise.reshape(B, Ln, -1)
            if step_noise is not None:
                step_noise = step_noise.reshape(step_noise.shape[0], B, Ln, -1)
                if plan.flip_noise:
                    step_noise = step_noise.flip(0)
            if not plan.group:
                # fallback paths: every scene's inputs G times along the batch axis (after the image encoding, which stays per scene)
                rep_ = lambda x: None if x is None else x.repeat_interleave(G, 0)
                tokens, ctx_xyz = [rep_(x) for x in tokens], [rep_(x) for x in ctx_xyz]
                cg, gg, instruction, trajectory_mask = rep_(cg), rep_(gg), rep_(instruction), rep_(trajectory_mask)
        if not fused_conditioning:
            # start pose at index 0, goal at L - pad - 1 and after (no host sync: index arithmetic on device)
            rows = trajectory_mask.shape[0]                 # per scene on the candidate-group path (expanded below), else per trajectory
            ar = torch.arange(Ln, device=dev)[None, :]
            cond_mask = (ar == 0)
            cond_data = torch.zeros((rows, Ln, D), device=dev)
            cond_data[:, 0] = cg
            if self._use_goal_at_test:
                gidx = (Ln - trajectory_mask.sum(1).long() - 1)[:, None]
                cond_mask = cond_mask | (ar >= gidx)
                cond_data = torch.where((ar == gidx)[..., None], gg[:, None, :], cond_data)
            cond_mask_u8 = cond_mask[..., None].expand(rows, Ln, D).to(torch.uint8).contiguous()
            cond_data = cond_data.contiguous()
            kmask = trajectory_mask.to(torch.uint8).contiguous()
            if plan.group:
                # per trajectory from here on: conditioning, masks, noise, the trajectory itself (scene-major); ctx / instr stay per scene
                cond_mask_u8, cond_data, kmask = (x.repeat_interleave(G, 0).contiguous() for x in (cond_mask_u8, cond_data, kmask))
            if pins is not None:
                # on the per-trajectory tensors, before the start trajectory is formed from them: the kernel expands the scene's pins
                self._pin(pins, cond_data, cond_mask_u8, None, None, scene_mask_rows, G or 1)
        if init_noise is None:
            init_noise = torch.randn((B, Ln, D), device=dev)
        if sched is not None and sched.noise_free:
            step_noise = None                               # DDIM with eta = 0: no draw is made, captured or read
        else:
            if step_noise is None:
                step_noise = torch.randn((self.n_steps if sched is None else sched.K, B, Ln, D), device=dev)
            step_noise = step_noise.to(dev).float().contiguous()
        if not fused_conditioning:
            traj = (init_noise.to(dev).float() + cond_data).contiguous()
        return _Conditioned(B_scene, B, tokens, ctx_xyz, instruction, cg, gg, trajectory_mask, cond_data, cond_mask_u8, kmask,
                            step_noise, traj)

    def _pin(self, pins, cond_data, cond_mask_u8, traj, init_noise, trajectory_mask, G):
        """traj_pins on the call's in-painting tensors; last_pins = Pins(index, applied), (B, P) device tensors, nothing synchronised"""
        applied = traj_pins(cond_data, cond_mask_u8, traj, init_noise, pins, self.gripper_loc_bounds, trajectory_mask, G,
                            self._use_goal_at_test)
        index = pins["index"] if isinstance(pins, dict) else pins.index
        self.last_pins = Pins(index.detach().to(device=applied.device, dtype=torch.int32), applied)

    def _sampler_state(self, plan, sched, call, c, pcd_obs, trajectory_mask, scene_mask, fused_conditioning, replay):
        """The step-invariant state of the planned path -> (state, static, key, gd): static is what a captured graph refreshes in
        place, key names the graph that serves the call, gd holds what the guide pair reads (None without a guide).  trajectory_mask:
        the call's own, per scene."""
        head = self.prediction_head
        Ln = c.traj.shape[1]
        # tables of the AdaLN modulation: by timestep (full chain) or by step position (schedule)
        time_sin = self._time_tables["sin"] if sched is None else sched.time_sin
        if plan.path == "multi-round":
            # the fine-scale context follows the previous prediction, so nothing but the image encoding is step-invariant: every
            # step evaluates the full head (no K/V cache, no fused kernels)
            state, static = {"tmask": c.trajectory_mask.bool()}, c.tokens + c.ctx_xyz + [c.instruction, c.cg, c.gg]
        else:
            ctx, cxyz, instr = head.encode_context(c.tokens[0], c.ctx_xyz[0], c.instruction, c.cg, c.gg)
            if plan.path == "op-by-op":
                state = head.build_kv_cache(ctx, cxyz, instr)
                static = [kv[k] for kv in state["ctx"] for k in ("Ks", "Vt")] + \
                    ([state["lang"]["Ks"], state["lang"]["Vt"]] if "lang" in state else [])
            else:
                # fused kernels (csrc/denoise.hip); the persistent sampler's own state follows below, once the graph key is known
                state = head.build_fused(ctx, cxyz, instr, c.kmask, time_sin, Ln, n_cand=call.G if plan.group else 1)
                static = list(state["tensors"])
        static = static + ([] if c.step_noise is None else [c.step_noise]) + [c.cond_data, c.cond_mask_u8, c.kmask]
        if sched is not None:
            static = static + [sched.coef_pos, sched.coef_rot] + ([] if sched.kappa_pos is None else [sched.kappa_pos, sched.kappa_rot])
        gd = None
        if call.guide is not None:
            # what the guide pair reads: the caller's cloud and masks in place; a captured graph addresses copies the planner owns,
            # refreshed with the other static inputs, so a replay sees this call's cloud and never writes into the caller's tensor
            sc = prepare_scene(pcd_obs, scene_mask, c.B_scene)
            g_in = [sc.cloud, _mask_bytes(trajectory_mask)] + ([] if sc.mask is None else [sc.mask])
            gd = {"bounds": O._c(self.gripper_loc_bounds)}
            static = static + g_in
        # the graph key, built here and nowhere else; every option that changes the launches wraps the options before it, so the
        # last entry of a plain scheduled call is the schedule's own key (the tests read it that way)
        options = None if sched is None else sched.key
        if call.G is not None:
            options = (options, "num_samples", call.G, "group" if plan.group else "expanded")
        if fused_conditioning:
            options = (options, "fused_conditioning")
        if call.guide is not None:
            options = (options, "guide") + call.guide + (call.margin,) + call.skip + (scene_mask is not None,)
        key = (c.B, Ln, plan.steps, plan.path, tuple((tuple(t_.shape), t_.dtype) for t_ in static), options)
        captured = replay and self._graph is not None and self._graph["key"] == key
        if call.guide is not None:
            if replay and not captured:                     # this call captures: the copies are made once
                g_in = [t_.clone() for t_ in g_in]
                static[-len(g_in):] = g_in
            gd["scene"], gd["tm"] = sc._replace(cloud=g_in[0], mask=g_in[2] if len(g_in) > 2 else None), g_in[1]
        if plan.path == "persistent":
            # a replay of the captured loop addresses the state retained in self._graph: no second set of persistent-sampler buffers
            # (a ctypes table, a pageable host-to-device copy = a host sync, five allocations) that would be thrown away
            state["persist"] = self._graph["state"]["persist"] if captured else \
                head._build_persist(state, c.B, Ln, time_sin.shape[0], plan.group)
        if sched is not None and sched.kappa_pos is not None:
            # the history buffer of a multistep schedule: every non-terminal step leaves its clipped prediction there for the next one,
            # whichever launch runs it.  It belongs to the sampler state and, like the persistent sampler's buffers, to the captured
            # graph: a replay addresses the buffer of the capturing call (static holds it so that it stays with the graph; nothing
            # is copied into it -- position 0 never reads it)
            state["hist"] = self._graph["state"]["hist"] if captured else torch.zeros_like(c.cond_data)
            static = static + [state["hist"]]
        if plan.group and state.get("persist") is None:
            raise RuntimeError("num_samples: the per-scene cache was built for a3d_dn_persist_group, which cannot serve this call")
        return state, static, key, gd

    def _guide_step(self, x, last, call, c, gd):
        """The guide pair on x, the tensor a step just produced (every path returns a new one): updated in place, stream-ordered.
        last: the step was the final one -- the distances found before the push are kept as gd["nearest"]."""
        G, Ln = call.G, x.shape[1]
        if "ws" not in gd:
            gd["ws"] = scan_workspace("a3d_traj_guide", c.B_scene, G or 1, Ln, call.cams * call.pix, x.device)
        nearest = torch.empty((c.B_scene, G, Ln) if G is not None else (c.B_scene, Ln), device=x.device, dtype=torch.float32) \
            if last else None
        _guide_launch(x, gd["tm"], c.cond_mask_u8, gd["bounds"], gd["scene"], call.margin, call.skip[0], call.skip[1], call.guide[0],
                      call.guide[1], nearest, gd["ws"], c.B_scene, G or 1, Ln)
        if last:
            gd["nearest"] = nearest

    def _run_steps(self, x, plan, tables, call, c, state, gd, segments, trace):
        """The planned steps on the trajectory batch x, segment by segment (guided_segments: the steps at positions first ..
        first + count - 1 of plan.steps; guided (count = 1): then the guide pair).  tables: the DDPM-step tables, by timestep
        (DDPMTables, full chain) or by step position (SamplerSchedule).  trace: the list every step's result is appended to, or
        None.  This is what a captured graph records."""
        head = self.prediction_head
        n_exec = len(plan.steps)
        if gd is not None:
            gd.pop("ws", None)                              # a workspace per run: a captured one belongs to the graph's pool
        for first, count, guided in segments:
            if plan.path == "persistent" and trace is None:         # the whole run of steps: one launch
                x = head.fused_persist(state, x, first if plan.scheduled else plan.steps[first], count, c.step_noise, c.cond_data,
                                       c.cond_mask_u8, tables)
                if guided:
                    self._guide_step(x, first == n_exec - 1, call, c, gd)
                continue
            for i in range(first, first + count):
                t = plan.steps[i]
                # a schedule addresses its tables and its noise by step POSITION and names its terminal step (timestep 0, position
                # K - 1); the full chain addresses them by timestep.  No step at timestep 0 reads noise.
                row, term = (i, t == 0) if plan.scheduled else (t, None)
                nz = None if (c.step_noise is None or t == 0) else c.step_noise[row]
                if plan.path == "persistent":               # traced: the same kernel, one step per launch
                    x = head.fused_persist(state, x, row, 1, c.step_noise, c.cond_data, c.cond_mask_u8, tables)
                elif plan.path == "per-phase":
                    x = head.fused_step(state, x, row, nz, c.cond_data, c.cond_mask_u8, tables)
                else:
                    if plan.path == "multi-round":
                        tt = torch.full((c.B,), t, device=x.device, dtype=torch.long)
                        out = head.forward_multi(x, state["tmask"], tt, c.tokens, c.ctx_xyz, c.instruction, c.cg, c.gg)[-1]
                    else:
                        out = head.denoise_tokens_cached(x, c.kmask, t, state, self._time_tables)
                    if term is None:
                        x = O.ddpm_step(out, x, nz, c.cond_data, c.cond_mask_u8, tables.coef_pos, tables.coef_rot, row)
                    elif state.get("hist") is None:
                        x = O.ddpm_step_sched(out, x, nz, c.cond_data, c.cond_mask_u8, tables.coef_pos, tables.coef_rot, row, term)
                    else:
                        x = O.ddpm_step_sched(out, x, nz, c.cond_data, c.cond_mask_u8, tables.coef_pos, tables.coef_rot, row, term,
                                              hist=state["hist"], kappa_pos=tables.kappa_pos, kappa_rot=tables.kappa_rot)
                if guided:
                    self._guide_step(x, i == n_exec - 1, call, c, gd)
                if trace is not None:
                    trace.append(x)
        return x

    def _finish(self, call, c, traj, trace, gd, segments, replay, trajectory_mask, pcd_obs, goal_gripper, select, rot_weight,
                scene_mask, clear_margin, clear_skip, clear_body=None):
        """last_guidance, poses, the candidate axis, ranking (last_ranking) -> compute_trajectory's result.  trajectory_mask,
        pcd_obs (the caller's tensor, in world coordinates) and goal_gripper are the call's own, per scene."""
        G, Ln = call.G, traj.shape[1]
        self.last_guidance = None
        if gd is not None:
            nearest = gd.get("nearest")
            if replay:
                # the captured guide pair writes the tensor of the capturing call: kept with the graph, handed out as a copy
                nearest = self._graph.setdefault("guide_nearest", nearest).clone()
            self.last_guidance = Guidance(tuple(i for i, _, guided in segments if guided), nearest)
        final = signal_to_pose(traj, self.gripper_loc_bounds)
        if G is not None:
            final = final.reshape(c.B_scene, G, Ln, final.shape[-1])
            if trace is not None:
                trace = [x.reshape(c.B_scene, G, Ln, x.shape[-1]) for x in trace]
        if select is not None:
            rk = rank_trajectories(final, trajectory_mask, goal_gripper, self.gripper_loc_bounds, select, rot_weight, scene=pcd_obs,
                                   scene_mask=scene_mask, margin=clear_margin, skip=clear_skip, body=clear_body)
            self.last_ranking = (ScenePlannerRanking if len(rk) == 7 else PlannerRanking)(*rk, candidates=final)
            final = rk.selected
        return final if trace is None else (final, trace)

    def _replay(self, key, run, traj, static, state):
        """run(traj) through the planner's captured graph (_graph_replay): "in" is the captured start trajectory, "state" keeps every
        buffer the captured launches address alive (workspaces, the persistent sampler's tables)."""
        def capture():
            static_in = traj.clone()
            return (lambda: run(static_in)), {"in": static_in, "static": static, "state": state}, None

        self._graph = _graph_replay(self._graph, key, capture, [traj] + static, lambda gr: [gr["in"]] + gr["static"])
        return self._graph["out"]
