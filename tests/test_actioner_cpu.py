"""CPU-only tests of the chained keypose-to-trajectory call (actioner.Actioner) and of the conditioning kernel's host side:
argument validation of a3d_traj_condition without a device, every ValueError of Actioner on CPU tensors before any library call,
the backbone-sharing rule, and the plain-torch restatement of compute_trajectory's conditioning block (the reference the GPU
test compares the kernel with) on hand-written cases."""
import ctypes
import random

import pytest
import torch
import torch.nn as nn

from conftest import load_pkg


# ------------------------------------------------------------------------------------------------ the torch block, restated
def torch_condition_block(cg, gg, trajectory_mask, init_noise, G, use_goal):
    """DiffusionPlanner.compute_trajectory's conditioning (start pose on row 0, goal on row L - pad - 1 and the mask from there on,
    then G trajectories per scene, scene-major, and the noisy start trajectory) in plain torch, as the op-by-op path computes it.
    cg, gg: (B, D) signals; trajectory_mask: (B, L) bool; init_noise: (B G, L, D) or None.
    Returns (cond_data, cond_mask_u8, kmask, traj or None)."""
    B, Ln = trajectory_mask.shape
    D = cg.shape[-1]
    dev = cg.device
    ar = torch.arange(Ln, device=dev)[None, :]
    cond_mask = (ar == 0)
    cond_data = torch.zeros((B, Ln, D), device=dev)
    cond_data[:, 0] = cg
    if use_goal:
        gidx = (Ln - trajectory_mask.sum(1).long() - 1)[:, None]
        cond_mask = cond_mask | (ar >= gidx)
        cond_data = torch.where((ar == gidx)[..., None], gg[:, None, :], cond_data)
    cond_mask_u8 = cond_mask[..., None].expand(B, Ln, D).to(torch.uint8).contiguous()
    cond_data = cond_data.contiguous()
    kmask = trajectory_mask.to(torch.uint8).contiguous()
    cond_mask_u8, cond_data, kmask = (x.repeat_interleave(G, 0).contiguous() for x in (cond_mask_u8, cond_data, kmask))
    traj = None if init_noise is None else (init_noise.float() + cond_data).contiguous()
    return cond_data, cond_mask_u8, kmask, traj


def suffix_mask(pads, L):
    """(B, L) bool mask whose row b pads its last pads[b] steps"""
    return torch.arange(L)[None, :] >= (L - torch.tensor(pads))[:, None]


def test_torch_condition_block_on_hand_written_cases():
    D = 9
    cg = torch.arange(1, D + 1, dtype=torch.float32)[None] * torch.tensor([[1.0], [10.0]])          # rows 1..9 and 10..90
    gg = -cg
    L = 4
    # pad = 0 (goal on the last row), pad = L - 1 (goal on row 0: it wins over the start pose)
    data, mask, kmask, traj = torch_condition_block(cg, gg, suffix_mask([0, L - 1], L), None, 1, True)
    assert traj is None and data.shape == (2, L, D) and mask.dtype == torch.uint8 and kmask.dtype == torch.uint8
    assert torch.equal(data[0], torch.stack([cg[0], torch.zeros(D), torch.zeros(D), gg[0]]))
    assert mask[0, :, 0].tolist() == [1, 0, 0, 1] and torch.equal(mask[0], mask[0, :, :1].expand(L, D))
    assert torch.equal(data[1], torch.stack([gg[1], torch.zeros(D), torch.zeros(D), torch.zeros(D)]))
    assert mask[1, :, 0].tolist() == [1, 1, 1, 1]
    assert kmask.tolist() == [[0, 0, 0, 0], [0, 1, 1, 1]]
    # pad = L (gidx = -1): every row masked, no row holds the goal; pad = 1: goal on row L - 2
    data, mask, kmask, _ = torch_condition_block(cg, gg, suffix_mask([L, 1], L), None, 1, True)
    assert torch.equal(data[0], torch.stack([cg[0]] + [torch.zeros(D)] * 3)) and bool(mask[0].all())
    assert torch.equal(data[1], torch.stack([cg[1], torch.zeros(D), gg[1], torch.zeros(D)]))
    assert mask[1, :, 0].tolist() == [1, 0, 1, 1]
    # without the goal: the start pose on row 0 and nothing else, whatever the padding
    data, mask, _, _ = torch_condition_block(cg, gg, suffix_mask([L, 1], L), None, 1, False)
    assert torch.equal(data[:, 0], cg) and not data[:, 1:].any()
    assert mask[:, :, 0].tolist() == [[1, 0, 0, 0]] * 2
    # L = 1: pad = 0 puts the goal on the only row, pad = 1 leaves the start pose there
    data, mask, kmask, _ = torch_condition_block(cg, gg, suffix_mask([0, 1], 1), None, 1, True)
    assert torch.equal(data[:, 0], torch.stack([gg[0], cg[1]])) and bool(mask.all()) and kmask.tolist() == [[0], [1]]
    # G = 3: rows are scene-major (trajectory b G + g reads scene b) and the noise is added per trajectory
    noise = torch.arange(2 * 3 * L * D, dtype=torch.float32).reshape(6, L, D)
    data, mask, kmask, traj = torch_condition_block(cg, gg, suffix_mask([0, 2], L), noise, 3, True)
    one = torch_condition_block(cg, gg, suffix_mask([0, 2], L), None, 1, True)
    for b in range(2):
        for g in range(3):
            assert torch.equal(data[b * 3 + g], one[0][b]) and torch.equal(mask[b * 3 + g], one[1][b])
            assert torch.equal(kmask[b * 3 + g], one[2][b])
            assert torch.equal(traj[b * 3 + g], noise[b * 3 + g] + one[0][b])


# ------------------------------------------------------------------------------------------------ the C entry point
def test_traj_condition_rejects_bad_arguments_without_a_device():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    d = ctypes.c_void_p(64)                                         # aligned, never dereferenced
    call = lib.a3d_traj_condition

    def args(**kw):
        a = dict(curr=d, ldc=7, goal=d, ldg=8, bounds=d, tmask=d, noise=d, cg=d, gg=d, data=d, mask=d, kmask=d, traj=d,
                 B=2, G=1, L=16, Dp=7, use_goal=1)
        a.update(kw)
        return list(a.values()) + [None]

    for name in ("curr", "goal", "bounds", "tmask", "cg", "gg", "data", "mask", "kmask"):
        assert call(*args(**{name: None})) == -22, name
        assert b"a3d_traj_condition" in lib.a3d_last_error_string()
    assert call(*args(noise=None)) == -22                           # noise and traj go together
    assert call(*args(traj=None)) == -22
    for name in ("B", "G", "L"):
        for v in (0, -1):
            assert call(*args(**{name: v})) == -22, (name, v)
    assert call(*args(Dp=6)) == -22
    assert call(*args(Dp=31, ldc=31, ldg=31)) == -22                # D = Dp + 2 beyond the kernel's 32 signal channels
    assert call(*args(ldc=6)) == -22
    assert call(*args(Dp=8, ldg=7, ldc=8)) == -22
    assert b"leading dimension" in lib.a3d_last_error_string()


# ------------------------------------------------------------------------------------------------ Actioner on the host
class _Keypose(nn.Module):
    def __init__(self, seed=0, rot="quat_from_query"):
        super().__init__()
        torch.manual_seed(seed)
        self.backbone = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))
        self.backbone_dtype, self.fpn_dtype = torch.float32, torch.float32
        self.rotation_parametrization = rot
        self.calls = 0

    def forward(self, *a, **kw):
        self.calls += 1
        raise AssertionError("the model must not run")


class _Head(nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.backbone = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))
        self.backbone_dtype, self.fpn_dtype = torch.float32, torch.float32


class _Planner(nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        self.prediction_head = _Head(seed)

    def compute_trajectory(self, *a, **kw):
        raise AssertionError("the model must not run")


def _obs(B=2, hist=1, ncam=2, hw=8):
    return (torch.zeros(B, hist, ncam, 3, hw, hw), torch.zeros(B, hist, ncam, 3, hw, hw), torch.zeros(B, hist, 8))


def test_actioner_is_exported_and_keeps_the_reference_constructor():
    a3d = load_pkg()
    assert a3d.Actioner is a3d.actioner.Actioner
    kp, pl = _Keypose().train(), _Planner().train()
    act = a3d.Actioner(kp, pl, {"task": {0: [torch.ones(53, 512), torch.zeros(53, 512)]}},
                       ("left_shoulder", "right_shoulder", "wrist"), 7, True, True)
    assert not kp.training and not pl.training                      # the models it will use are put into eval()
    kp2 = _Keypose().train()
    a3d.Actioner(kp2, None, None, predict_keypose=False)
    assert kp2.training                                             # ... and only those
    random.seed(3)
    act.load_episode("task", 0)
    random.seed(3)
    want = random.choice([torch.ones(53, 512), torch.zeros(53, 512)])
    assert act._instr.shape == (1, 53, 512) and torch.equal(act._instr[0], want)
    act.set_instruction(torch.full((1, 53, 512), 2.0))
    assert float(act._instr[0, 0, 0]) == 2.0


def test_actioner_value_errors_are_raised_on_the_host_before_any_launch():
    a3d = load_pkg()
    A = a3d.Actioner
    rgbs, pcds, grip = _obs()
    mask = torch.zeros(2, 8, dtype=torch.bool)
    instr = torch.zeros(1, 53, 512)
    kp, pl = _Keypose(), _Planner()

    def ready(**kw):
        a = A(kp, pl, predict_keypose=True, predict_trajectory=True, **kw)
        a.set_instruction(instr)
        return a

    with pytest.raises(ValueError, match="instruction"):
        A(kp, pl, predict_trajectory=True).predict(rgbs, pcds, grip, None, mask)              # no instruction set
    for ad in (6, 9, 3):
        with pytest.raises(ValueError, match="action_dim"):
            A(kp, pl, action_dim=ad)
    for rot in ("6D_from_query", "6D_from_top_ghost"):
        with pytest.raises(ValueError, match="6D"):
            A(_Keypose(rot=rot), pl, predict_trajectory=True)
    with pytest.raises(ValueError, match="trajectory_mask"):
        ready().predict(rgbs, pcds, grip)                                                     # trajectory requested, no mask
    with pytest.raises(ValueError, match="rgbs"):
        ready().predict(rgbs[:, 0], pcds, grip, None, mask)                                   # wrong rank
    with pytest.raises(ValueError, match="pcds"):
        ready().predict(rgbs, pcds[:, 0], grip, None, mask)
    with pytest.raises(ValueError, match="gripper"):
        ready().predict(rgbs, pcds, grip[:, 0], None, mask)
    with pytest.raises(ValueError, match="batch"):
        ready().predict(rgbs, pcds[:1], grip, None, mask)
    with pytest.raises(ValueError, match="batch"):
        ready().predict(rgbs, pcds, grip[:1], None, mask)
    with pytest.raises(ValueError, match="cameras"):
        ready().predict(rgbs, pcds[:, :, :1], grip, None, mask)
    a = A(kp, pl, predict_keypose=False, predict_trajectory=True)
    a.set_instruction(instr)
    with pytest.raises(ValueError, match="gt_action"):
        a.predict(rgbs, pcds, grip, None, mask)
    with pytest.raises(ValueError, match="share_backbone"):
        A(kp, _Planner(seed=1), predict_trajectory=True, share_backbone=True)                 # different backbones
    with pytest.raises(ValueError, match="share_backbone"):
        A(kp, pl, predict_trajectory=False, share_backbone=True)                              # nothing to share with
    with pytest.raises(ValueError, match="share_backbone"):
        A(kp, pl, predict_trajectory=True, share_backbone="yes")
    assert kp.calls == 0


def test_share_backbone_rule():
    a3d = load_pkg()
    A = a3d.Actioner
    kp, same, other = _Keypose(0), _Planner(0), _Planner(0)
    with torch.no_grad():
        other.prediction_head.backbone[0].weight[1, 2, 0, 1] += 1e-3                          # one perturbed weight
    assert a3d.actioner.backbones_identical(kp, same) and not a3d.actioner.backbones_identical(kp, other)
    assert A(kp, same, predict_trajectory=True).shares_backbone                               # "auto": shares when possible
    assert A(kp, same, predict_trajectory=True, share_backbone=True).shares_backbone
    assert not A(kp, same, predict_trajectory=True, share_backbone=False).shares_backbone     # False: never
    assert not A(kp, other, predict_trajectory=True).shares_backbone                          # "auto": falls back to two passes
    with pytest.raises(ValueError, match="identical"):
        A(kp, other, predict_trajectory=True, share_backbone=True)
    # a BatchNorm buffer counts as much as a weight
    drift = _Planner(0)
    drift.prediction_head.backbone[1].running_mean += 0.5
    assert not A(kp, drift, predict_trajectory=True).shares_backbone
    # a backbone whose convolution weights its first reduced-precision pass has already converted still matches its fp32 twin
    conv = _Planner(0)
    conv.prediction_head.backbone[0].to(torch.bfloat16)
    assert A(kp, conv, predict_trajectory=True).shares_backbone
    # equal weights are not enough: the backbone dtype and the kind of maps the FPNs ask for must agree as well, at every call
    act = A(kp, same, predict_trajectory=True)
    true = A(kp, same, predict_trajectory=True, share_backbone=True)
    true.set_instruction(torch.zeros(1, 53, 512))
    same.prediction_head.backbone_dtype = torch.bfloat16
    assert not act.shares_backbone
    with pytest.raises(ValueError, match="backbone_dtype"):
        true.predict(*_obs(), None, torch.zeros(2, 8, dtype=torch.bool))
    kp.backbone_dtype = torch.bfloat16
    assert act.shares_backbone
    kp.fpn_dtype = torch.bfloat16
    assert not act.shares_backbone
    same.prediction_head.fpn_dtype = torch.bfloat16
    assert act.shares_backbone


def test_compute_trajectory_has_the_fused_conditioning_keyword_off_by_default():
    import inspect
    a3d = load_pkg()
    p = inspect.signature(a3d.DiffusionPlanner.compute_trajectory).parameters["fused_conditioning"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "a3d_traj_condition" in a3d.lib.SIGNATURES
