"""GPU tests of the chained keypose-to-trajectory call: the one-launch conditioning kernel (a3d_traj_condition) against the torch
block it replaces, compute_trajectory(fused_conditioning=True) against the default call, Actioner.predict against the two calls
written out by hand (with and without the shared backbone pass), its graph replay against an eager twin, and the candidate /
few-step options through the seam.  Every comparison is torch.equal: the chained call runs the same kernels on the same bits.

Models as in tests/test_joint_gpu.py: 128 x 128 images, 2 cameras, B = 2, Act3D with 2 levels and 128 ghost points, a planner with
E = 120 and num_query_cross_attn_layers = 2.  torch.backends.cudnn.deterministic is set for the duration of a test (the
convolution library's wide kernels are otherwise not reproducible run to run)."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import common as C  # noqa: E402
from test_actioner_cpu import suffix_mask, torch_condition_block  # noqa: E402

pytestmark = pytest.mark.gpu
IMG, NCAM, E = 128, 2, 120


@pytest.fixture(autouse=True)
def deterministic_convolutions():
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


# ------------------------------------------------------------------------------------------------ fixtures
def make_keypose(a3d, dev, seed=0):
    torch.manual_seed(seed)
    m = a3d.Act3D(image_size=(IMG, IMG), embedding_dim=60, num_attn_heads=4, gripper_loc_bounds=C.PERACT_BOUNDS,
                  num_ghost_points=128, num_ghost_points_val=128, num_sampling_level=2, sampler_seed=5).to(dev)
    return m.eval()


def make_planner(a3d, dev, seed=1, backbone_of=None):
    torch.manual_seed(seed)
    m = a3d.DiffusionPlanner(image_size=(IMG, IMG), embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=1,
                             num_query_cross_attn_layers=2, use_instruction=True, use_goal=True, use_goal_at_test=True,
                             weight_tying=True, gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D",
                             diffusion_timesteps=100).to(dev)
    for mod in m.modules():                      # AdaLN is zero-initialised in the reference; give it non-trivial weights
        if isinstance(mod, a3d.nn.AdaLN):
            torch.nn.init.normal_(mod.modulation[1].weight, std=0.02)
    if backbone_of is not None:                  # both policies load the same frozen CLIP backbone
        m.prediction_head.backbone.load_state_dict(backbone_of.backbone.state_dict())
    return m.eval()


def poses(g, n, lo, hi):
    q = torch.randn(*n, 4, generator=g)
    return torch.cat([lo + 0.15 * (hi - lo) + torch.rand(*n, 3, generator=g) * 0.7 * (hi - lo), q / q.norm(dim=-1, keepdim=True)], -1)


def observation(dev, seed, B, Ln, hist=2, pads=None):
    """rgbs in [-1, 1], pcds inside the planner's workspace, gripper history rows [pose | open], per-call noise"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(C.DIFFUSION_BOUNDS[0], dtype=torch.float32), torch.tensor(C.DIFFUSION_BOUNDS[1], dtype=torch.float32)
    o = {"rgbs": torch.rand(B, hist, NCAM, 3, IMG, IMG, generator=g) * 2 - 1,
         "pcds": lo.view(1, 1, 1, 3, 1, 1) + torch.rand(B, hist, NCAM, 3, IMG, IMG, generator=g) * (hi - lo).view(1, 1, 1, 3, 1, 1),
         "gripper": torch.cat([poses(g, (B, hist), lo, hi), torch.rand(B, hist, 1, generator=g)], -1),
         "gt_action": torch.cat([poses(g, (B, hist), lo, hi), torch.rand(B, hist, 1, generator=g)], -1),
         "mask": suffix_mask(pads if pads is not None else [3, 0][:B], Ln),
         "init_noise": torch.randn(B, Ln, 9, generator=g), "step_noise": torch.randn(100, B, Ln, 9, generator=g)}
    return {k: v.to(dev) for k, v in o.items()}


@pytest.fixture(scope="module")
def models(a3d, dev):
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        kp = make_keypose(a3d, dev)
        pl = make_planner(a3d, dev, backbone_of=kp)
        g = torch.Generator().manual_seed(77)
        instr = torch.randn(1, 53, 512, generator=g).to(dev)
        # settle: the convolution library may change a configuration's algorithm between its first calls
        o = observation(dev, 1, 2, 16)
        for _ in range(2):
            by_hand(kp, pl, instr, o, n_steps=1)
        return kp, pl, instr
    finally:
        torch.backends.cudnn.deterministic = old


RNG0 = (5, 0)


def set_rng(kp, state=RNG0):
    kp._rng_state.copy_(torch.tensor(state, dtype=torch.int64))


@torch.no_grad()
def by_hand(kp, pl, instr, o, action_dim=7, **kw):
    """the seam written out: rescale, Act3D forward, the cat, compute_trajectory"""
    B = o["rgbs"].shape[0]
    rgbs = o["rgbs"] / 2 + 0.5
    ins = instr.expand(B, -1, -1).contiguous()
    curr = o["gripper"][:, -1, :action_dim]
    pred = kp(rgbs[:, -1], o["pcds"][:, -1], ins, curr)
    action = torch.cat([pred["position"], pred["rotation"], pred["gripper"]], dim=1)
    traj = pl.compute_trajectory(o["mask"], rgbs[:, -1], o["pcds"][:, -1], ins, curr, action[..., :action_dim], **kw)
    return action, traj, pred


def abort_word(pl):
    torch.cuda.synchronize()
    ps = pl.prediction_head._last_persist
    assert ps is not None
    return int(ps["sync"][2].item())


# ------------------------------------------------------------------------------------------------ 1: the kernel
GUARD = 64


def guarded(n, dtype, dev):
    """a buffer of n elements with a poisoned band of GUARD elements on either side: (whole, view of the n elements)"""
    whole = torch.full((n + 2 * GUARD,), 85, device=dev, dtype=torch.uint8) if dtype == torch.uint8 else \
        torch.full((n + 2 * GUARD,), -12345.5, device=dev, dtype=dtype)
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    want = 85 if whole.dtype == torch.uint8 else -12345.5
    return bool((whole[:GUARD] == want).all()) and bool((whole[GUARD + n:] == want).all())


def raw_condition(a3d, curr, ldc, goal, ldg, bounds, tmask, noise, B, G, L, Dp, use_goal):
    """a3d_traj_condition into guarded output buffers; returns {name: (whole, view)}"""
    Lb, dev, D = a3d.lib, bounds.device, Dp + 2
    out = {"cg": guarded(B * D, torch.float32, dev), "gg": guarded(B * D, torch.float32, dev),
           "cond_data": guarded(B * G * L * D, torch.float32, dev), "cond_mask": guarded(B * G * L * D, torch.uint8, dev),
           "kmask": guarded(B * G * L, torch.uint8, dev), "traj": guarded(B * G * L * D, torch.float32, dev)}
    p = lambda k: out[k][1].data_ptr()
    Lb.call("a3d_traj_condition", curr.data_ptr(), ldc, goal.data_ptr(), ldg, bounds.data_ptr(), tmask.data_ptr(),
            None if noise is None else noise.data_ptr(), p("cg"), p("gg"), p("cond_data"), p("cond_mask"), p("kmask"),
            None if noise is None else p("traj"), B, G, L, Dp, int(use_goal), Lb.stream())
    return out


@pytest.mark.parametrize("B,G,L,Dp", [(1, 1, 1, 7), (2, 1, 16, 7), (3, 3, 17, 8), (2, 2, 50, 7), (2, 4, 64, 8)])
def test_kernel_equals_the_torch_block(a3d, dev, B, G, L, Dp):
    D_ = a3d.diffusion
    g = torch.Generator().manual_seed(100 * B + L)
    lo, hi = torch.tensor(C.DIFFUSION_BOUNDS[0], dtype=torch.float32), torch.tensor(C.DIFFUSION_BOUNDS[1], dtype=torch.float32)
    bounds = torch.tensor(C.DIFFUSION_BOUNDS, dtype=torch.float32).to(dev)
    # start poses: the last history row of (B, 2, 8) gripper rows (leading dimension 16); goal poses: (B, 8) action rows read at
    # Dp channels (leading dimension 8, also for Dp = 7)
    gripper = torch.cat([poses(g, (B, 2), lo, hi), torch.rand(B, 2, 1, generator=g)], -1).to(dev)
    action = torch.cat([poses(g, (B,), lo, hi), torch.rand(B, 1, generator=g)], -1).to(dev)
    curr, goal = gripper[:, -1, :Dp], action[:, :Dp]
    D = Dp + 2
    cg_ref = D_.pose_to_signal(curr.contiguous(), bounds)
    gg_ref = D_.pose_to_signal(goal.contiguous(), bounds)
    noise = torch.randn(B * G, L, D, generator=g).to(dev)
    patterns = {"none": [0] * B, "suffix": [min(L, 3 + 2 * b) for b in range(B)], "all-but-one": [L - 1] * B, "all": [L] * B,
                "mixed": [(0, L, L - 1, 1)[b % 4] if L > 1 else b % 2 for b in range(B)]}
    sizes = {"cg": B * D, "gg": B * D, "cond_data": B * G * L * D, "cond_mask": B * G * L * D, "kmask": B * G * L, "traj": B * G * L * D}
    for name, pads in patterns.items():
        mask = suffix_mask(pads, L).to(dev)
        tm = mask.view(torch.uint8)
        for use_goal in (True, False):
            for nz in (noise, None):
                data, cmask, kmask, traj = torch_condition_block(cg_ref, gg_ref, mask, nz, G, use_goal)
                want = {"cg": cg_ref, "gg": gg_ref, "cond_data": data, "cond_mask": cmask, "kmask": kmask, "traj": traj}
                runs = [raw_condition(a3d, gripper[:, -1], 16, action, 8, bounds, tm, nz, B, G, L, Dp, use_goal) for _ in range(2)]
                for k, ref in want.items():
                    whole, view = runs[0][k]
                    tag = (name, use_goal, nz is not None, k)
                    assert guards_intact(whole, sizes[k]), tag
                    if ref is None:                                  # no noise: traj is not written at all
                        assert bool((view == -12345.5).all()), tag
                        continue
                    assert torch.equal(view.view(ref.shape), ref), tag
                    assert torch.equal(runs[1][k][0], whole), tag     # a second launch is bit-identical
                # the Python wrapper reads the same strided rows in place
                got = D_.traj_condition(curr, goal, bounds, mask, nz, G, use_goal)
                for x, k in zip(got, ("cg", "gg", "cond_data", "cond_mask", "kmask", "traj")):
                    assert (x is None and want[k] is None) or torch.equal(x, want[k]), (name, use_goal, k)


# ------------------------------------------------------------------------------------------------ 2: compute_trajectory
def tokens_of(pl, o):
    with torch.no_grad():
        return pl.prediction_head.encode_images(o["rgbs"][:, -1] / 2 + 0.5, None)


def both_ways(pl, o, tokens, goal, **kw):
    """compute_trajectory with and without fused_conditioning on the same inputs -> (default, fused, paths)"""
    B = o["mask"].shape[0]
    args = (o["mask"], None, o["pcds"][:, -1], o["instr"].expand(B, -1, -1).contiguous(), o["gripper"][:, -1, :7], goal)
    ref = pl.compute_trajectory(*args, visual_tokens=tokens, **kw)
    p0 = pl.last_sampler_path
    got = pl.compute_trajectory(*args, visual_tokens=tokens, fused_conditioning=True, **kw)
    return ref, got, (p0, pl.last_sampler_path)


def candidate_noise(dev, B, G, Ln, K, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, G, Ln, 9, generator=g).to(dev), torch.randn(K, B, G, Ln, 9, generator=g).to(dev)


def test_fused_conditioning_equals_the_default_call(models, dev):
    kp, pl, instr = models
    # L = 16, one trajectory per scene, the full chain truncated to 3 steps
    o = observation(dev, 11, 2, 16)
    o["instr"] = instr
    tokens = tokens_of(pl, o)
    goal = o["gt_action"][:, -1]                                       # (B, 8) rows, read at 7 channels
    ref, got, paths = both_ways(pl, o, tokens, goal[..., :7], init_noise=o["init_noise"], step_noise=o["step_noise"], n_steps=3)
    assert paths[0] == paths[1] == "persistent (a3d_dn_persist)" and abort_word(pl) == 0
    assert torch.isfinite(ref).all() and torch.equal(got, ref)
    # the goal is not part of the conditioning with use_goal_at_test=False
    pl._use_goal_at_test = False
    try:
        ref2, got2, paths = both_ways(pl, o, tokens, goal[..., :7], init_noise=o["init_noise"], step_noise=o["step_noise"], n_steps=3)
    finally:
        pl._use_goal_at_test = True
    assert paths[0] == paths[1] and torch.equal(got2, ref2) and not torch.equal(ref2, ref)
    # L = 50, two candidates per scene on the grouped persistent sampler, DDIM eta = 0 with K = 4
    o = observation(dev, 12, 2, 50, pads=[7, 0])
    o["instr"] = instr
    tokens = tokens_of(pl, o)
    init, _ = candidate_noise(dev, 2, 2, 50, 4)
    ref, got, paths = both_ways(pl, o, tokens, o["gt_action"][:, -1, :7], init_noise=init, num_samples=2, num_inference_steps=4,
                                scheduler="ddim", eta=0.0)
    assert paths[0] == paths[1] == "persistent (a3d_dn_persist_group)" and abort_word(pl) == 0
    assert ref.shape == (2, 2, 50, 7) and torch.isfinite(ref).all() and torch.equal(got, ref)
    # the flag is part of the graph key: a replayed default call followed by a fused one rebuilds, and both equal the eager result
    o = observation(dev, 11, 2, 16)
    o["instr"] = instr
    tokens = tokens_of(pl, o)
    kw = dict(init_noise=o["init_noise"], num_inference_steps=4, scheduler="ddim")
    eager, _, _ = both_ways(pl, o, tokens, goal[..., :7], **kw)
    ref, got, _ = both_ways(pl, o, tokens, goal[..., :7], use_graph=True, **kw)
    assert "fused_conditioning" in repr(pl._graph["key"]) and torch.equal(ref, eager) and torch.equal(got, eager)
    pl._graph = None


def _fallback_child():
    """A3D_DN_PERSIST=0 (read at import): num_samples on the expanded context, with and without the fused conditioning"""
    import importlib
    root = os.path.dirname(HERE)
    if root not in sys.path:
        sys.path.insert(0, root)
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    assert a3d.diffusion.DN_PERSIST is False
    pl = make_planner(a3d, dev)
    o = observation(dev, 13, 2, 16)
    g = torch.Generator().manual_seed(3)
    o["instr"] = torch.randn(1, 53, 512, generator=g).to(dev)
    tokens = torch.randn(2, NCAM * (IMG // 4) ** 2, E, generator=g).to(dev)
    init, step = candidate_noise(dev, 2, 3, 16, 4)
    ref, got, paths = both_ways(pl, o, tokens, o["gt_action"][:, -1, :7], init_noise=init, step_noise=step, num_samples=3,
                                num_inference_steps=4, scheduler="ddpm")
    assert paths[0] == paths[1] == "per-phase fused launches", paths
    assert ref.shape == (2, 3, 16, 7) and torch.isfinite(ref).all() and torch.equal(got, ref)
    print("fallback-child ok")


def test_fused_conditioning_on_the_expanded_fallback_in_a_fresh_process(dev):
    env = dict(os.environ)
    env["A3D_DN_PERSIST"] = "0"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "fallback-child"], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "fallback-child ok" in p.stdout


# ------------------------------------------------------------------------------------------------ 3: predict == by hand
def test_predict_equals_the_hand_written_sequence(a3d, models, dev):
    kp, pl, instr = models
    o = observation(dev, 21, 2, 16)
    kw = dict(init_noise=o["init_noise"], step_noise=o["step_noise"], n_steps=3)
    set_rng(kp)
    action, traj, pred = by_hand(kp, pl, instr, o, **kw)
    rng_after = kp._rng_state.clone()
    assert not torch.equal(rng_after.cpu(), torch.tensor(RNG0)) and action.shape == (2, 8) and traj.shape == (2, 16, 7) and torch.isfinite(traj).all()
    for share, passes in ((False, 2), ("auto", 1), (True, 1)):
        act = a3d.Actioner(kp, pl, predict_keypose=True, predict_trajectory=True, share_backbone=share)
        act.set_instruction(instr)
        set_rng(kp)
        out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], **kw)
        assert sorted(out) == ["action", "attention", "trajectory"] and out["attention"] == {}
        assert act.last_backbone_passes == passes and act.shares_backbone == (share is not False)
        assert torch.equal(out["action"], action), share
        assert torch.equal(out["trajectory"], traj), share
        for a, b in zip(act.last_keypose_output["position_pyramid"], pred["position_pyramid"]):
            assert torch.equal(a, b), share
        assert torch.equal(kp._rng_state, rng_after)                            # the draws of one eager forward
    # the unfused seam gives the same bits
    act = a3d.Actioner(kp, pl, predict_trajectory=True, share_backbone=False, fused_conditioning=False)
    act.set_instruction(instr)
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], **kw)
    assert torch.equal(out["action"], action) and torch.equal(out["trajectory"], traj)
    # a planner with another backbone: "auto" falls back to two passes, with the same result as by hand
    other = make_planner(a3d, dev, seed=1)
    act = a3d.Actioner(kp, other, predict_trajectory=True)
    act.set_instruction(instr)
    set_rng(kp)
    a2, t2, _ = by_hand(kp, other, instr, o, **kw)
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], **kw)
    assert act.last_backbone_passes == 2 and torch.equal(out["action"], a2) and torch.equal(out["trajectory"], t2)
    assert not torch.equal(t2, traj)
    # predict_keypose=False: the action is gt_action's last row and the goal its first 7 channels
    act = a3d.Actioner(kp, pl, predict_keypose=False, predict_trajectory=True)
    act.set_instruction(instr)
    before = kp._rng_state.clone()
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], o["gt_action"], o["mask"], **kw)
    rgb = o["rgbs"][:, -1] / 2 + 0.5
    ins = instr.expand(2, -1, -1).contiguous()
    want = pl.compute_trajectory(o["mask"], rgb, o["pcds"][:, -1], ins, o["gripper"][:, -1, :7], o["gt_action"][:, -1, :7], **kw)
    assert torch.equal(out["action"], o["gt_action"][:, -1]) and torch.equal(out["trajectory"], want)
    assert act.last_backbone_passes == 1 and torch.equal(kp._rng_state, before)
    # predict_trajectory=False: the keypose alone
    act = a3d.Actioner(kp, None, predict_keypose=True, predict_trajectory=False)
    act.set_instruction(instr)
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"])
    assert out["trajectory"] is None and torch.equal(out["action"], action) and act.last_backbone_passes == 1


# ------------------------------------------------------------------------------------------------ 4: graph replay
def test_graph_replay_equals_an_eager_twin(a3d, models, dev):
    kp, pl, instr = models
    kp2 = make_keypose(a3d, dev)                                          # same seeds: identical weights
    pl2 = make_planner(a3d, dev, backbone_of=kp2)
    assert all(torch.equal(a, b) for a, b in zip(list(kp.parameters()) + list(pl.parameters()), list(kp2.parameters()) + list(pl2.parameters())))
    pl._graph = pl2._graph = None
    graphed = a3d.Actioner(kp, pl, predict_trajectory=True)
    eager = a3d.Actioner(kp2, pl2, predict_trajectory=True)
    for a in (graphed, eager):
        a.set_instruction(instr)
    set_rng(kp)
    set_rng(kp2)
    graphs = []
    for i, (B, seed) in enumerate([(2, 31), (2, 32), (2, 33), (1, 34), (1, 35)]):
        o = observation(dev, seed, B, 16, pads=[i % 4, 0][:B])
        kw = dict(init_noise=o["init_noise"], step_noise=o["step_noise"][:4].contiguous(), num_inference_steps=4, scheduler="ddpm")
        want = eager.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], **kw)
        got = graphed.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], use_graph=True, **kw)
        assert graphed.last_backbone_passes == 1
        assert torch.equal(got["action"], want["action"]), i
        assert torch.equal(got["trajectory"], want["trajectory"]), i
        assert torch.equal(kp._rng_state, kp2._rng_state), i                  # a replay draws what the eager call draws
        assert pl.last_sampler_path == pl2.last_sampler_path == "persistent (a3d_dn_persist_sched)"
        assert abort_word(pl) == 0
        graphs.append((graphed._graph["g"], pl._graph["g"]))
    # three calls at B = 2 replay ONE graph each for the keypose half and the sampling loop; B = 1 rebuilds both
    assert graphs[0][0] is graphs[1][0] is graphs[2][0] and graphs[0][1] is graphs[1][1] is graphs[2][1]
    assert graphs[3][0] is not graphs[2][0] and graphs[3][1] is not graphs[2][1] and graphs[4][0] is graphs[3][0]
    pl._graph = None
    graphed._graph = None


# ------------------------------------------------------------------------------------------------ 5: candidates, few steps
def test_candidates_and_few_step_options_through_the_seam(a3d, models, dev):
    """num_samples / num_inference_steps / scheduler reach compute_trajectory unchanged: (B, 3, L, action_dim) -- the last
    dimension is the pose width the planner is given, 7 here (8 with action_dim = 8 rows)."""
    kp, pl, instr = models
    B, G, Ln = 2, 3, 16
    o = observation(dev, 41, B, Ln)
    init, _ = candidate_noise(dev, B, G, Ln, 4)
    act = a3d.Actioner(kp, pl, predict_trajectory=True)
    act.set_instruction(instr)
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], num_samples=G, num_inference_steps=4, scheduler="ddim",
                      init_noise=init)
    assert out["trajectory"].shape == (B, G, Ln, 7) and torch.isfinite(out["trajectory"]).all()
    assert pl.last_sampler_path == "persistent (a3d_dn_persist_group)" and abort_word(pl) == 0
    rgb = o["rgbs"][:, -1] / 2 + 0.5
    want = pl.compute_trajectory(o["mask"], rgb, o["pcds"][:, -1], instr.expand(B, -1, -1).contiguous(), o["gripper"][:, -1, :7],
                                 out["action"][..., :7], num_samples=G, num_inference_steps=4, scheduler="ddim", init_noise=init)
    assert torch.equal(out["trajectory"], want)
    assert not torch.equal(out["trajectory"][:, 0], out["trajectory"][:, 1])


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "fallback-child":
    torch.backends.cudnn.deterministic = True
    _fallback_child()
