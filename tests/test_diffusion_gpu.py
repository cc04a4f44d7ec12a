"""End-to-end parity of the HIP trajectory-diffusion path against golden outputs of the REFERENCE (tests/golden/diffusion.pt):
denoiser forward, training loss + gradients with injected noise/timesteps, and the full 100-step sampling loop with
injected noise (eager and hipGraph-captured).  The DDPM scheduler itself is third-party (parity unpinned)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import common as C  # noqa: E402
from test_oracle_golden import _diffusion_params, load  # noqa: E402

pytestmark = pytest.mark.gpu


def scale_close(name, got, ref, tol=1e-3, floor=1.0):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs().max().item()
    scale = max(floor, ref.abs().max().item())
    print(f"[parity] {name}: max_abs_err={err:.3e} ref_absmax={ref.abs().max().item():.3e} rel_to_scale={err / scale:.2e}")
    assert torch.isfinite(got).all(), name
    assert err <= tol * scale, f"{name}: max err {err:.3e} > {tol} * {scale:.3e}"


@pytest.fixture(scope="module")
def setup(a3d, dev):
    r = load("diffusion.pt")
    cfg = r["cfg"]
    m = a3d.DiffusionPlanner(embedding_dim=cfg["E"], output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100,
                             dropout=0.0)          # the reference goldens were recorded with dropout disabled
    res = m.load_state_dict(_diffusion_params(r), strict=False)
    assert not res.unexpected_keys
    assert all(".backbone." in k or "feature_pyramid" in k for k in res.missing_keys), res.missing_keys
    m.to(dev)
    inp = C.trajectory_inputs(r["seed"], cfg["B"], cfg["L"], cfg["ncam"], cfg["E"], pad_last=cfg["pad_last"])
    inp = {k: v.to(dev) for k, v in inp.items()}
    inp["tokens"] = C.tokens_from_maps(inp["fmap"])
    return r, cfg, m, inp


def test_denoiser_forward(setup, dev):
    r, cfg, m, inp = setup
    m.eval()
    head = m.prediction_head
    with torch.no_grad():
        tokens, ctx_xyz, cg, gg = m._prepare(None, inp["pcd"], inp["curr_gripper"], inp["goal_gripper"], inp["tokens"])
        scale_close("curr gripper 9d", cg, r["conv"]["curr9"], 1e-5)
        ctx, cxyz, instr = head.encode_context(tokens, ctx_xyz, inp["instr"], cg, gg)
        pred = head.forward_tokens(r["head_in"].to(dev), inp["mask"], inp["timesteps"], ctx, cxyz, instr)
    scale_close("denoiser forward", pred, r["head_out"])


def test_training_loss_and_grads(setup, dev):
    r, cfg, m, inp = setup
    m.train()
    for p in m.parameters():
        p.grad = None
    loss = m(inp["trajectory"], inp["mask"], None, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"],
             noise=inp["noise"], timesteps=inp["timesteps"], visual_tokens=inp["tokens"])
    scale_close("train loss", loss, r["train_loss"], 1e-3)
    loss.backward()
    named = dict(m.named_parameters())
    for n, gref in r["grads"].items():
        scale_close("grad " + n, named[n].grad, gref, 1.5e-3, floor=1e-3)      # observed <= 1.1e-3 of scale
    with_grad = set(r["manifest"]["with_grad"])
    for n, p in named.items():
        if ".backbone." in n or "feature_pyramid" in n:
            continue
        if n in with_grad:
            assert p.grad is not None, f"{n} should receive a gradient"
            nr = r["grad_norms"][n]
            assert abs(p.grad.norm().item() - nr) <= 3e-3 * nr + 1e-4, f"grad norm {n}: {p.grad.norm().item()} vs {nr}"
        else:
            assert p.grad is None or p.grad.abs().max().item() == 0.0, f"{n} must not receive a gradient (SURVEY G12)"


def test_sampling_loop_100_steps(setup, dev):
    r, cfg, m, inp = setup
    m.eval()
    final, trace = m.compute_trajectory(inp["mask"], None, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"],
                                        init_noise=inp["init_noise"], step_noise=inp["step_noise"], visual_tokens=inp["tokens"],
                                        return_trace=True)
    for t, ref in r["sample_trace_inputs"].items():
        if t == 99:
            continue
        scale_close(f"state before t={t}", trace[98 - t], ref, 2e-4)           # observed 1e-5 after 100 steps
    scale_close("sampled xyz", final[..., :3], r["sample_final"][..., :3], 2e-4)
    q, qr = final[..., 3:].cpu(), r["sample_final"][..., 3:]
    sign = torch.sign((q * qr).sum(-1, keepdim=True))
    scale_close("sampled quaternion", q * sign, qr, 2e-4)
    # hipGraph-captured loop == eager loop (same injected noise), twice (capture + replay)
    for rep in range(2):
        g_final = m.compute_trajectory(inp["mask"], None, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"],
                                       init_noise=inp["init_noise"], step_noise=inp["step_noise"], visual_tokens=inp["tokens"],
                                       use_graph=True)
        assert torch.allclose(g_final, final, atol=1e-5), f"graph replay {rep} differs from the eager loop"


def test_cfg3_full_shape_graph_vs_oracle(a3d, dev):
    """BASELINE.json configs[2] at its full shape: batch 64, horizon 16, 3 cameras (S = 3 * 1024 + 2 context tokens),
    100 denoise steps, hipGraph-captured -- against the CPU oracle's 100-step loop on a sub-batch (the samples of a
    trajectory batch never interact, so two of the 64 rows pin the whole batch's arithmetic)."""
    import numpy as np
    from oracle import diffusion as OD
    from oracle import sampling as OS
    r = load("diffusion.pt")
    E, B, Ln, ncam, H = 120, 64, 16, 3, 8
    m = a3d.DiffusionPlanner(embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100)
    P = _diffusion_params(r)
    m.load_state_dict(P, strict=False)
    m.to(dev).eval()
    inp = C.trajectory_inputs(91, B, Ln, ncam, E, pad_last=3)
    tokens = C.tokens_from_maps(inp["fmap"])
    d = {k: v.to(dev) for k, v in inp.items()}
    outs = []
    for rep in range(2):                                   # capture + replay
        outs.append(m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"],
                                         init_noise=d["init_noise"], step_noise=d["step_noise"], visual_tokens=tokens.to(dev),
                                         use_graph=True).cpu())
    assert torch.equal(outs[0], outs[1]), "graph replay differs from the captured run (max abs diff %.3e)" % (outs[0] - outs[1]).abs().max().item()
    eager = m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"],
                                 init_noise=d["init_noise"], step_noise=d["step_noise"], visual_tokens=tokens.to(dev)).cpu()
    assert torch.allclose(outs[0], eager, atol=1e-5), "graph differs from the eager loop"
    assert torch.isfinite(outs[0]).all()
    sub = [3, 40]                                          # one unpadded and one padded trajectory
    bounds = torch.from_numpy(C.DIFFUSION_BOUNDS)
    pcdn = OD.normalize_pos(inp["pcd"][sub].permute(0, 1, 3, 4, 2), bounds).permute(0, 1, 4, 2, 3).contiguous()
    cxyz_n = torch.from_numpy(OS.pcd_downsample(pcdn.numpy(), 8))
    with torch.no_grad():
        ofinal, _ = OD.compute_trajectory(P, OD.DDPMSchedules(100), inp["mask"][sub], tokens[sub], None, inp["instr"][sub],
                                          inp["curr_gripper"][sub], inp["goal_gripper"][sub], bounds, inp["init_noise"][sub],
                                          inp["step_noise"][:, sub], H, ctx_xyz_norm=cxyz_n)
    got = outs[0][sub]
    scale_close("cfg3 sampled xyz", got[..., :3], ofinal[..., :3], 3e-4)
    sign = torch.sign((got[..., 3:] * ofinal[..., 3:]).sum(-1, keepdim=True))
    scale_close("cfg3 sampled quaternion", got[..., 3:] * sign, ofinal[..., 3:], 3e-4)


def test_fused_denoise_step_equals_op_by_op_path(setup, dev):
    """csrc/denoise.hip (18 launches per network evaluation: head, per-layer cross + rest, tail; fp32 K cache) against the
    op-by-op path (AdaLN / projection / RoPE-split / attention / LayerNorm kernels, three-part bf16 K cache), state by state
    over the first steps and at the end of the full loop, with padded trajectories and goal in-painting."""
    r, cfg, m, inp = setup
    m.eval()
    kw = dict(init_noise=inp["init_noise"], step_noise=inp["step_noise"], visual_tokens=inp["tokens"], return_trace=True)
    args = (inp["mask"], None, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"])
    fa, ta = m.compute_trajectory(*args, fused=True, **kw)
    fb, tb = m.compute_trajectory(*args, fused=False, **kw)
    for i in (0, 1, 2, 50, 99):
        scale_close(f"fused vs op-by-op state after step {i}", ta[i], tb[i], 2e-5)
    scale_close("fused vs op-by-op final pose", fa, fb, 2e-5)


@pytest.mark.parametrize("B,Ln,n_steps", [(3, 16, 100), (64, 16, 12), (5, 7, 9)])
def test_persistent_sampler_equals_per_phase_launches(a3d, dev, B, Ln, n_steps):
    """a3d_dn_persist (the whole denoise loop as ONE launch: one workgroup per trajectory walks head / layers / tail across the
    steps, the other CUs stream the cached context for whichever (sample, layer) is ready) against the per-phase launches
    (a3d_dn_head / a3d_dn_cross / a3d_dn_rest / a3d_dn_tail, 18 per step): same arithmetic up to the summation order of the
    query projection and of the key-split combine.  Full loop in one launch, the traced variant (one step per launch) state by
    state, the abort word stays zero, and a second launch reproduces the first bit for bit."""
    r = load("diffusion.pt")
    E, ncam = 120, 3
    m = a3d.DiffusionPlanner(embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100)
    m.load_state_dict(_diffusion_params(r), strict=False)
    m.to(dev).eval()
    inp = C.trajectory_inputs(91, B, Ln, ncam, E, pad_last=3 if Ln > 8 else 1)
    tokens = C.tokens_from_maps(inp["fmap"]).to(dev)
    d = {k: v.to(dev) for k, v in inp.items()}
    D = a3d.diffusion

    def run(persist, **kw):
        keep = D.DN_PERSIST
        D.DN_PERSIST = persist
        try:
            out = m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], init_noise=d["init_noise"],
                                       step_noise=d["step_noise"], visual_tokens=tokens, n_steps=n_steps, **kw)
            torch.cuda.synchronize()
            if persist:
                ps = m.prediction_head._last_persist
                assert ps is not None and int(ps["sync"][2].item()) == 0, "the persistent sampler gave up waiting"
            return out
        finally:
            D.DN_PERSIST = keep

    ref, ref_trace = run(False, return_trace=True)
    got = run(True)
    scale_close(f"persistent vs per-phase, {n_steps} steps in one launch", got, ref, 5e-5)
    assert torch.equal(run(True), got), "the persistent sampler is not run-to-run deterministic"
    got_t, trace = run(True, return_trace=True)
    for i in sorted(set([0, 1, n_steps // 2, n_steps - 1])):
        scale_close(f"persistent (traced) vs per-phase state after step {i}", trace[i], ref_trace[i], 5e-5)
    scale_close("persistent traced vs one launch", got_t, got, 1e-6)


@pytest.mark.parametrize("E,H,Ln", [(60, 4, 16), (30, 2, 16), (90, 6, 16), (60, 4, 20)])
def test_other_head_counts_three_paths_agree(a3d, dev, E, H, Ln):
    """Head counts no trained weights exist for (H = 4, 2, 6: the persistent sampler splits a unit's keys over nsub = 8 / H = 2, 4, 1
    waves per head; E = 30 / 90 take the scalar weight loader of the dense layers) on a randomly initialised planner, B = 3, 6 steps:
    the persistent sampler, the per-phase launches and the op-by-op path agree state by state at the tolerances this file uses for
    E = 120 (2e-5 fused against op-by-op, 5e-5 persistent against per-phase), the abort word stays zero and a second persistent launch
    gives the same bits.  Ln = 20 is two row tiles: the per-phase kernels serve one tile only, so the persistent sampler is held against
    the op-by-op path alone."""
    B, ncam, n_steps = 3, 2, 6
    torch.manual_seed(1000 + E + Ln)
    m = a3d.DiffusionPlanner(embedding_dim=E, num_attn_heads=H, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100)
    m.to(dev).eval()
    inp = C.trajectory_inputs(95, B, Ln, ncam, E, pad_last=3)
    tokens = C.tokens_from_maps(inp["fmap"]).to(dev)
    d = {k: v.to(dev) for k, v in inp.items()}
    D = a3d.diffusion
    assert a3d.lib.load().a3d_dn_persist_splits(H, 1) == (8 // H if 8 % H == 0 else 1)

    def run(persist, **kw):
        keep = D.DN_PERSIST
        D.DN_PERSIST = persist
        head = m.prediction_head
        head._last_persist = None
        try:
            out = m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], init_noise=d["init_noise"],
                                       step_noise=d["step_noise"], visual_tokens=tokens, n_steps=n_steps, **kw)
            torch.cuda.synchronize()
            if persist and kw.get("fused", True):
                ps = head._last_persist
                assert ps is not None and int(ps["sync"][2].item()) == 0, "not on the persistent sampler / it gave up waiting"
            return out
        finally:
            D.DN_PERSIST = keep

    tag = f"E={E} H={H} Ln={Ln}"
    _, t_ops = run(False, fused=False, return_trace=True)
    got = run(True)
    assert torch.isfinite(got).all()
    assert torch.equal(run(True), got), "the persistent sampler is not run-to-run deterministic"
    got_t, t_pers = run(True, return_trace=True)
    scale_close(f"{tag}: persistent traced vs one launch", got_t, got, 1e-6)
    if Ln <= 16:
        _, t_phase = run(False, return_trace=True)
        for i in range(n_steps):
            scale_close(f"{tag}: per-phase fused vs op-by-op state after step {i}", t_phase[i], t_ops[i], 2e-5)
            scale_close(f"{tag}: persistent vs per-phase state after step {i}", t_pers[i], t_phase[i], 5e-5)
    else:
        for i in range(n_steps):
            scale_close(f"{tag}: persistent (two row tiles) vs op-by-op state after step {i}", t_pers[i], t_ops[i], 2e-5)


def test_cfg4_trajectory_half_per_gpu_shape_vs_oracle(a3d, dev):
    """BASELINE.json configs[3] (joint keypose + trajectory-diffusion training, DP batch 128 over 8 GPUs), trajectory half at its
    PER-GPU shape: 16 trajectories of horizon 50 (scripts/train_trajectory.sh), 3 cameras (S = 3074), E = 120 -- training loss and
    gradients of the HIP step against the CPU oracle's planner loss (diffusion_model.py:253-324) on the same noise / timesteps,
    dropout off (the Philox dropout has its own parity tests).  The keypose half: test_act3d_gpu.py [cfg4-keypose]."""
    from oracle import diffusion as OD
    from oracle import sampling as OS
    r = load("diffusion.pt")
    E, B, Ln, ncam, H = 120, 16, 50, 3, 8
    m = a3d.DiffusionPlanner(embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100, dropout=0.0)
    P = _diffusion_params(r)
    m.load_state_dict(P, strict=False)
    m.to(dev).train()
    inp = C.trajectory_inputs(95, B, Ln, ncam, E, pad_last=6)
    tokens = C.tokens_from_maps(inp["fmap"])
    g = torch.Generator().manual_seed(95)
    noise = torch.randn(B, Ln, 9, generator=g)
    timesteps = torch.randint(0, 100, (B,), generator=g)
    d = {k: v.to(dev) for k, v in inp.items()}
    for p in m.parameters():
        p.grad = None
    # the device's ReLU masks, per site (= qualified name of the MLP's first Linear, the oracle's site names) in call order
    O_ = a3d.ops
    site_of = {id(mod): name for name, mod in m.named_modules()}
    dev_masks = {}
    mlp_orig = O_.mlp

    def mlp_recording(x, lin1, lin2, *a_, **k_):
        h = O_.linear2d(x.detach().reshape(-1, x.shape[-1]).contiguous(), lin1.weight, lin1.bias, act=1)   # the kernel MLPFn runs
        dev_masks.setdefault(site_of[id(lin1)], []).append((h > 0).cpu())
        return mlp_orig(x, lin1, lin2, *a_, **k_)
    O_.mlp = mlp_recording
    try:
        loss, pred, gt = m(d["trajectory"], d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], noise=noise.to(dev),
                           timesteps=timesteps.to(dev), visual_tokens=tokens.to(dev), return_pred=True)
    finally:
        O_.mlp = mlp_orig
    # the oracle on leaf copies of the same parameters, TWICE: in fp32 (the reference's arithmetic) and lifted to float64 (the same
    # function, exact for this purpose: oracle.blocks.LIFT)
    from oracle import blocks as OB
    bounds = torch.from_numpy(C.DIFFUSION_BOUNDS)
    pcdn = OD.normalize_pos(inp["pcd"].permute(0, 1, 3, 4, 2), bounds).permute(0, 1, 4, 2, 3).contiguous()
    cxyz_n = torch.from_numpy(OS.pcd_downsample(pcdn.numpy(), 8))

    def oracle(dt, masks=None):
        OB.LIFT = None if dt == torch.float32 else dt
        OB.RELU_MASKS = None if masks is None else {k: list(v) for k, v in masks.items()}
        OB.RELU_DIFFS = [] if masks is not None else None
        try:
            leaf, Po = {}, {}
            for n, t in P.items():
                if id(t) not in leaf:
                    leaf[id(t)] = (t.to(dt) if t.dtype.is_floating_point else t).clone().requires_grad_(t.dtype.is_floating_point)
                Po[n] = leaf[id(t)]
            cv = lambda x: x.to(dt) if x.dtype.is_floating_point else x
            ol, op, og = OD.planner_loss(Po, OD.DDPMSchedules(100), cv(inp["trajectory"]), inp["mask"], cv(tokens), None, cv(inp["instr"]),
                                         cv(inp["curr_gripper"]), cv(inp["goal_gripper"]), cv(bounds), cv(noise), timesteps, H,
                                         ctx_xyz_norm=cv(cxyz_n))
            return Po, ol, op, og, OB.RELU_DIFFS
        finally:
            OB.LIFT = None
            OB.RELU_MASKS = OB.RELU_DIFFS = None

    # forward parity against the oracle as it is (its own ReLU branches)
    _, oloss, opred, ogt, _ = oracle(torch.float32)
    scale_close("cfg4 trajectory-half loss", loss, oloss.detach(), 1e-3)
    scale_close("cfg4 trajectory-half prediction", pred, opred.detach(), 5e-4)
    # gradient parity ON THE DEVICE'S BRANCH of the piecewise-linear network: both oracle runs take the device's ReLU masks
    Po, _, opred, ogt, diffs32 = oracle(torch.float32, dev_masks)
    P64, l64, p64, g64, diffs64 = oracle(torch.float64, dev_masks)
    scale_close("cfg4 trajectory-half prediction vs the float64 oracle", pred, p64.detach(), 5e-4)
    nflip = sum(n for _, n, _, _ in diffs64)
    print(f"[parity] cfg4 trajectory half: the device's ReLU masks differ from the float64 oracle's own sign pattern on {nflip} of "
          f"{sum(mk.numel() for v in dev_masks.values() for mk in v)} units; "
          + "; ".join(f"{site}: {n} unit(s), largest |pre-activation| {mx:.1e} (layer scale {sc:.1e})" for site, n, mx, sc in diffs64 if n))
    assert all(mx <= 1e-4 * max(sc, 1.0) for _, n, mx, sc in diffs64 if n), "a ReLU unit far from its kink has the wrong sign on the device"
    # Gradients.  Round 5 held them only in aggregate and blamed the L1 loss's kinks (a residual within rounding of zero flips
    # sign(pred - gt)); the round-5 review asked for evidence.  Round 6 has it, and the L1 explanation was WRONG: all runs
    # back-propagate the loss LINEARISED AT THE FLOAT64 ORACLE'S SIGN PATTERN (no L1 kink can act) and no residual is near a kink
    # (count below).  The kinks that do act are the ReLUs of the FFNs: profiles/cfg4_grad_debug.py followed the gradient of every
    # sub-block output down the stack (gpurun_out r06, profiles/r06_cfg4_grad_chain.txt) -- exact (7e-6) into the FFN block of
    # traj_attention layer 3, 2e-3 out of it, ~1e-3 in everything upstream: ONE hidden unit of ONE token whose pre-activation is
    # within rounding of zero sits on the other side of its kink on the device (count and magnitudes printed above), and the
    # discrete gradient step propagates to every earlier layer (the fp32 ORACLE flips units of its own: against float64 it is up to
    # 6e-3 of scale off on the same tensors when each run keeps its own branch).  Evaluated on the device's branch, every
    # parameter gradient of the device is held ELEMENT-WISE against the float64 oracle to 2e-4 of the tensor's scale -- five times
    # inside north_star's 1e-3 (observed 1.6e-5; the fp32 oracle itself: 2.3e-5).
    resid = (p64 - g64).detach()
    w = torch.empty_like(resid)
    w[..., :3] = 100.0 / resid[..., :3].numel()
    w[..., 3:] = 10.0 / resid[..., 3:].numel()
    up = torch.sign(resid) * w
    near = int((resid.abs() < 1e-6).sum())
    flipped = int((torch.sign((pred.detach().cpu().double() - gt.detach().cpu().double())) != torch.sign(resid)).sum())
    print(f"[parity] cfg4 trajectory half: {near} of {resid.numel()} residuals within 1e-6 of the L1 kink; the device's own sign pattern "
          f"differs from the float64 oracle's in {flipped} entries")
    (pred * up.float().to(dev)).sum().backward()
    (opred * up.float()).sum().backward()
    (p64 * up).sum().backward()
    named = dict(m.named_parameters())
    rows = []
    for n, p in named.items():
        if n in P64 and P64[n].grad is not None and p.grad is not None and "backbone" not in n:
            gx = P64[n].grad
            sc = gx.abs().max().item()
            if sc < 1e-7:
                continue
            e_dev = (p.grad.detach().double().cpu() - gx).abs().max().item() / sc
            e_o32 = (Po[n].grad.double() - gx).abs().max().item() / sc
            l2_dev = ((p.grad.detach().double().cpu() - gx).norm() / gx.norm()).item()
            rows.append((e_dev, e_o32, l2_dev, n))
    rows.sort(reverse=True)
    worst_o32 = max(r_[1] for r_ in rows)
    med = sorted(r_[2] for r_ in rows)[len(rows) // 2]
    print(f"[parity] cfg4 trajectory half, {len(rows)} parameter gradients against the float64 oracle: device worst {rows[0][0]:.2e} of scale "
          f"({rows[0][3]}; the fp32 oracle on the same tensor: {rows[0][1]:.2e}); fp32 oracle worst {worst_o32:.2e}; device median "
          f"relative L2 {med:.2e}; {sum(1 for r_ in rows if r_[0] > 1e-3)} tensors above 1e-3 (fp32 oracle: {sum(1 for r_ in rows if r_[1] > 1e-3)})")
    for e_dev, e_o32, l2_dev, n in rows[:6]:
        print(f"[parity] cfg4 grad {n}: device {e_dev:.2e} / fp32 oracle {e_o32:.2e} of scale vs float64; device relative L2 {l2_dev:.2e}")
    assert len(rows) >= 40, "too few gradient tensors were comparable (parameter names changed?)"
    # observed (round 6): device worst 1.6e-5 of scale, fp32 oracle worst 2.3e-5, device median relative L2 4.9e-6
    bad = [(n, e_dev, e_o32) for e_dev, e_o32, _, n in rows if e_dev > max(2e-4, 3.0 * e_o32)]
    assert not bad, bad
    assert med <= 1e-4, med


def test_persistent_sampler_script_horizon_50_vs_oracle(a3d, dev):
    """The horizon the reference deploys (interpolation_length = 50: scripts/train_trajectory.sh:7-8, online_evaluation/eval.sh:17)
    on the fused path: four 16-step row tiles per trajectory, one sample-role workgroup each, self-attention keys / values exchanged
    between the tiles of a trajectory.  100 steps in one launch with a padded trajectory, against (a) the op-by-op path (separate
    kernels, three-part bf16 K cache) on the whole batch and (b) the CPU oracle's loop on two of the samples."""
    from oracle import diffusion as OD
    from oracle import sampling as OS
    r = load("diffusion.pt")
    E, B, Ln, ncam, H = 120, 6, 50, 3, 8
    m = a3d.DiffusionPlanner(embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100)
    P = _diffusion_params(r)
    m.load_state_dict(P, strict=False)
    m.to(dev).eval()
    inp = C.trajectory_inputs(93, B, Ln, ncam, E, pad_last=7)
    tokens = C.tokens_from_maps(inp["fmap"])
    d = {k: v.to(dev) for k, v in inp.items()}
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
    kw = dict(init_noise=d["init_noise"], step_noise=d["step_noise"], visual_tokens=tokens.to(dev))
    got = m.compute_trajectory(*args, **kw)
    torch.cuda.synchronize()
    ps = m.prediction_head._last_persist
    assert ps is not None and ps["kvx"] is not None and int(ps["sync"][2].item()) == 0, "not on the persistent sampler / it gave up waiting"
    assert torch.isfinite(got).all()
    ref = m.compute_trajectory(*args, fused=False, **kw)
    scale_close("L = 50 persistent sampler vs op-by-op path (100 steps)", got, ref, 1e-4)
    g2 = m.compute_trajectory(*args, use_graph=True, **kw)
    g3 = m.compute_trajectory(*args, use_graph=True, **kw)
    assert torch.equal(g2, got) and torch.equal(g3, got), "graph capture / replay of the L = 50 sampler differs from the eager launch"
    sub = [1, 4]                                           # one unpadded and one padded trajectory (pad_last pads the second half)
    bounds = torch.from_numpy(C.DIFFUSION_BOUNDS)
    pcdn = OD.normalize_pos(inp["pcd"][sub].permute(0, 1, 3, 4, 2), bounds).permute(0, 1, 4, 2, 3).contiguous()
    cxyz_n = torch.from_numpy(OS.pcd_downsample(pcdn.numpy(), 8))
    with torch.no_grad():
        ofinal, _ = OD.compute_trajectory(P, OD.DDPMSchedules(100), inp["mask"][sub], tokens[sub], None, inp["instr"][sub],
                                          inp["curr_gripper"][sub], inp["goal_gripper"][sub], bounds, inp["init_noise"][sub],
                                          inp["step_noise"][:, sub], H, ctx_xyz_norm=cxyz_n)
    o = got[sub].cpu()
    scale_close("L = 50 sampled xyz vs oracle", o[..., :3], ofinal[..., :3], 3e-4)
    sign = torch.sign((o[..., 3:] * ofinal[..., 3:]).sum(-1, keepdim=True))
    scale_close("L = 50 sampled quaternion vs oracle", o[..., 3:] * sign, ofinal[..., 3:], 3e-4)


def test_multi_round_multi_scale_head_vs_reference(a3d, dev):
    """attn_rounds = 2 x feat_scales_to_use = 2, untied module sets, goal-conditioned (diffusion_head.py:249-275) against
    tests/golden/diffusion_multi.pt: the four chained predictions, the find_traj_nn neighbourhoods (a3d_traj_nn_topk), the
    training loss summed over all four with its gradients, and the state after 5 sampling steps."""
    from test_oracle_golden import multi_head_inputs
    r = load("diffusion_multi.pt")
    cfg = r["cfg"]
    inp, feats, xyz, P, bounds = multi_head_inputs(r)
    m = a3d.DiffusionPlanner(embedding_dim=cfg["E"], output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, feat_scales_to_use=2, attn_rounds=2,
                             weight_tying=False, gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D",
                             diffusion_timesteps=100, dropout=0.0)
    res = m.load_state_dict(P, strict=False)
    assert not res.unexpected_keys
    assert all(".backbone." in k or "feature_pyramid" in k for k in res.missing_keys), res.missing_keys
    m.to(dev)
    inp = {k: v.to(dev) for k, v in inp.items()}
    toks = [f.to(dev) for f in feats]
    head = m.prediction_head
    # ---- k-NN kernel against the oracle's restatement on the reference's own query (bit-exact sets and order)
    from oracle import sampling as OS
    prev = r["head_outs"][0][..., :3]
    idx_ref, _ = OS.traj_nn_topk(prev.numpy(), xyz[1].numpy(), 64 * cfg["L"])
    idx = a3d.ops.traj_nn_topk(prev.to(dev), xyz[1].to(dev), 64 * cfg["L"])
    assert torch.equal(idx.cpu(), torch.from_numpy(idx_ref))
    # ---- eval forward: the chained predictions
    m.eval()
    with torch.no_grad():
        tokens, ctx_xyz, cg, gg = m._prepare(None, inp["pcd"], inp["curr_gripper"], inp["goal_gripper"], toks)
        for a, b in zip(ctx_xyz, xyz):
            assert torch.equal(a.cpu(), b)
        preds = head.forward_multi(r["head_in"].to(dev), inp["mask"], inp["timesteps"], tokens, ctx_xyz, inp["instr"], cg, gg)
    assert len(preds) == 4
    for i, (p_, ref) in enumerate(zip(preds, r["head_outs"])):
        scale_close(f"prediction {i}", p_, ref)
    # ---- training loss over all four predictions + gradients
    m.train()
    loss = m(inp["trajectory"], inp["mask"], None, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"],
             noise=inp["noise"], timesteps=inp["timesteps"], visual_tokens=toks)
    scale_close("train loss", loss, r["train_loss"], 1e-3)
    loss.backward()
    named = dict(m.named_parameters())
    for n, gref in r["grads"].items():
        scale_close("grad " + n, named[n].grad, gref, 1.5e-3, floor=1e-3)
    # norms of all 900+ gradient tensors (only six are stored in full): 1.5e-3 each, no exceptions (observed worst 1.6e-4 on
    # MI355X, profiles/r03_parity_report.txt; the L1 sign kinks of the four chained predictions that made round 2 allow 5e-3
    # do not show at this fixture's margins once the attention gradients are 1e-5-class)
    dev_rel = {n: abs(named[n].grad.norm().item() - nr) / (nr + 1e-4) for n, nr in r["grad_norms"].items()}
    worst = max(dev_rel, key=dev_rel.get)
    print(f"[parity] relative gradient-norm deviation over {len(dev_rel)} tensors: worst {dev_rel[worst]:.2e} ({worst})")
    assert dev_rel[worst] <= 1.5e-3, (worst, dev_rel[worst])
    # ---- 5 steps of the sampling loop (no K/V cache: the fine-scale context follows the prediction)
    m.eval()
    _, trace = m.compute_trajectory(inp["mask"], None, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"],
                                    init_noise=inp["init_noise"], step_noise=inp["step_noise"], visual_tokens=toks, n_steps=5,
                                    return_trace=True)
    scale_close("state after 5 steps", trace[-1], r["sample_state_after_5_steps"], 1e-3)      # observed 2.4e-7 of scale


def _script_planner(a3d, dev):
    r = load("diffusion.pt")
    m = a3d.DiffusionPlanner(embedding_dim=120, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100)
    m.load_state_dict(_diffusion_params(r), strict=False)
    return m.to(dev).eval()


def test_bf16_fpn_of_the_diffusion_head_close_to_its_fp32_fpn(a3d, dev):
    """DiffusionHead.fpn_dtype = bf16 (round 6: the FPN on the backbone's bf16 maps, channels padded to 128, only the map the head reads
    converted to fp32) against the fp32 FPN on fp32 copies of the SAME bf16 backbone maps: visual tokens within bf16 convolution noise,
    and a training step's loss / FPN gradients close.  (The backbone is a random stand-in, so this is a consistency test of the two
    FPN paths, not a parity test: the FPN is third-party arithmetic)"""
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench_denoise as BD
    m = BD.build_planner(a3d, dev, train=True)
    head = m.prediction_head
    assert head.fpn_dtype == torch.bfloat16 and head.backbone_dtype == torch.bfloat16
    s = BD.synthetic_inputs(2, 8, 2, dev)
    B, ncam = s["rgbs"].shape[:2]
    nnm = importlib.import_module("act3d-chained-diffuser_amd.nn")
    # ONE backbone run feeds both FPN paths: the library's (MIOpen) wide bf16 3x3 convolutions of layers 2 - 4 are not run-to-run
    # reproducible unless torch.backends.cudnn.deterministic is set (profiles/r06_fpn_diag.txt: plain torch shows the same; res1 / res2
    # bit-equal between two runs, res3 off by 0.09, res5 by 1.2 -- the untrained network amplifies a flipped rounding; with the
    # deterministic solvers every map, our kernels included, is bit-equal), which the first version of this test mistook for a 6 %
    # error of the bf16 FPN
    with torch.no_grad():
        feats = nnm.run_frozen_backbone(head.backbone, s["rgbs"].flatten(0, 1), torch.bfloat16, keep_dtype=True, normalize=head.normalize)
    res = {}
    for tag, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        head.fpn_dtype = dt
        m.zero_grad(set_to_none=True)
        toks = head.tokens_from_backbone_maps(feats if dt == torch.bfloat16 else {k: v.float() for k, v in feats.items()}, B, ncam)
        toks = toks if isinstance(toks, torch.Tensor) else toks[0]
        loss = (toks * torch.linspace(-1, 1, toks.shape[-1], device=dev)).square().mean()
        loss.backward()
        res[tag] = (toks.detach().clone(), loss.detach().clone(),
                    {n: p.grad.clone() for n, p in head.feature_pyramid.named_parameters() if p.grad is not None})
    head.fpn_dtype = torch.bfloat16
    (ta, la, ga), (tb, lb, gb) = res["bf16"], res["fp32"]
    assert ta.shape == tb.shape and ta.dtype == torch.float32
    sc = tb.abs().max().item()
    err = (ta - tb).abs().max().item()
    rel = ((ta - tb).norm() / tb.norm()).item()
    print(f"[parity] diffusion head bf16 FPN vs fp32 FPN tokens: max_abs_err={err:.3e} ref_absmax={sc:.3e} relative L2 {rel:.3e}; "
          f"loss {la.item():.6f} vs {lb.item():.6f}")
    # bf16 operands AND bf16 intermediate maps through three top-down levels: 4e-3 relative L2 measured per level
    # (profiles/r06_fpn_diag.txt: 4.0e-3 at res3 for the product path, 4.9e-3 for plain torch autocast without padding / fused kernels)
    assert torch.isfinite(ta).all() and rel <= 1e-2 and err <= 0.03 * sc
    assert abs(la.item() - lb.item()) <= 5e-3 * abs(lb.item())
    assert set(ga) == set(gb)
    for n in sorted(gb):
        e, g_sc = (ga[n] - gb[n]).abs().max().item(), gb[n].abs().max().item()
        print(f"[parity] diffusion head bf16 FPN gradient {n}: err {e:.3e} of scale {g_sc:.3e}")
        assert torch.isfinite(ga[n]).all() and e <= 0.05 * g_sc + 1e-8, (n, e, g_sc)


def test_persistent_sampler_abort_is_visible_in_the_result(a3d, dev):
    """A persistent launch whose workgroups give up waiting (here forced with the A3D_DN_SPIN_LIMIT=0 test hook: any wait longer
    than 128 polls aborts; in the field: fewer free CUs than the grid assumes) must not return a plausible trajectory: the abort
    word is set AND the whole batch comes back NaN (dn_persist_poison_kernel, part of the launch sequence), without the caller
    having asked for a check.  The next launch, with the hook removed, is healthy again."""
    m = _script_planner(a3d, dev)
    B, Ln, ncam, E = 4, 16, 3, 120
    inp = C.trajectory_inputs(95, B, Ln, ncam, E, pad_last=2)
    d = {k: v.to(dev) for k, v in inp.items()}
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
    kw = dict(init_noise=d["init_noise"], step_noise=d["step_noise"], visual_tokens=C.tokens_from_maps(inp["fmap"]).to(dev), n_steps=10)
    good = m.compute_trajectory(*args, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(good).all() and int(m.prediction_head._last_persist["sync"][2].item()) == 0
    os.environ["A3D_DN_SPIN_LIMIT"] = "0"
    try:
        bad = m.compute_trajectory(*args, **kw)
        torch.cuda.synchronize()
        aborted = int(m.prediction_head._last_persist["sync"][2].item())
    finally:
        del os.environ["A3D_DN_SPIN_LIMIT"]
    print(f"[parity] forced abort: abort word {aborted}, NaN entries {int(torch.isnan(bad).sum())} of {bad.numel()}")
    assert aborted != 0, "the test hook did not force an abort (no wait exceeded 128 polls?)"
    # (every pose is poisoned: position and rotation carry NaN; signal_to_pose's quaternion pivot may leave one zero component)
    assert torch.isnan(bad[..., :3]).all() and torch.isnan(bad).any(-1).all(), "an aborted persistent launch returned finite poses"
    again = m.compute_trajectory(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(again, good)


def test_persistent_sampler_stress_every_cu_200_replays(a3d, dev):
    """The occupancy limit of the persistent sampler under repetition: B = 30 trajectories of horizon 50 = 4 row tiles x 2 roles
    = 240 sample-role workgroups + 16 streamers = every CU of the device, replayed 200 times from a captured graph (20 denoise
    steps each = 4000 steps, ~10^6 exchange hand-offs).  Every replay must reproduce the first eager result bit for bit and
    leave the abort word at zero.  (The exchange protocol is relaxed sc1 word stores / loads ordered by workgroup barriers --
    outside what the HIP memory model promises, see denoise.hip: this is the test that stands behind it.)"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    Ln, ncam, E = 50, 3, 120
    B = (cus - 16) // 8
    if B < 2:
        pytest.skip("device too small")
    m = _script_planner(a3d, dev)
    inp = C.trajectory_inputs(97, B, Ln, ncam, E, pad_last=5)
    d = {k: v.to(dev) for k, v in inp.items()}
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
    kw = dict(init_noise=d["init_noise"], step_noise=d["step_noise"], visual_tokens=C.tokens_from_maps(inp["fmap"]).to(dev), n_steps=20)
    first = m.compute_trajectory(*args, **kw)
    torch.cuda.synchronize()
    ps = m.prediction_head._last_persist
    assert ps is not None and ps["kvx"] is not None, "not on the persistent sampler"
    assert int(ps["sync"][2].item()) == 0 and torch.isfinite(first).all()
    bad = 0
    for rep in range(200):
        out = m.compute_trajectory(*args, use_graph=True, **kw)
        if rep % 20 == 19 or rep < 2:
            torch.cuda.synchronize()
            if not torch.equal(out, first):
                bad += 1
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    gsync = m._graph["state"]["persist"]["sync"] if isinstance(m._graph, dict) and "state" in m._graph and "persist" in m._graph["state"] else None
    if gsync is not None:
        assert int(gsync[2].item()) == 0
    print(f"[parity] persistent sampler stress: B = {B}, L = {Ln}, {2 * B * 4 + 16} workgroups on {cus} CUs, 200 replays x 20 steps, "
          f"{bad} mismatching checkpoints of 12")
    assert bad == 0
