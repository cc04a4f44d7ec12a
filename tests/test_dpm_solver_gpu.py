"""scheduler="dpm++" (DPM-Solver++ 2M) on the device: compute_trajectory(num_inference_steps=K, scheduler="dpm++", solver_order=...,
lower_order_final=...) through the persistent sampler (a3d_dn_persist_sched / _group, the history tile in LDS), the per-phase launches
(a3d_dn_tail_sched), the op-by-op path and the multi-round loop (a3d_ddpm_step_hist) -- solver_order = 1 against "ddim" with eta = 0
(bit identity), order 2 against a loop written HERE from the CPU oracle's head with the float64 tables of tests/dpm_solver_ref.py,
the paths against each other, the history buffer across launches and graph replays, candidates, the guide, and Actioner.predict.

The update, restated: x_prev = c0 D_i + c1 x_t + kappa_i (D_i - D_{i-1}) with D_i the clipped, in-painted network output at step
position i, (c0, c1) the DDIM row at eta = 0 and kappa_i as in dpm_solver_ref.schedule; the step at position K - 1 (timestep 0)
returns the in-painted network output."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import common as C  # noqa: E402
import dpm_solver_ref as R  # noqa: E402
from test_oracle_golden import load  # noqa: E402
from test_sampler_schedule_gpu import H, T, abort_word, inputs, planner, sample, scale_close  # noqa: E402, F401

pytestmark = pytest.mark.gpu

PERSIST = "persistent (a3d_dn_persist_sched)"
GROUP = "persistent (a3d_dn_persist_group)"


def dpm(m, d, tdev, K, order=2, lof=True, **kw):
    """a "dpm++" call without a noise table (none is drawn or read)"""
    return sample(m, d, tdev, K, "dpm++", 0.0, noise=None, solver_order=order, lower_order_final=lof, **kw)


def ddim(m, d, tdev, K, **kw):
    return sample(m, d, tdev, K, "ddim", 0.0, noise=None, **kw)


class switch:
    """with switch(a3d, persist): the module switch that sends a call to the persistent sampler or past it"""

    def __init__(self, a3d, persist):
        self.D, self.persist = a3d.diffusion, persist

    def __enter__(self):
        self.keep, self.D.DN_PERSIST = self.D.DN_PERSIST, self.persist

    def __exit__(self, *exc):
        self.D.DN_PERSIST = self.keep


# ------------------------------------------------------------------------------------------------ the oracle loop
def oracle_dpm_loop(network, traj_mask, cg, gg, init_noise, K, order, lof, n_steps=None):
    """The multistep loop on the CPU: `network(traj, t)` is one evaluation of the oracle's head; in-painting as the reference
    (oracle.diffusion.make_conditioning); the update in float64 with the float64 tables of dpm_solver_ref."""
    from oracle import diffusion as OD
    o = OD.DDPMSchedules(T)
    ts, rows_pos, kap_pos = R.schedule(o.acp_pos, T, K, order, lof)
    _, rows_rot, kap_rot = R.schedule(o.acp_rot, T, K, order, lof)
    cond, cmask = OD.make_conditioning(traj_mask, cg, gg)
    traj = init_noise + cond
    trace, d_last = [], None
    for i, t in enumerate(ts[:n_steps]):
        out = network(traj, t).clone()
        out[cmask] = cond[cmask]
        if i < K - 1:
            x0 = out.double().clamp(-1.0, 1.0)
            new = torch.empty_like(x0)
            for sl, rows, kap in ((slice(0, 3), rows_pos, kap_pos), (slice(3, None), rows_rot, kap_rot)):
                new[..., sl] = R.three_term_step(rows[i], kap[i], traj[..., sl].double(), x0[..., sl],
                                                 None if d_last is None else d_last[..., sl])
            d_last = x0
            out = new.float()
        traj = out
        trace.append(traj.clone())
    return traj, trace


def oracle_script_head_dpm(P, inp, tokens, sub, K, order, lof):
    """The single-round script head (oracle.diffusion.head_forward) on the samples `sub` of a trajectory batch -> final poses."""
    from oracle import diffusion as OD
    from oracle import sampling as OS
    bounds = torch.from_numpy(C.DIFFUSION_BOUNDS)
    pcdn = OD.normalize_pos(inp["pcd"][sub].permute(0, 1, 3, 4, 2), bounds).permute(0, 1, 4, 2, 3).contiguous()
    cxyz = torch.from_numpy(OS.pcd_downsample(pcdn.numpy(), 8))
    cg, gg = inp["curr_gripper"][sub].clone(), inp["goal_gripper"][sub].clone()
    cg[:, :3] = OD.normalize_pos(cg[:, :3], bounds)
    gg[:, :3] = OD.normalize_pos(gg[:, :3], bounds)
    cg, gg = OD.convert_rot(cg), OD.convert_rot(gg)
    mask, toks, instr = inp["mask"][sub], tokens[sub], inp["instr"][sub]

    def network(traj, t):
        return OD.head_forward(P, traj, mask, torch.full((traj.shape[0],), t, dtype=torch.long), toks, cxyz, cg, gg, instr, H)

    with torch.no_grad():
        traj, _ = oracle_dpm_loop(network, mask, cg, gg, inp["init_noise"][sub], K, order, lof)
    final = OD.unconvert_rot(traj)
    return torch.cat([OD.unnormalize_pos(final[..., :3], bounds), final[..., 3:]], dim=-1)


def pose_close(tag, got, ref, tol):
    scale_close(tag + " xyz", got[..., :3], ref[..., :3], tol)
    sign = torch.sign((got[..., 3:] * ref[..., 3:]).sum(-1, keepdim=True))
    scale_close(tag + " quaternion", got[..., 3:] * sign, ref[..., 3:], tol)


# ------------------------------------------------------------------------------------------------ 1: order 1 is DDIM
@pytest.mark.parametrize("B,Ln", [(3, 16), (2, 17)])
def test_solver_order_1_is_ddim_bit_for_bit(planner, dev, a3d, B, Ln):
    """kappa = 0 everywhere: the history variants of the three kernels (and of the persistent sampler's tail) must give the bits of
    the kernels without it -- the same c0 x0 + c1 x_t, nothing added -- on every path the shape can take."""
    m, _ = planner
    K = 10
    inp, tokens, d, tdev = inputs(dev, 91, B, Ln, 3)
    paths = [(True, None, PERSIST), (False, None, "per-phase fused launches" if Ln <= 16 else "op-by-op")]
    if Ln <= 16:
        paths.append((False, False, "op-by-op"))
    for persist, fused, label in paths:
        with switch(a3d, persist):
            ref = ddim(m, d, tdev, K, fused=fused)
            assert m.last_sampler_path == label
            got = dpm(m, d, tdev, K, order=1, fused=fused)
            assert m.last_sampler_path == label
            both = dpm(m, d, tdev, K, order=1, lof=False, fused=fused)
        if persist:
            assert abort_word(m) == 0
        assert torch.isfinite(ref).all()
        assert torch.equal(got, ref), "%s: solver_order=1 differs from ddim (max abs diff %.3e)" % (label, (got - ref).abs().max().item())
        assert torch.equal(both, ref), label
        # and it is not a schedule on which nothing happens: order 2 moves the result
        with switch(a3d, persist):
            assert not torch.equal(dpm(m, d, tdev, K, fused=fused), ref), label


def test_solver_order_1_is_ddim_on_the_group_path(planner, dev):
    from test_multi_candidate_gpu import cand_inputs, sample_group
    m, _ = planner
    B, G, Ln, K = 2, 3, 16, 10
    inp, tokens, d, tdev = cand_inputs(dev, 91, B, G, Ln, 3)
    ref = sample_group(m, d, tdev, G, K, "ddim", 0.0)
    assert m.last_sampler_path == GROUP
    got = sample_group(m, d, tdev, G, K, "dpm++", 0.0, step=None, solver_order=1)
    assert m.last_sampler_path == GROUP and abort_word(m) == 0
    assert got.shape == (B, G, Ln, 7) and torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ 2: order 2 against the oracle
@pytest.mark.parametrize("B,Ln", [(3, 16), (2, 17)])
@pytest.mark.parametrize("K", [10, 4])
def test_order_2_vs_float64_table_oracle(planner, dev, B, Ln, K):
    """One row tile with padded rows, and two tiles (the second with one row); K = 10 and the smallest schedule with a second-order
    step.  Bar: 3e-4 of scale, the bar of the scheduled-sampler comparisons (test_sampler_schedule_gpu)."""
    m, P = planner
    inp, tokens, d, tdev = inputs(dev, 91, B, Ln, 3)
    got = dpm(m, d, tdev, K)
    assert m.last_sampler_path == PERSIST and abort_word(m) == 0
    sub = [0, B - 1]                                        # one unpadded and one padded trajectory
    assert int(inp["mask"][0].sum()) == 0 and int(inp["mask"][B - 1].sum()) == 3
    want = oracle_script_head_dpm(P, inp, tokens, sub, K, 2, True)
    pose_close(f"dpm++ order 2 K={K} B={B} L={Ln} sampled vs oracle", got[sub].cpu(), want, 3e-4)


# ------------------------------------------------------------------------------------------------ 3: the paths
@pytest.mark.parametrize("n_steps", [None, 6])
def test_paths_agree_state_by_state(planner, dev, a3d, n_steps):
    """The bars of test_paths_agree_under_a_schedule: persistent vs per-phase 5e-5, per-phase vs op-by-op 2e-5, the persistent
    sampler traced (one launch per step: the history travels through the global buffer) vs one launch (the LDS tile) 1e-6."""
    m, _ = planner
    B, Ln, K = 5, 16, 10
    inp, tokens, d, tdev = inputs(dev, 95, B, Ln, 3)
    n = K if n_steps is None else n_steps
    tag = f"dpm++ K={K} ({n} steps)"
    with switch(a3d, True):
        got = dpm(m, d, tdev, K, n_steps=n_steps)
        assert m.last_sampler_path == PERSIST and abort_word(m) == 0
        again = dpm(m, d, tdev, K, n_steps=n_steps)
        assert abort_word(m) == 0
        got_t, trace = dpm(m, d, tdev, K, n_steps=n_steps, return_trace=True)
        assert abort_word(m) == 0 and len(trace) == n
    assert torch.equal(again, got), "the persistent sampler is not run-to-run deterministic under dpm++"
    with switch(a3d, False):
        ref, ref_trace = dpm(m, d, tdev, K, n_steps=n_steps, return_trace=True)
        assert m.last_sampler_path == "per-phase fused launches" and len(ref_trace) == n
        op, op_trace = dpm(m, d, tdev, K, n_steps=n_steps, return_trace=True, fused=False)
        assert m.last_sampler_path == "op-by-op"
    scale_close(f"persistent vs per-phase, {tag} in one launch", got, ref, 5e-5)
    for i in sorted(set([0, 1, n // 2, n - 1])):
        scale_close(f"persistent (traced) vs per-phase state after step {i}, {tag}", trace[i], ref_trace[i], 5e-5)
        scale_close(f"per-phase vs op-by-op state after step {i}, {tag}", ref_trace[i], op_trace[i], 2e-5)
    scale_close(f"persistent traced vs one launch, {tag}", got_t, got, 1e-6)
    # per-phase vs op-by-op at the end: the final STATE is trace[n - 1] above; of the final pose the position is held to the same
    # bar.  Its quaternion is printed, not asserted: signal_to_pose orthonormalises the two 6D vectors, which turns a state
    # difference e into an angle e / |a2 - (b1 . a2) b1|, and after the terminal step of the 10-step chain (the raw output of this
    # seeded, untrained network) sample 4, row 2 has |a2 - (b1 . a2) b1| = 0.0123: the states differ by 3.4e-6 there (2.2e-6 of scale
    # overall), the quaternions by 1.08e-4 -- the conversion's conditioning at that row, not a difference between the samplers
    scale_close(f"per-phase vs op-by-op final position, {tag}", ref[..., :3], op[..., :3], 2e-5)
    print(f"[parity] per-phase vs op-by-op final quaternion, {tag}: max_abs_diff={(ref[..., 3:] - op[..., 3:]).abs().max().item():.3e}")


# ------------------------------------------------------------------------------------------------ 4: the history buffer
def test_history_buffer_and_graph_replay(planner, dev, monkeypatch):
    """Position 0 never reads the history: a buffer full of NaN before a replay changes nothing.  Capture, two replays and the eager
    call agree bit for bit; another solver_order recaptures; no noise is drawn and no noise table is captured."""
    m, _ = planner
    B, Ln, K = 4, 16, 10
    inp, tokens, d, tdev = inputs(dev, 97, B, Ln, 2)
    m._graph = None
    calls = []
    real_randn = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: (calls.append(a), real_randn(*a, **k))[1])
    eager = dpm(m, d, tdev, K)
    cap = dpm(m, d, tdev, K, use_graph=True)
    g, key = m._graph["g"], m._graph["key"]
    assert key[-1] == (K, "dpm++", 0.0, 2, True)
    hist = m._graph["state"]["hist"]
    assert hist.shape == (B, Ln, 9) and hist.dtype == torch.float32 and any(t_ is hist for t_ in m._graph["static"])
    torch.cuda.synchronize()
    assert torch.isfinite(hist).all() and hist.abs().max() > 0 and hist.abs().max() <= 1, "the steps leave their clipped prediction"
    rep = dpm(m, d, tdev, K, use_graph=True)
    assert m._graph["g"] is g and m._graph["state"]["hist"] is hist
    hist.fill_(float("nan"))
    poisoned = dpm(m, d, tdev, K, use_graph=True)
    assert m._graph["g"] is g
    monkeypatch.undo()
    assert not calls, "dpm++ drew noise"
    assert torch.isfinite(eager).all()
    assert torch.equal(cap, eager) and torch.equal(rep, eager) and torch.equal(poisoned, eager)
    assert int(m._graph["state"]["persist"]["sync"][2].item()) == 0
    assert not any(t_.dim() == 4 and tuple(t_.shape[1:]) == (B, Ln, 9) for t_ in m._graph["static"]), "a noise table was captured"
    # a given noise table is ignored, not read
    junk = sample(m, d, tdev, K, "dpm++", 0.0, noise=torch.full((K, B, Ln, 9), float("nan"), device=dev))
    assert torch.equal(junk, eager)
    # another solver_order (and another lower_order_final) recaptures, and still equals its eager call
    for order, lof in ((1, True), (2, False)):
        other = dpm(m, d, tdev, K, order=order, lof=lof, use_graph=True)
        assert m._graph["g"] is not g and m._graph["key"] != key and m._graph["key"][-1] == (K, "dpm++", 0.0, order, lof)
        assert torch.equal(other, dpm(m, d, tdev, K, order=order, lof=lof)) and not torch.equal(other, eager)
    # a scheduler without a history has no buffer
    ddim(m, d, tdev, K, use_graph=True)
    assert "hist" not in m._graph["state"]
    m._graph = None


# ------------------------------------------------------------------------------------------------ 5: candidates
def test_group_path_vs_expanded_batch(planner, dev):
    """G = 3 candidates per scene on the shared K / V cache against the same candidates as a batch of B G scenes: 5e-5 of scale, the
    bar of test_multi_candidate_gpu.test_equals_the_replicated_call."""
    from test_multi_candidate_gpu import cand_inputs, sample_group, sample_replicated
    m, _ = planner
    B, G, Ln, K = 2, 3, 16, 10
    inp, tokens, d, tdev = cand_inputs(dev, 91, B, G, Ln, 3)
    got = sample_group(m, d, tdev, G, K, "dpm++", 0.0, step=None)
    assert m.last_sampler_path == GROUP and abort_word(m) == 0 and got.shape == (B, G, Ln, 7)
    assert m._last_state["hist"].shape == (B * G, Ln, 9)
    ref = sample_replicated(m, d, tdev, G, K, "dpm++", 0.0)
    assert m.last_sampler_path == PERSIST and abort_word(m) == 0
    scale_close(f"dpm++ num_samples B={B} G={G} L={Ln} K={K} vs expanded batch", got, ref, 5e-5)
    assert not torch.equal(got, sample_group(m, d, tdev, G, K, "ddim", 0.0))


# ------------------------------------------------------------------------------------------------ 6: guide
def test_guided_segments_continue_the_chain(planner, dev, a3d):
    """guide from the middle of the loop on: one launch for positions 0..4, then one launch per step with the guide pair between them
    -- the history crosses launches through the global buffer.  Against the per-phase guided run (5e-5 of scale); the pinned rows
    are the in-painted ones, whatever the sampler."""
    m, _ = planner
    B, Ln, K = 3, 16, 10
    inp, tokens, d, tdev = inputs(dev, 91, B, Ln, 3)
    guide = dict(push=0.5, start=0.5)
    with switch(a3d, True):
        got = dpm(m, d, tdev, K, guide=guide)
        assert m.last_sampler_path == PERSIST and abort_word(m) == 0 and m.last_guidance.steps == (5, 6, 7, 8, 9)
        plain = dpm(m, d, tdev, K)
        base = ddim(m, d, tdev, K)
    with switch(a3d, False):
        ref = dpm(m, d, tdev, K, guide=guide)
        assert m.last_sampler_path == "per-phase fused launches"
    assert torch.isfinite(got).all() and not torch.equal(got, plain)
    scale_close(f"dpm++ guided K={K}: persistent (segmented) vs per-phase", got, ref, 5e-5)
    npad = d["mask"].sum(1)
    ar = torch.arange(Ln, device=dev)[None, :]
    pinned = (ar == 0) | (ar >= (Ln - npad - 1)[:, None])
    assert torch.equal(got[pinned], base[pinned]) and not torch.equal(got[~pinned], base[~pinned])


# ------------------------------------------------------------------------------------------------ 7: multi-round head
def test_multi_round_head_vs_oracle(a3d, dev):
    """attn_rounds = 2 x feat_scales_to_use = 2 (tests/golden/diffusion_multi.pt; the op-by-op loop over a3d_ddpm_step_hist) at
    K = 10 against the same loop over oracle.diffusion.head_forward_multi: 3e-4 of scale."""
    from oracle import diffusion as OD
    from test_oracle_golden import multi_head_inputs
    r = load("diffusion_multi.pt")
    cfg = r["cfg"]
    inp, feats, xyz, P, bounds = multi_head_inputs(r)
    m = a3d.DiffusionPlanner(embedding_dim=cfg["E"], output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, feat_scales_to_use=2, attn_rounds=2,
                             weight_tying=False, gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D",
                             diffusion_timesteps=T, dropout=0.0)
    m.load_state_dict(P, strict=False)
    m.to(dev).eval()
    d = {k: v.to(dev) for k, v in inp.items()}
    toks = [f.to(dev) for f in feats]
    cg, gg = r["conv"]["curr9"], r["conv"]["goal9"]

    def network(traj, t):
        outs, _ = OD.head_forward_multi(P, traj, inp["mask"], torch.full((traj.shape[0],), t, dtype=torch.long), feats, xyz, cg, gg,
                                        inp["instr"], 8, attn_rounds=2, feat_scales=2)
        return outs[-1]

    K = 10
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
    final, trace = m.compute_trajectory(*args, return_trace=True, init_noise=d["init_noise"], visual_tokens=toks,
                                        num_inference_steps=K, scheduler="dpm++")
    assert m.last_sampler_path == "multi-round" and len(trace) == K
    with torch.no_grad():
        otraj, otrace = oracle_dpm_loop(network, inp["mask"], cg, gg, inp["init_noise"], K, 2, True)
    for i in (0, 1, K - 2, K - 1):
        scale_close(f"multi-round dpm++ K={K} state after step {i} vs oracle", trace[i], otrace[i], 3e-4)
    ofinal = OD.unconvert_rot(otraj)
    ofinal = torch.cat([OD.unnormalize_pos(ofinal[..., :3], bounds), ofinal[..., 3:]], dim=-1)
    pose_close(f"multi-round dpm++ K={K} sampled vs oracle", final.cpu(), ofinal, 3e-4)


# ------------------------------------------------------------------------------------------------ 8: Actioner.predict
def test_actioner_predict_equals_the_chained_call(a3d, dev):
    from test_actioner_gpu import make_keypose, make_planner, observation, set_rng
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        kp = make_keypose(a3d, dev)
        pl = make_planner(a3d, dev, backbone_of=kp)
        instr = torch.randn(1, 53, 512, generator=torch.Generator().manual_seed(77)).to(dev)
        B, Ln = 2, 16
        o = observation(dev, 41, B, Ln)
        act = a3d.Actioner(kp, pl, predict_trajectory=True)
        act.set_instruction(instr)
        kw = dict(scheduler="dpm++", num_inference_steps=10, init_noise=o["init_noise"])
        for _ in range(2):                       # settle the convolution library's algorithm choice
            set_rng(kp)
            out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], **kw)
        assert out["trajectory"].shape == (B, Ln, 7) and torch.isfinite(out["trajectory"]).all()
        assert pl.last_sampler_path == PERSIST
        rgb = o["rgbs"][:, -1] / 2 + 0.5
        args = (o["mask"], rgb, o["pcds"][:, -1], instr.expand(B, -1, -1).contiguous(), o["gripper"][:, -1, :7], out["action"][..., :7])
        want = pl.compute_trajectory(*args, **kw)
        assert torch.equal(out["trajectory"], want)
        assert not torch.equal(want, pl.compute_trajectory(*args, **dict(kw, scheduler="ddim")))
        rng = kp._rng_state.clone()
        with pytest.raises(ValueError):          # the solver keywords reach the host-side check before the keypose half runs
            act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], **dict(kw, scheduler="ddim", solver_order=1))
        assert torch.equal(kp._rng_state, rng)
        set_rng(kp)
        assert torch.equal(act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], solver_order=1, **kw)["trajectory"],
                           pl.compute_trajectory(*args, **dict(kw, scheduler="ddim")))
    finally:
        torch.backends.cudnn.deterministic = old
