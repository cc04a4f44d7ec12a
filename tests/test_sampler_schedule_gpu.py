"""Few-step trajectory sampling on the device: compute_trajectory(num_inference_steps=K, scheduler=..., eta=...) through the
persistent sampler (a3d_dn_persist_sched), the per-phase launches (a3d_dn_tail_sched), the op-by-op path and the multi-round loop
(a3d_ddpm_step_sched), hipGraph-captured and eager -- against the default 100-step call (bit identity of K = T), against each other,
and against a scheduled loop written HERE from the CPU oracle's pieces with float64 coefficient tables.

The schedule semantics, restated (diffusers is not a dependency): leading spacing r = T // K, t_i = (K - 1 - i) r; prev = t - r,
a_prev = acp[prev] or 1; every step x_prev = c0 clip(x0) + c1 x_t + c2 z after the in-painting; "ddpm": the fixed_small posterior
between t and prev; "ddim": sigma = eta sqrt((1-a_prev)/(1-a_t)) sqrt(1 - a_t/a_prev), c1 = sqrt(1-a_prev-sigma^2)/sqrt(1-a_t),
c0 = sqrt(a_prev) - c1 sqrt(a_t), c2 = sigma; the step at t = 0 returns the in-painted network output; noise row i = step position."""
import math
import os
import sys
from collections import Counter

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import common as C  # noqa: E402
from test_oracle_golden import _diffusion_params, load  # noqa: E402

pytestmark = pytest.mark.gpu

T, E, NCAM, H = 100, 120, 3, 8


def scale_close(name, got, ref, tol=1e-3, floor=1.0):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs().max().item()
    scale = max(floor, ref.abs().max().item())
    print(f"[parity] {name}: max_abs_err={err:.3e} ref_absmax={ref.abs().max().item():.3e} rel_to_scale={err / scale:.2e}")
    assert torch.isfinite(got).all(), name
    assert err <= tol * scale, f"{name}: max err {err:.3e} > {tol} * {scale:.3e}"


# ------------------------------------------------------------------------------------------------ the oracle loop
def ref_schedule(acp, K, scheduler, eta):
    """(timesteps, [K][3] float64 rows) from the float32 alphas_cumprod of one beta schedule."""
    r = T // K
    ts = [(K - 1 - i) * r for i in range(K)]
    rows = []
    for t in ts:
        a_t = float(acp[t])
        a_prev = float(acp[t - r]) if t - r >= 0 else 1.0
        if scheduler == "ddpm":
            cur_a = a_t / a_prev
            var = max((1 - a_prev) / (1 - a_t) * (1 - cur_a), 1e-20)
            rows.append((math.sqrt(a_prev) * (1 - cur_a) / (1 - a_t), math.sqrt(cur_a) * (1 - a_prev) / (1 - a_t), math.sqrt(var)))
        else:
            sigma = eta * math.sqrt((1 - a_prev) / (1 - a_t)) * math.sqrt(1 - a_t / a_prev)
            c1 = math.sqrt(max(1 - a_prev - sigma * sigma, 0.0)) / math.sqrt(1 - a_t)
            rows.append((math.sqrt(a_prev) - c1 * math.sqrt(a_t), c1, sigma))
    return ts, rows


def oracle_scheduled_loop(network, traj_mask, cg, gg, init_noise, step_noise, K, scheduler, eta, n_steps=None):
    """The scheduled sampling loop on the CPU: `network(traj, t)` is one evaluation of the oracle's head on the normalised,
    converted state; in-painting as the reference (oracle.diffusion.make_conditioning), the update with float64 coefficients."""
    from oracle import diffusion as OD
    o = OD.DDPMSchedules(T)
    ts, rows_pos = ref_schedule(o.acp_pos, K, scheduler, eta)
    _, rows_rot = ref_schedule(o.acp_rot, K, scheduler, eta)
    cond, cmask = OD.make_conditioning(traj_mask, cg, gg)
    traj = init_noise + cond
    trace = []
    for i, t in enumerate(ts[:n_steps]):
        out = network(traj, t).clone()
        out[cmask] = cond[cmask]
        if i < K - 1:
            x0 = out.double().clamp(-1.0, 1.0)
            new = torch.empty_like(x0)
            for sl, rows in ((slice(0, 3), rows_pos), (slice(3, None), rows_rot)):
                c0, c1, c2 = rows[i]
                new[..., sl] = c0 * x0[..., sl] + c1 * traj[..., sl].double()
                if c2 != 0.0:
                    new[..., sl] += c2 * step_noise[i][..., sl].double()
            out = new.float()
        traj = out
        trace.append(traj.clone())
    return traj, trace


def oracle_script_head(P, inp, tokens, sub, K, scheduler, eta, n_steps=None):
    """The single-round script head (oracle.diffusion.head_forward) on the samples `sub` of a trajectory batch -> final poses."""
    import numpy as np  # noqa: F401
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
        traj, trace = oracle_scheduled_loop(network, mask, cg, gg, inp["init_noise"][sub], inp["step_noise"][:K][:, sub], K,
                                            scheduler, eta, n_steps)
    final = OD.unconvert_rot(traj)
    return torch.cat([OD.unnormalize_pos(final[..., :3], bounds), final[..., 3:]], dim=-1), trace


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def planner(a3d, dev):
    r = load("diffusion.pt")
    m = a3d.DiffusionPlanner(embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=T)
    P = _diffusion_params(r)
    m.load_state_dict(P, strict=False)
    return m.to(dev).eval(), P


_INPUTS = {}


def inputs(dev, seed, B, Ln, pad_last):
    key = (seed, B, Ln, pad_last)
    if key not in _INPUTS:
        inp = C.trajectory_inputs(seed, B, Ln, NCAM, E, pad_last=pad_last)
        tokens = C.tokens_from_maps(inp["fmap"])
        d = {k: v.to(dev) for k, v in inp.items()}
        _INPUTS.clear()                                     # one shape at a time stays resident
        _INPUTS[key] = (inp, tokens, d, tokens.to(dev))
    return _INPUTS[key]


def sample(m, d, tokens_dev, K=None, scheduler="ddpm", eta=0.0, noise="by_position", **kw):
    if isinstance(noise, str):
        kw["step_noise"] = None if (scheduler == "ddim" and eta == 0) else d["step_noise"][:K].contiguous()
    elif noise is not None:
        kw["step_noise"] = noise
    return m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"],
                                init_noise=d["init_noise"], visual_tokens=tokens_dev, num_inference_steps=K, scheduler=scheduler,
                                eta=eta, **kw)


def abort_word(m):
    torch.cuda.synchronize()
    ps = m.prediction_head._last_persist
    assert ps is not None
    return int(ps["sync"][2].item())


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("B,Ln", [(3, 16), (2, 50)])
def test_full_ddpm_schedule_is_bit_identical_to_the_default_call(planner, dev, B, Ln):
    """num_inference_steps = T, scheduler = "ddpm" through a3d_dn_persist_sched (tables by step position: the AdaLN rows, the
    coefficients and the noise of timestep T - 1 - i at row i) against the default call (a3d_dn_persist, tables by timestep)."""
    m, _ = planner
    inp, tokens, d, tdev = inputs(dev, 91, B, Ln, 3)
    ref = sample(m, d, tdev, noise=d["step_noise"])
    assert m.last_sampler_path == "persistent (a3d_dn_persist)" and abort_word(m) == 0
    got = sample(m, d, tdev, K=T, noise=d["step_noise"].flip(0).contiguous())
    assert m.last_sampler_path == "persistent (a3d_dn_persist_sched)" and abort_word(m) == 0
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref), "K = T ddpm differs from the default chain (max abs diff %.3e)" % (got - ref).abs().max().item()
    # truncated alike: n_steps counts scheduled steps, and a truncated run has no terminal step
    ref7 = sample(m, d, tdev, noise=d["step_noise"], n_steps=7)
    got7 = sample(m, d, tdev, K=T, noise=d["step_noise"].flip(0).contiguous(), n_steps=7)
    assert torch.equal(got7, ref7)
    # and replayed from a captured graph
    g = [sample(m, d, tdev, K=T, noise=d["step_noise"].flip(0).contiguous(), use_graph=True) for _ in range(2)]
    assert torch.equal(g[0], ref) and torch.equal(g[1], ref)
    m._graph = None


ORACLE_CASES = [("ddpm", 0.0, 10), ("ddim", 0.0, 10), ("ddim", 0.5, 20)]


@pytest.mark.parametrize("scheduler,eta,K", ORACLE_CASES)
def test_cfg3_shape_scheduled_vs_oracle(planner, dev, scheduler, eta, K):
    """BASELINE.json configs[2] at its full shape (batch 64, horizon 16, S = 3074), K-step schedules, hipGraph-captured, against
    the oracle loop on two of the 64 samples -- at the bar of test_cfg3_full_shape_graph_vs_oracle (3e-4 of scale), which the
    100-step chain meets: a shorter chain gets no looser one."""
    m, P = planner
    B, Ln = 64, 16
    inp, tokens, d, tdev = inputs(dev, 91, B, Ln, 3)
    outs = [sample(m, d, tdev, K, scheduler, eta, use_graph=True).cpu() for _ in range(2)]
    assert m.last_sampler_path == "persistent (a3d_dn_persist_sched)"
    assert torch.equal(outs[0], outs[1]), "graph replay differs from the captured run"
    eager = sample(m, d, tdev, K, scheduler, eta).cpu()
    assert abort_word(m) == 0
    assert torch.equal(outs[0], eager), "graph differs from the eager launch"
    m._graph = None
    sub = [3, 40]                                          # one unpadded and one padded trajectory
    ofinal, _ = oracle_script_head(P, inp, tokens, sub, K, scheduler, eta)
    got = outs[0][sub]
    tag = f"cfg3 {scheduler} eta={eta} K={K}"
    scale_close(tag + " sampled xyz vs oracle", got[..., :3], ofinal[..., :3], 3e-4)
    sign = torch.sign((got[..., 3:] * ofinal[..., 3:]).sum(-1, keepdim=True))
    scale_close(tag + " sampled quaternion vs oracle", got[..., 3:] * sign, ofinal[..., 3:], 3e-4)


@pytest.mark.parametrize("scheduler,eta,K", ORACLE_CASES)
def test_horizon_50_scheduled_vs_oracle(planner, dev, scheduler, eta, K):
    """B = 24 trajectories of the deployed horizon 50 (four row tiles each: 2 * 24 * 4 + 16 = 208 workgroups), K-step schedules on
    the persistent sampler against the oracle loop on two samples, at the bar of
    test_persistent_sampler_script_horizon_50_vs_oracle (3e-4 of scale)."""
    m, P = planner
    B, Ln = 24, 50
    inp, tokens, d, tdev = inputs(dev, 93, B, Ln, 7)
    got = sample(m, d, tdev, K, scheduler, eta)
    assert m.last_sampler_path == "persistent (a3d_dn_persist_sched)"
    assert abort_word(m) == 0 and m.prediction_head._last_persist["kvx"] is not None
    pad = inp["mask"].sum(1)
    sub = [int((pad == 0).nonzero()[0]), int((pad > 0).nonzero()[0])]      # one unpadded and one padded trajectory
    ofinal, _ = oracle_script_head(P, inp, tokens, sub, K, scheduler, eta)
    o = got[sub].cpu()
    tag = f"L=50 B=24 {scheduler} eta={eta} K={K}"
    scale_close(tag + " sampled xyz vs oracle", o[..., :3], ofinal[..., :3], 3e-4)
    sign = torch.sign((o[..., 3:] * ofinal[..., 3:]).sum(-1, keepdim=True))
    scale_close(tag + " sampled quaternion vs oracle", o[..., 3:] * sign, ofinal[..., 3:], 3e-4)


@pytest.mark.parametrize("scheduler,eta,K,n_steps", [("ddpm", 0.0, 10, None), ("ddim", 0.5, 20, None), ("ddim", 0.0, 10, None),
                                                     ("ddpm", 0.0, 20, 6)])
def test_paths_agree_under_a_schedule(planner, dev, a3d, scheduler, eta, K, n_steps):
    """Persistent sampler vs per-phase launches (5e-5, the bar of test_persistent_sampler_equals_per_phase_launches) and per-phase
    launches vs the op-by-op path (2e-5, the bar of test_fused_denoise_step_equals_op_by_op_path) under a schedule, state by state
    and at the end; the abort word stays zero and a second launch reproduces the first bit for bit."""
    m, _ = planner
    B, Ln = 5, 16
    inp, tokens, d, tdev = inputs(dev, 95, B, Ln, 3)
    D = a3d.diffusion

    def run(persist, **kw):
        keep = D.DN_PERSIST
        D.DN_PERSIST = persist
        try:
            out = sample(m, d, tdev, K, scheduler, eta, n_steps=n_steps, **kw)
            path = m.last_sampler_path
            if persist and kw.get("fused", True):
                assert abort_word(m) == 0, "the persistent sampler gave up waiting"
            return out, path
        finally:
            D.DN_PERSIST = keep

    n = K if n_steps is None else n_steps
    tag = f"{scheduler} eta={eta} K={K} ({n} steps)"
    (got, path) = run(True)
    assert path == "persistent (a3d_dn_persist_sched)"
    (again, _) = run(True)
    assert torch.equal(again, got), "the scheduled persistent sampler is not run-to-run deterministic"
    ((ref, ref_trace), path) = run(False, return_trace=True)
    assert path == "per-phase fused launches" and len(ref_trace) == n
    scale_close(f"persistent vs per-phase, {tag} in one launch", got, ref, 5e-5)
    ((got_t, trace), _) = run(True, return_trace=True)
    for i in sorted(set([0, 1, n // 2, n - 1])):
        scale_close(f"persistent (traced) vs per-phase state after step {i}, {tag}", trace[i], ref_trace[i], 5e-5)
    scale_close(f"persistent traced vs one launch, {tag}", got_t, got, 1e-6)
    ((op, op_trace), path) = run(False, fused=False, return_trace=True)
    assert path == "op-by-op"
    for i in sorted(set([0, 1, n // 2, n - 1])):
        scale_close(f"per-phase vs op-by-op state after step {i}, {tag}", ref_trace[i], op_trace[i], 2e-5)
    scale_close(f"per-phase vs op-by-op final pose, {tag}", ref, op, 2e-5)


def test_graph_capture_follows_the_schedule(planner, dev, monkeypatch):
    """Capture and replay are bit-equal; another K or another scheduler recaptures and both results still equal the eager call;
    DDIM with eta = 0 and step_noise = None draws, captures and reads no noise table."""
    m, _ = planner
    B, Ln = 4, 16
    inp, tokens, d, tdev = inputs(dev, 97, B, Ln, 2)
    m._graph = None
    seen = []
    for K, scheduler, eta in [(10, "ddpm", 0.0), (20, "ddpm", 0.0), (20, "ddim", 0.5), (20, "ddim", 1.0), (10, "ddpm", 0.0)]:
        eager = sample(m, d, tdev, K, scheduler, eta)
        cap = sample(m, d, tdev, K, scheduler, eta, use_graph=True)
        g, key = m._graph["g"], m._graph["key"]
        assert key[-1] == (K, scheduler, float(eta))
        assert not seen or (g is not seen[-1][0] and key != seen[-1][1]), "a new schedule must recapture"
        rep = sample(m, d, tdev, K, scheduler, eta, use_graph=True)
        assert m._graph["g"] is g, "the same schedule must replay the captured graph"
        assert torch.equal(cap, eager) and torch.equal(rep, eager), (K, scheduler, eta)
        assert int(m._graph["state"]["persist"]["sync"][2].item()) == 0
        seen.append((g, key, eager))
    assert torch.equal(seen[0][2], seen[-1][2])
    assert not torch.equal(seen[1][2], seen[2][2]) and not torch.equal(seen[2][2], seen[3][2])      # eta acts
    # eta = 1 DDIM is the strided DDPM sampler up to the float32 rounding of the two coefficient tables: reported, not asserted
    print("[parity] ddim eta=1 vs strided ddpm, K=20: max_abs_diff=%.3e" % (seen[3][2] - seen[1][2]).abs().max().item())
    # ---- the noise-free schedule: no draw, no table in the captured set
    calls = []
    real_randn = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: (calls.append(a), real_randn(*a, **k))[1])
    eager = sample(m, d, tdev, 10, "ddim", 0.0, noise=None)
    cap = sample(m, d, tdev, 10, "ddim", 0.0, noise=None, use_graph=True)
    rep = sample(m, d, tdev, 10, "ddim", 0.0, noise=None, use_graph=True)
    monkeypatch.undo()
    assert not calls, "a noise-free schedule drew noise"
    assert torch.equal(cap, eager) and torch.equal(rep, eager) and torch.isfinite(eager).all()
    assert not any(t_.dim() == 4 and tuple(t_.shape[1:]) == (B, Ln, 9) for t_ in m._graph["static"]), "a noise table was captured"
    # a given table is ignored, not read: the result does not depend on it
    junk = sample(m, d, tdev, 10, "ddim", 0.0, noise=torch.full((10, B, Ln, 9), float("nan"), device=dev))
    assert torch.equal(junk, eager)
    m._graph = None


def test_multi_round_head_scheduled_vs_oracle(a3d, dev):
    """attn_rounds = 2 x feat_scales_to_use = 2 (the op-by-op loop over a3d_ddpm_step_sched; tests/golden/diffusion_multi.pt)
    under a schedule against the same oracle loop over oracle.diffusion.head_forward_multi.  Bar: 3e-4 of
    scale, the bar of the single-round oracle comparisons above (the existing 5-step test of this head allows 1e-3)."""
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

    for scheduler, eta, K in [("ddim", 0.5, 5), ("ddpm", 0.0, 4)]:
        sn = d["step_noise"][:K].contiguous()
        kw = dict(init_noise=d["init_noise"], step_noise=sn, visual_tokens=toks, num_inference_steps=K, scheduler=scheduler, eta=eta)
        args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
        final, trace = m.compute_trajectory(*args, return_trace=True, **kw)
        assert m.last_sampler_path == "multi-round" and len(trace) == K
        with torch.no_grad():
            otraj, otrace = oracle_scheduled_loop(network, inp["mask"], cg, gg, inp["init_noise"], inp["step_noise"][:K], K, scheduler, eta)
        tag = f"multi-round {scheduler} eta={eta} K={K}"
        for i in (0, K - 2, K - 1):
            scale_close(f"{tag} state after step {i} vs oracle", trace[i], otrace[i], 3e-4)
        ofinal = OD.unconvert_rot(otraj)
        ofinal = torch.cat([OD.unnormalize_pos(ofinal[..., :3], bounds), ofinal[..., 3:]], dim=-1)
        f = final.cpu()
        scale_close(f"{tag} sampled xyz vs oracle", f[..., :3], ofinal[..., :3], 3e-4)
        sign = torch.sign((f[..., 3:] * ofinal[..., 3:]).sum(-1, keepdim=True))
        scale_close(f"{tag} sampled quaternion vs oracle", f[..., 3:] * sign, ofinal[..., 3:], 3e-4)


# ------------------------------------------------------------------------------------------------ launch census
# Launches of ONE op-by-op denoise step of the `planner` head (trajectory encoder, instruction layer, eight attention layers, the two
# regressors, the DDPM step), recorded with the wrapper below at ea60aa8, the commit before sampler_plan; the same at L = 8 and L = 20.
OP_BY_OP_LAUNCHES_PER_STEP = 189
N_LAYERS = 8                                                # 4 shared + 2 position + 2 rotation layers of num_query_cross_attn_layers = 6

CENSUS = [  # name, Ln, G, DN_PERSIST, fused, path
    ("persistent", 8, None, True, None, "persistent (a3d_dn_persist)"),
    ("persistent, two row tiles", 20, None, True, None, "persistent (a3d_dn_persist)"),
    ("candidate group", 8, 2, True, None, "persistent (a3d_dn_persist_group)"),
    ("per-phase", 8, None, False, None, "per-phase fused launches"),
    ("op-by-op", 8, None, True, False, "op-by-op"),
    ("op-by-op, L = 20 without the persistent sampler", 20, None, False, None, "op-by-op"),
    ("op-by-op, L = 20 with too many trajectories for the CUs", 20, None, True, None, "op-by-op"),
]


def launches(m, a3d, d, tdev, persist, **kw):
    """Entry names of one eager compute_trajectory call, in launch order (lib.call wrapped as in test_act3d_gpu.py)."""
    D = a3d.diffusion
    seen, call, keep = [], a3d.lib.call, D.DN_PERSIST
    D.DN_PERSIST = persist
    a3d.ops.L.call = lambda entry, *args: (seen.append(entry), call(entry, *args))[1]
    try:
        m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], visual_tokens=tdev, **kw)
    finally:
        a3d.ops.L.call = call
        D.DN_PERSIST = keep
    return seen


@pytest.mark.parametrize("name,Ln,G,persist,fused,path", CENSUS, ids=[c[0] for c in CENSUS])
def test_launch_census_of_every_sampler_path(planner, dev, a3d, name, Ln, G, persist, fused, path):
    """Which entry points two eager steps of compute_trajectory launch, per path: the persistent sampler is ONE launch for the loop,
    the per-phase path 1 + 2 * layers + 1 per step, the op-by-op path no a3d_dn_* launch and the recorded count per step.  A call the
    plan sends to the op-by-op path builds no fused state first: it launches what the fused=False call launches."""
    m, _ = planner
    n = 2
    B = 2
    if "too many" in name:                                  # 2 * B * ceil(L / 16) + 16 one above the CU count
        B = (torch.cuda.get_device_properties(dev).multi_processor_count - 16) // 4 + 1
    inp, tokens, d, tdev = inputs(dev, 99, B, Ln, 2)
    seen = launches(m, a3d, d, tdev, persist, n_steps=n, fused=fused, num_samples=G)
    assert m.last_sampler_path == path
    dn = [e for e in seen if e.startswith("a3d_dn_")]
    print(f"[census] {name}: {len(seen)} launches in the call, a3d_dn_*: {sorted(set(dn))}, "
          f"a3d_proj_rope_split16: {seen.count('a3d_proj_rope_split16')}")
    if path.startswith("persistent"):
        assert dn == [path[path.index("(") + 1:-1]], dn
        assert abort_word(m) == 0
    elif path.startswith("per-phase"):
        per_step = {"a3d_dn_head": 1, "a3d_dn_cross": N_LAYERS, "a3d_dn_rest": N_LAYERS, "a3d_dn_tail": 1}
        assert sum(per_step.values()) == 1 + 2 * N_LAYERS + 1 == 18
        assert {e: dn.count(e) for e in set(dn)} == {e: n * c for e, c in per_step.items()}, dn
        first, last = seen.index("a3d_dn_head"), len(seen) - 1 - seen[::-1].index("a3d_dn_tail")
        assert last + 1 - first == n * 18, "other launches inside the step loop: %s" % seen[first:last + 1]
    else:
        assert not dn, dn
        ends = [i for i, e in enumerate(seen) if e == "a3d_ddpm_step"]
        assert len(ends) == n
        per_step = ends[1] - ends[0]
        steps = [seen[i + 1 - per_step:i + 1] for i in ends]
        print(f"[census] {name}: {per_step} launches per step")
        assert ends[0] + 1 - per_step >= 0 and steps[0] == steps[1]
        assert per_step == OP_BY_OP_LAUNCHES_PER_STEP
        if Ln > 16:
            # the op-by-op path launches a3d_proj_rope_split16 itself (encode_context, the self-attention operands), so "none of
            # build_fused's" is held against the fused=False call: the same launches in the same order, before the loop and in it
            ref = launches(m, a3d, d, tdev, persist, n_steps=n, fused=False)
            assert seen == ref, "a fused state was built for a call the op-by-op path serves: %s" % dict(Counter(seen) - Counter(ref))
