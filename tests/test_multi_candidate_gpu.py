"""Several candidate trajectories per scene on the device: compute_trajectory(num_samples=G) through a3d_dn_persist_group (one
context K / V cache per scene, one K / V pass per chunk of candidates) against the existing single-candidate call on inputs
repeated G times along the batch axis (the reference: today's behaviour), against the CPU oracle's loop, eager and hipGraph-replayed,
on the fallback paths, and with the bounded-wait abort forced once.

Trajectory order is scene-major: candidate g of scene b is trajectory b G + g.  Bars: 5e-5 of the tensor scale max(1, |ref|_max)
against the replicated call and between candidates (test_persistent_sampler_equals_per_phase_launches), 3e-4 against the oracle
(test_cfg3_full_shape_graph_vs_oracle), 5e-5 persistent <-> per-phase and 2e-5 per-phase <-> op-by-op on the fallbacks."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))             # the fallback child runs this file as a script, without conftest
sys.path.insert(0, os.path.join(HERE, "golden"))
import common as C  # noqa: E402
from test_oracle_golden import _diffusion_params, load  # noqa: E402

pytestmark = pytest.mark.gpu

T, E, NCAM, H = 100, 120, 3, 8
GROUP_PATH = "persistent (a3d_dn_persist_group)"


def scale_err(name, got, ref, tol, floor=1.0):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs().max().item()
    scale = max(floor, ref.abs().max().item())
    print(f"[parity] {name}: max_abs_err={err:.3e} ref_absmax={ref.abs().max().item():.3e} rel_to_scale={err / scale:.2e} "
          f"torch.equal={torch.equal(got, ref)}")
    assert torch.isfinite(got).all(), name
    assert err <= tol * scale, f"{name}: max err {err:.3e} > {tol} * {scale:.3e}"


def make_planner(a3d, dev):
    r = load("diffusion.pt")
    m = a3d.DiffusionPlanner(embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=T)
    P = _diffusion_params(r)
    m.load_state_dict(P, strict=False)
    return m.to(dev).eval(), P


@pytest.fixture(scope="module")
def planner(a3d, dev):
    return make_planner(a3d, dev)


def cand_inputs(dev, seed, B, G, Ln, pad_last, ncam=NCAM):
    """Per-scene inputs of C.trajectory_inputs + per-candidate noise: init (B, G, L, 9), step (T, B, G, L, 9)."""
    inp = C.trajectory_inputs(seed, B, Ln, ncam, E, pad_last=pad_last)
    tokens = C.tokens_from_maps(inp["fmap"])
    g = torch.Generator().manual_seed(1000 + seed)
    inp["init_noise"] = torch.randn(B, G, Ln, 9, generator=g)
    inp["step_noise"] = torch.randn(T, B, G, Ln, 9, generator=g)
    del inp["fmap"]
    d = {k: v.to(dev) for k, v in inp.items()}
    return inp, tokens, d, tokens.to(dev)


def _noise(step, K, scheduler, eta):
    if scheduler == "ddim" and eta == 0:
        return None
    return step if K is None else step[:K].contiguous()


def sample_group(m, d, tdev, G, K=None, scheduler="ddpm", eta=0.0, init=None, step=None, **kw):
    init = d["init_noise"] if init is None else init
    step = d["step_noise"] if step is None else step
    return m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], init_noise=init,
                                step_noise=_noise(step, K, scheduler, eta), visual_tokens=tdev, num_inference_steps=K,
                                scheduler=scheduler, eta=eta, num_samples=G, **kw)


def sample_replicated(m, d, tdev, G, K=None, scheduler="ddpm", eta=0.0, **kw):
    """Today's call on every input repeated G times along the batch axis and the same noise reshaped -> (B, G, L, 7)."""
    rep = lambda x: x.repeat_interleave(G, 0).contiguous()
    B, _, Ln, D = d["init_noise"].shape
    step = _noise(d["step_noise"], K, scheduler, eta)
    out = m.compute_trajectory(rep(d["mask"]), None, rep(d["pcd"]), rep(d["instr"]), rep(d["curr_gripper"]), rep(d["goal_gripper"]),
                               init_noise=d["init_noise"].reshape(B * G, Ln, D),
                               step_noise=None if step is None else step.reshape(step.shape[0], B * G, Ln, D).contiguous(),
                               visual_tokens=rep(tdev), num_inference_steps=K, scheduler=scheduler, eta=eta, **kw)
    return out.reshape(B, G, Ln, out.shape[-1])


def abort_word(m):
    torch.cuda.synchronize()
    ps = m.prediction_head._last_persist
    assert ps is not None
    return int(ps["sync"][2].item())


SCHEDULES = [("full chain, 12 steps", dict(n_steps=12)), ("ddpm K=10", dict(K=10, scheduler="ddpm")),
             ("ddim eta=0 K=10", dict(K=10, scheduler="ddim", eta=0.0))]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("B,G,Ln", [(3, 4, 16), (2, 5, 16), (2, 3, 20), (2, 2, 50)])
def test_equals_the_replicated_call(planner, dev, B, G, Ln):
    """One K / V pass per candidate chunk against G copies of the scene in the batch: the streamed arithmetic per query tile is the
    same, only the grouping of the tiles into items differs."""
    m, _ = planner
    inp, tokens, d, tdev = cand_inputs(dev, 91, B, G, Ln, 3)
    for tag, kw in SCHEDULES:
        got = sample_group(m, d, tdev, G, **kw)
        assert m.last_sampler_path == GROUP_PATH and abort_word(m) == 0
        assert got.shape == (B, G, Ln, 7)
        ref = sample_replicated(m, d, tdev, G, **kw)
        assert "persistent (a3d_dn_persist" in m.last_sampler_path and m.last_sampler_path != GROUP_PATH and abort_word(m) == 0
        scale_err(f"num_samples B={B} G={G} L={Ln} vs replicated call, {tag}", got, ref, 5e-5)
    # traced: every entry (B, G, L, D), the states of the one-launch result
    final, trace = sample_group(m, d, tdev, G, K=10, return_trace=True)
    assert len(trace) == 10 and all(x.shape == (B, G, Ln, 9) for x in trace) and final.shape == (B, G, Ln, 7)
    scale_err(f"num_samples B={B} G={G} L={Ln} traced vs one launch", final, sample_group(m, d, tdev, G, K=10), 1e-6)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("B,G,Ln,pad,seed,K,scheduler,eta", [(16, 4, 16, 3, 91, 10, "ddpm", 0.0), (12, 2, 50, 7, 93, 10, "ddim", 0.5)])
def test_candidates_vs_oracle(planner, dev, B, G, Ln, pad, seed, K, scheduler, eta):
    """A cfg-3-shaped call (B G = 64 trajectories of horizon 16, S = 3074) and a script-horizon call (B G = 24 of horizon 50) against
    the oracle's scheduled loop on every candidate of two scenes (one unpadded, one padded)."""
    from test_sampler_schedule_gpu import oracle_script_head
    m, P = planner
    inp, tokens, d, tdev = cand_inputs(dev, seed, B, G, Ln, pad)
    got = sample_group(m, d, tdev, G, K, scheduler, eta, use_graph=True)
    assert m.last_sampler_path == GROUP_PATH
    eager = sample_group(m, d, tdev, G, K, scheduler, eta)
    assert abort_word(m) == 0 and torch.equal(got, eager), "graph differs from the eager launch"
    m._graph = None
    npad = inp["mask"].sum(1)
    scenes = [int((npad == 0).nonzero()[0]), int((npad > 0).nonzero()[0])]
    # the oracle sees the candidates as a batch: scene inputs repeated, the candidates' own noise
    rep = {k: v.repeat_interleave(G, 0) for k, v in inp.items() if k not in ("init_noise", "step_noise")}
    rep["init_noise"] = inp["init_noise"].reshape(B * G, Ln, 9)
    rep["step_noise"] = inp["step_noise"].reshape(T, B * G, Ln, 9)
    sub = [s * G + g for s in scenes for g in range(G)]
    ofinal, _ = oracle_script_head(P, rep, tokens.repeat_interleave(G, 0), sub, K, scheduler, eta)
    o = got[scenes].reshape(len(sub), Ln, 7).cpu()
    tag = f"num_samples B={B} G={G} L={Ln} {scheduler} eta={eta} K={K}"
    scale_err(tag + " sampled xyz vs oracle", o[..., :3], ofinal[..., :3], 3e-4)
    sign = torch.sign((o[..., 3:] * ofinal[..., 3:]).sum(-1, keepdim=True))
    scale_err(tag + " sampled quaternion vs oracle", o[..., 3:] * sign, ofinal[..., 3:], 3e-4)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("B,G,Ln", [(3, 4, 16), (2, 3, 20)])
def test_candidates_are_independent_and_deterministic(planner, dev, B, G, Ln):
    m, _ = planner
    inp, tokens, d, tdev = cand_inputs(dev, 95, B, G, Ln, 2)
    kw = dict(K=10, scheduler="ddim", eta=0.5)
    a = sample_group(m, d, tdev, G, **kw)
    b = sample_group(m, d, tdev, G, **kw)
    assert abort_word(m) == 0 and torch.equal(a, b), "two launches with identical inputs differ"
    # only candidate 1's draws change: every other candidate of every scene is untouched
    init, step = d["init_noise"].clone(), d["step_noise"].clone()
    init[:, 1] = torch.randn_like(init[:, 1])
    step[:, :, 1] = torch.randn_like(step[:, :, 1])
    c = sample_group(m, d, tdev, G, init=init, step=step, **kw)
    others = [g for g in range(G) if g != 1]
    assert torch.equal(c[:, others], a[:, others]), "another candidate's noise leaked (max abs diff %.3e)" % (c[:, others] - a[:, others]).abs().max().item()
    assert not torch.equal(c[:, 1], a[:, 1])
    # equal noise: the candidates of a scene agree; different noise: they differ
    init = d["init_noise"][:, :1].expand(-1, G, -1, -1).contiguous()
    step = d["step_noise"][:, :, :1].expand(-1, -1, G, -1, -1).contiguous()
    e = sample_group(m, d, tdev, G, init=init, step=step, **kw)
    for g in range(1, G):
        scale_err(f"B={B} G={G} L={Ln} candidate {g} vs candidate 0 on equal noise", e[:, g], e[:, 0], 5e-5)
    for g in range(1, G):
        assert (a[:, g] - a[:, 0]).abs().max().item() > 1e-3, "candidates with different noise coincide"


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("B,G,Ln,pad", [(4, 4, 16, 3), (2, 2, 50, 7)])
def test_candidates_conform_to_the_conditioning(planner, dev, B, G, Ln, pad):
    """Row 0 holds the scene's current pose and the goal row and every row after it the goal / padding in-painting, for every
    candidate, exactly as the single-candidate call returns them for that scene."""
    m, _ = planner
    inp, tokens, d, tdev = cand_inputs(dev, 97, B, G, Ln, pad)
    got = sample_group(m, d, tdev, G, K=10)
    single = m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"],
                                  init_noise=d["init_noise"][:, 0].contiguous(), step_noise=d["step_noise"][:10, :, 0].contiguous(),
                                  visual_tokens=tdev, num_inference_steps=10)
    npad = inp["mask"].sum(1)
    assert int(npad.max()) == pad and int(npad.min()) == 0
    for b in range(B):
        goal = Ln - int(npad[b]) - 1
        rows = [0] + list(range(goal, Ln))
        for g in range(G):
            assert torch.equal(got[b, g, rows], single[b, rows]), (b, g)
        cg, gg = d["curr_gripper"][b], d["goal_gripper"][b]
        assert (got[b, :, 0, :3] - cg[:3]).abs().max().item() < 1e-5 and (got[b, :, goal, :3] - gg[:3]).abs().max().item() < 1e-5
        qs = torch.sign((got[b, :, 0, 3:7] * cg[3:7]).sum(-1, keepdim=True))
        # (fp32 round trip quaternion -> 6D -> Gram-Schmidt -> quaternion with a square-root pivot: 1e-4, not the 1e-5 of the positions)
        assert (got[b, :, 0, 3:7] * qs - cg[3:7]).abs().max().item() < 1e-4
    # candidate 0 drew the single call's noise: the whole trajectory follows it (padded steps included)
    scale_err(f"B={B} G={G} L={Ln} candidate 0 vs the single-candidate call", got[:, 0], single, 5e-5)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("B,G,Ln", [(3, 4, 16), (2, 2, 50)])
def test_the_cache_is_per_scene(planner, dev, a3d, B, G, Ln):
    m, _ = planner
    inp, tokens, d, tdev = cand_inputs(dev, 99, B, G, Ln, 2)
    sample_group(m, d, tdev, G, K=10)
    assert m.last_sampler_path == GROUP_PATH and abort_word(m) == 0
    st = m._last_state
    S = NCAM * 1024 + 2
    Sp = -(-S // 64) * 64
    assert st["n_cand"] == G and len(st["layers"]) == 8
    for rec in st["layers"]:
        assert tuple(rec["Kf"].shape) == (B, H, Sp, 32) and tuple(rec["Vt"].shape) == (B, H, 2, 16, Sp)
    assert st["lang_kv"].numel() == B * st["S_lang"] * 2 * E
    ps = st["persist"]
    NT = -(-Ln // 16)
    lib = a3d.lib.load()
    assert ps["group"] and ps["n_cand"] == G and ps["qbuf"].numel() == 2 * B * G * NT * 16 * 128
    assert ps["xbuf"].numel() == lib.a3d_dn_persist_xbuf_floats(B * G, Ln)
    assert (ps["kvx"] is None) == (NT == 1) and (NT == 1 or ps["kvx"].numel() == lib.a3d_dn_persist_kvx_floats(B * G, Ln, E))
    assert tuple(st["kmask"].shape) == (B * G, Ln)


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("B,G,Ln", [(3, 4, 16), (2, 2, 50)])
def test_graph_replay_with_candidates(planner, dev, a3d, B, G, Ln):
    m, _ = planner
    m._graph = None
    inp, tokens, d, tdev = cand_inputs(dev, 101, B, G, Ln, 3)
    graph = None
    for rep in range(3):                                      # capture + two replays, fresh noise every time
        init, step = torch.randn_like(d["init_noise"]), torch.randn_like(d["step_noise"])
        eager = sample_group(m, d, tdev, G, K=20, init=init, step=step)
        got = sample_group(m, d, tdev, G, K=20, init=init, step=step, use_graph=True)
        assert m.last_sampler_path == GROUP_PATH
        assert m._graph["key"][-1][1:3] == ("num_samples", G), "the graph key carries G"
        assert graph is None or m._graph["g"] is graph, "the same call must replay the captured graph"
        graph = m._graph["g"]
        assert torch.equal(got, eager), f"replay {rep} differs from the eager launch (max abs diff {(got - eager).abs().max().item():.3e})"
        assert int(m._graph["state"]["persist"]["sync"][2].item()) == 0
    # the default call afterwards, on the same planner, is what a fresh planner returns
    kw = dict(init_noise=d["init_noise"][:, 0].contiguous(), step_noise=d["step_noise"][:, :, 0].contiguous(), visual_tokens=tdev)
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
    after = m.compute_trajectory(*args, use_graph=True, **kw)
    assert m._graph["g"] is not graph and m.last_sampler_path == "persistent (a3d_dn_persist)"
    after_eager = m.compute_trajectory(*args, **kw)
    fresh, _ = make_planner(a3d, dev)
    want = fresh.compute_trajectory(*args, **kw)
    assert torch.equal(after, want) and torch.equal(after_eager, want)
    m._graph = None


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("B,Ln", [(3, 16), (2, 50)])
def test_the_default_path_is_untouched(planner, dev, B, Ln):
    m, _ = planner
    m._graph = None
    inp, tokens, d, tdev = cand_inputs(dev, 103, B, 1, Ln, 3)
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
    kw = dict(init_noise=d["init_noise"][:, 0].contiguous(), step_noise=d["step_noise"][:, :, 0].contiguous(), visual_tokens=tdev)
    for use_graph in (False, True):
        default = m.compute_trajectory(*args, use_graph=use_graph, **kw)
        assert m.last_sampler_path == "persistent (a3d_dn_persist)" and default.shape == (B, Ln, 7)
        none = m.compute_trajectory(*args, use_graph=use_graph, num_samples=None, **kw)
        one = sample_group(m, d, tdev, 1, use_graph=use_graph)
        assert m.last_sampler_path == GROUP_PATH and one.shape == (B, 1, Ln, 7)
        assert torch.isfinite(default).all() and torch.equal(none, default)
        assert torch.equal(one[:, 0], default), "num_samples=1 differs from the default call (max abs diff %.3e)" % (one[:, 0] - default).abs().max().item()
    m._graph = None


# ------------------------------------------------------------------------------------------------ 8
def _fallback_child(out_path):
    """A3D_DN_PERSIST=0 (read at import): num_samples on the per-phase launches and on the op-by-op path."""
    import importlib
    root = os.path.dirname(HERE)
    if root not in sys.path:
        sys.path.insert(0, root)
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    assert a3d.diffusion.DN_PERSIST is False
    m, _ = make_planner(a3d, dev)
    B, G, Ln = 3, 4, 16
    inp, tokens, d, tdev = cand_inputs(dev, 105, B, G, Ln, 3)
    got = sample_group(m, d, tdev, G, K=10)
    assert m.last_sampler_path == "per-phase fused launches", m.last_sampler_path
    ref = sample_replicated(m, d, tdev, G, K=10)
    scale_err("A3D_DN_PERSIST=0 num_samples vs replicated call (per-phase both)", got, ref, 5e-5)
    op = sample_group(m, d, tdev, G, K=10, fused=False)
    assert m.last_sampler_path == "op-by-op", m.last_sampler_path
    scale_err("A3D_DN_PERSIST=0 num_samples per-phase vs op-by-op", got, op, 2e-5)
    torch.save(got.cpu(), out_path)
    print("fallback-child ok")


def test_fallback_per_phase_in_a_fresh_process(planner, dev):
    m, _ = planner
    B, G, Ln = 3, 4, 16
    inp, tokens, d, tdev = cand_inputs(dev, 105, B, G, Ln, 3)
    here = sample_group(m, d, tdev, G, K=10)
    assert m.last_sampler_path == GROUP_PATH and abort_word(m) == 0
    env = dict(os.environ)
    env["A3D_DN_PERSIST"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        out_path = os.path.join(tmp, "per_phase.pt")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "fallback-child", out_path], env=env, capture_output=True, text=True,
                           timeout=600)
        print(p.stdout)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "fallback-child ok" in p.stdout
        there = torch.load(out_path)
    scale_err("num_samples persistent (group) vs per-phase (A3D_DN_PERSIST=0)", here, there, 5e-5)


@pytest.mark.parametrize("Ln,G", [(16, 4), (50, 2)])
def test_fallback_over_the_co_residency_limit(planner, dev, Ln, G):
    """More trajectories than 2 B G NT + 16 <= CU count admits: the call is served on the context expanded along the batch axis
    by the path the single-candidate call of that size takes (per-phase launches at L <= 16, op-by-op above)."""
    m, _ = planner
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    NT = -(-Ln // 16)
    B = (cus - 16) // (2 * NT * G) + 1
    assert 2 * B * G * NT + 16 > cus
    inp, tokens, d, tdev = cand_inputs(dev, 107, B, G, Ln, 3, ncam=1)
    got = sample_group(m, d, tdev, G, K=10)
    path = m.last_sampler_path
    assert path == ("per-phase fused launches" if Ln <= 16 else "op-by-op"), path
    ref = sample_replicated(m, d, tdev, G, K=10)
    assert m.last_sampler_path == path
    scale_err(f"over the limit (B={B} G={G} L={Ln}, {path}) num_samples vs replicated call", got, ref, 2e-5)
    # a sub-batch that fits, through the group entry
    sub = {k: v[:2].contiguous() for k, v in d.items() if k != "step_noise"}
    sub["step_noise"] = d["step_noise"][:, :2].contiguous()
    few = sample_group(m, sub, tdev[:2].contiguous(), G, K=10)
    assert m.last_sampler_path == GROUP_PATH and abort_word(m) == 0
    if Ln <= 16:
        scale_err(f"group entry vs per-phase fallback, scenes 0-1 of B={B} G={G} L={Ln}", few, got[:2], 5e-5)
    else:
        # persistent <-> op-by-op is not a bar the project states for one hop (5e-5 + 2e-5 through the per-phase path): reported
        print("[parity] group entry vs op-by-op fallback, scenes 0-1 of B=%d G=%d L=%d: max_abs_err=%.3e (reported)"
              % (B, G, Ln, (few - got[:2]).abs().max().item()))


# ------------------------------------------------------------------------------------------------ 9
def test_abort_stays_visible_with_candidates(planner, dev):
    """The bounded wait with candidate groups: with the A3D_DN_SPIN_LIMIT=0 hook of test_persistent_sampler_abort_is_visible_in_the_result
    (any wait longer than 128 polls gives up) the launch sets sync[2] and every candidate of every scene comes back NaN; the next
    launch is healthy.  Once, not in a loop."""
    m, _ = planner
    B, G, Ln = 2, 4, 16
    inp, tokens, d, tdev = cand_inputs(dev, 109, B, G, Ln, 2)
    good = sample_group(m, d, tdev, G, n_steps=10)
    assert m.last_sampler_path == GROUP_PATH and abort_word(m) == 0 and torch.isfinite(good).all()
    os.environ["A3D_DN_SPIN_LIMIT"] = "0"
    try:
        bad = sample_group(m, d, tdev, G, n_steps=10)
        aborted = abort_word(m)
    finally:
        del os.environ["A3D_DN_SPIN_LIMIT"]
    print(f"[parity] forced abort with num_samples={G}: abort word {aborted}, NaN entries {int(torch.isnan(bad).sum())} of {bad.numel()}")
    assert aborted != 0, "the test hook did not force an abort (no wait exceeded 128 polls?)"
    assert bad.shape == (B, G, Ln, 7)
    assert torch.isnan(bad[..., :3]).all() and torch.isnan(bad).any(-1).all(), "an aborted group launch returned finite poses"
    again = sample_group(m, d, tdev, G, n_steps=10)
    assert abort_word(m) == 0 and torch.equal(again, good)


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "fallback-child":
    _fallback_child(sys.argv[2])
