"""GPU tests of pinned waypoints: the kernel (a3d_traj_pins) against the torch restatement of tests/pins_ref.py, bit for bit, and
compute_trajectory(pins=...) / Actioner.predict(pins=...) on every sampler path, under every scheduler, against the CPU oracle's loop,
through graph replay, with the keyword off, and together with the guide.

The planner is the golden-weight one of tests/test_multi_candidate_gpu.py (E = 120, 3 cameras); B = 2 scenes, G = 3 candidates,
L = 8 and 16, pad_last = 3 (scene 1 only), K = 6 steps.  Bars: torch.equal wherever the same kernels run on the same bits; 5e-5 of
scale persistent <-> per-phase and group <-> replicated, 2e-5 per-phase <-> op-by-op, 3e-4 against the oracle (the bars of
tests/test_multi_candidate_gpu.py).

What a trace entry holds at a pinned element.  Every sampler step in-paints the network OUTPUT (x0 = cond_data where the mask is set)
and then applies its update x_prev = c0 clip(x0) + c1 x_t + c2 z; only the terminal step returns the in-painted output itself.  So the
LAST entry of a K-step schedule equals cond_data at every pinned element exactly (torch.equal), and entry i < K - 1 equals the update
of the previous entry with x0 = cond_data: that recurrence is evaluated here in float64 from the schedule's own fp32 tables and has
to hold within 4 fp32 roundings of the three products' magnitudes, 4 * 2^-24 (|c0 x0| + |c1 x_t| + |c2 z|) -- nothing the network
computes enters a pinned element at any step.  (Equality with cond_data at EVERY entry cannot hold for the non-terminal steps of any
sampler here, for the start and goal rows no more than for pins.)"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))             # the fallback child runs this file as a script, without conftest
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import common as C  # noqa: E402
import pins_ref as PR  # noqa: E402
from test_multi_candidate_gpu import T, H, cand_inputs, make_planner, sample_group, sample_replicated, scale_err  # noqa: E402

pytestmark = pytest.mark.gpu

B_, G_, K_, PAD = 2, 3, 6, 3
LENGTHS = [8, 16]
SCHEDULERS = [("ddpm", 0.0), ("ddim", 0.0), ("dpm++", 0.0)]


def bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


# ------------------------------------------------------------------------------------------------ 1: the kernel
def random_poses(g, n, Dp, lo, hi):
    """pose rows inside the workspace; quaternions of norm 1.7 (the row map normalises), extras in [0, 1)"""
    q = torch.randn(*n, 4, generator=g)
    xyz = lo + 0.15 * (hi - lo) + torch.rand(*n, 3, generator=g) * 0.7 * (hi - lo)
    return torch.cat([xyz, 1.7 * q / q.norm(dim=-1, keepdim=True), torch.rand(*n, Dp - 7, generator=g)], -1)


def pin_set(kind, L, pads):
    """(index (B, P), channels (B, P) uint8) of the named set; per scene last = L - pad - 1 >= 4.
    merge: an interior pose pin (slot 0, row 2); a position-only and a rotation-only pin on row 3 (slots 1, 2: they merge); slot 3 on
           row 2 again with another pose and all channels (the higher slot wins); an unused slot (-1)
    drop:  an interior pose pin; a pin on row 0; on the goal row; on a padded row (one past the end for an unpadded scene); unused
    all:   both in one launch, and a gripper-only pin on row 1 (P = 9)"""
    idx, ch = [], []
    for pad in pads:
        last = L - pad - 1
        assert last >= 4
        beyond = last + 2 if pad >= 2 else L
        merge, drop = [2, 3, 3, 2, -1], [2, 0, last, beyond, -1]
        idx.append({"merge": merge, "drop": drop, "all": merge + drop[1:4] + [1]}[kind])
        ch.append({"merge": [3, 1, 2, 7, 3], "drop": [3, 3, 3, 3, 3], "all": [3, 1, 2, 7, 3, 3, 3, 3, 4]}[kind])
    return torch.tensor(idx, dtype=torch.int32), torch.tensor(ch, dtype=torch.uint8)


def applied_want(kind, B, use_goal):
    return {"merge": [[1, 1, 1, 1, 0]], "drop": [[1, 0, 0 if use_goal else 1, 0, 0]],
            "all": [[1, 1, 1, 1, 0, 0, 0 if use_goal else 1, 0, 1]]}[kind] * B


KERNEL_CASES = [  # kind, B, G, L, Dp, use_goal, with_traj
    ("merge", 2, 3, 8, 8, 1, True), ("drop", 2, 3, 8, 8, 1, True), ("drop", 2, 3, 8, 8, 0, True), ("merge", 2, 3, 8, 8, 1, False),
    ("all", 2, 3, 8, 8, 1, True), ("all", 2, 3, 8, 8, 0, False),
    ("all", 2, 3, 8, 7, 1, True),                                   # no extras: the gripper bit selects no column
    ("all", 3, 70, 9, 8, 1, True),                                  # more candidates than workgroup rows (64): the g loop strides
    ("all", 2, 2, 300, 8, 0, True),                                 # more rows than threads: the padding count and the element loop stride
]


@pytest.mark.parametrize("kind,B,G,L,Dp,use_goal,with_traj", KERNEL_CASES)
def test_kernel_equals_the_twin(a3d, dev, kind, B, G, L, Dp, use_goal, with_traj):
    from test_actioner_gpu import guarded, guards_intact
    D_ = a3d.diffusion
    D = Dp + 2
    g = torch.Generator().manual_seed(7)
    bounds = torch.tensor(C.DIFFUSION_BOUNDS, dtype=torch.float32)
    lo, hi = bounds[0], bounds[1]
    pads = [0] * (B // 2) + [PAD] * (B - B // 2)
    tmask = torch.zeros(B, L, dtype=torch.bool)
    for b, pad in enumerate(pads):
        tmask[b, L - pad:] = pad > 0
    curr, goal = random_poses(g, (B,), Dp, lo, hi), random_poses(g, (B,), Dp, lo, hi)
    noise = torch.randn(B * G, L, D, generator=g)
    index, channels = pin_set(kind, L, pads)
    P = index.shape[1]
    poses = random_poses(g, (B, P), Dp, lo, hi)
    bd, nd, td = bounds.to(dev), noise.to(dev), tmask.to(dev)
    _, _, cond0, cmask0, _, traj0 = D_.traj_condition(curr.to(dev), goal.to(dev), bd, td, nd, G, bool(use_goal))
    # the launch writes into guarded copies
    n = B * G * L * D
    bufs = {"cond": guarded(n, torch.float32, dev), "cmask": guarded(n, torch.uint8, dev), "traj": guarded(n, torch.float32, dev)}
    view = lambda k: bufs[k][1].view(B * G, L, D)
    view("cond").copy_(cond0), view("cmask").copy_(cmask0), view("traj").copy_(traj0)
    pins = {"poses": poses.to(dev), "index": index.to(dev), "channels": channels.to(dev)}
    applied = D_.traj_pins(view("cond"), view("cmask"), view("traj") if with_traj else None, nd if with_traj else None, pins, bd, td, G,
                           bool(use_goal))
    torch.cuda.synchronize()
    assert all(guards_intact(w, n) for w, _ in bufs.values()), "a3d_traj_pins wrote outside its tensors"
    # the twin, on the tensors before the call and the pins converted by the existing pose_to_signal
    sig = D_.pose_to_signal(poses.to(dev), bd).cpu()
    cd, cm, tr, ap = PR.pins_ref(cond0.cpu(), cmask0.cpu(), traj0.cpu(), noise, sig, index, channels, tmask, G, bool(use_goal))
    assert ap.tolist() == applied_want(kind, B, use_goal), "the case does not hold what it is meant to"
    assert torch.equal(applied.cpu(), ap)
    assert torch.equal(bits(view("cond").cpu()), bits(cd)) and torch.equal(view("cmask").cpu(), cm)
    assert torch.equal(bits(view("traj").cpu()), bits(tr if with_traj else traj0.cpu()))
    # unpinned elements keep the bits they had; pinned ones (rows 1 .. last - 1, where the mask was 0) changed
    pinned = cm != cmask0.cpu()
    assert int(pinned.sum()) > 0 and not bool(pinned[:, 0].any())
    for got, before in ((view("cond"), cond0), (view("traj"), traj0)):
        assert torch.equal(bits(got.cpu())[~pinned], bits(before.cpu())[~pinned])
    assert torch.equal(view("cmask").cpu()[~pinned], cmask0.cpu()[~pinned])
    if kind != "drop":
        # the merged row: position of slot 1, rotation of slot 2; the contested row: slot 3 (all channels) over slot 0
        c = view("cond").cpu().view(B, G, L, D)
        for b in range(B):
            assert torch.equal(c[b, :, 3, :3], sig[b, 1, :3].expand(G, 3)) and torch.equal(c[b, :, 3, 3:9], sig[b, 2, 3:9].expand(G, 6))
            assert torch.equal(c[b, :, 2], sig[b, 3].expand(G, D)) and not torch.equal(sig[b, 3], sig[b, 0])
            assert not bool(cm.view(B, G, L, D)[b, :, 3, 9:].any())
    # a channel name in place of the tensor: the same launch with one mask for every slot
    if kind == "drop":
        view("cond").copy_(cond0), view("cmask").copy_(cmask0), view("traj").copy_(traj0)
        again = D_.traj_pins(view("cond"), view("cmask"), None, None, D_.TrajectoryPins(poses.to(dev), index.to(dev), "pose"), bd, td, G,
                             bool(use_goal))
        assert torch.equal(again.cpu(), ap) and torch.equal(bits(view("cond").cpu()), bits(cd)) and torch.equal(view("cmask").cpu(), cm)


def test_kernel_argument_errors(a3d, dev):
    """A3D_ERR_ARG (-22) with a message, before anything is launched; device pointers of real tensors."""
    lib = a3d.lib.load()
    B, G, P, L, Dp = 2, 3, 5, 8, 8
    t = {k: torch.zeros(n, device=dev, dtype=dt) for k, n, dt in (
        ("poses", B * P * Dp, torch.float32), ("index", B * P, torch.int32), ("channels", B * P, torch.uint8), ("bounds", 6, torch.float32),
        ("tmask", B * L, torch.uint8), ("init_noise", B * G * L * (Dp + 2), torch.float32), ("cond_data", B * G * L * (Dp + 2), torch.float32),
        ("cond_mask", B * G * L * (Dp + 2), torch.uint8), ("traj", B * G * L * (Dp + 2), torch.float32), ("applied", B * P, torch.uint8))}

    def rc(**kw):
        a = dict(poses=t["poses"].data_ptr(), ldp=Dp, index=t["index"].data_ptr(), channels=t["channels"].data_ptr(),
                 bounds=t["bounds"].data_ptr(), tmask=t["tmask"].data_ptr(), init_noise=t["init_noise"].data_ptr(),
                 cond_data=t["cond_data"].data_ptr(), cond_mask=t["cond_mask"].data_ptr(), traj=t["traj"].data_ptr(),
                 applied=t["applied"].data_ptr(), B=B, G=G, P=P, L=L, Dp=Dp, use_goal=1)
        a.update(kw)
        return lib.a3d_traj_pins(*a.values(), a3d.lib.stream())

    for kw in ([{k: None} for k in ("poses", "index", "channels", "bounds", "tmask", "cond_data", "cond_mask", "applied")]
               + [dict(init_noise=None), dict(P=0), dict(P=33), dict(Dp=6), dict(Dp=31, ldp=31), dict(ldp=7), dict(B=0), dict(G=0), dict(L=0)]):
        assert rc(**kw) == -22, kw
        assert "a3d_traj_pins" in a3d.lib.last_error(), kw
    with pytest.raises(RuntimeError, match="a3d_traj_pins"):
        a3d.lib.call("a3d_traj_pins", None, *([0] * 17))
    assert rc() == 0 and rc(traj=None, init_noise=None) == 0 and rc(traj=None) == 0
    torch.cuda.synchronize()
    assert not bool(t["applied"].any()) and not bool(t["cond_mask"].any())      # all-zero channel masks: nothing applied, nothing written


# ------------------------------------------------------------------------------------------------ 2: the planner
@pytest.fixture(scope="module")
def planner(a3d, dev):
    return make_planner(a3d, dev)


_CASES = {}


def case(dev, Ln, seed=131):
    """inputs of one shape (cand_inputs) and its pins, P = 4 per scene from the golden trajectory of the scene: slot 0 a pose pin on
    row 2, slot 1 position-only on row 3, slot 2 rotation-only on row 1, slot 3 on row L - 1 (the goal row of scene 0, a padded row
    of scene 1: dropped)."""
    if (Ln, seed) not in _CASES:
        inp, tokens, d, tdev = cand_inputs(dev, seed, B_, G_, Ln, PAD)
        assert inp["mask"].sum(1).tolist() == [0, PAD]
        rows = [2, 3, 1, Ln - 1]
        poses = inp["trajectory"][:, [5, 2, 3, 1]].clone()             # rows of the golden trajectory, put elsewhere
        poses[..., :3] += 0.02
        pins = {"poses": poses.to(dev), "index": torch.tensor([rows] * B_, device=dev),
                "channels": torch.tensor([[3, 1, 2, 3]] * B_, dtype=torch.uint8, device=dev)}
        _CASES.clear()
        _CASES[(Ln, seed)] = (inp, tokens, d, tdev, pins)
    return _CASES[(Ln, seed)]


def conditioning(a3d, m, d, pins, G):
    """(cond_data, cond_mask bool (B G, L, D), applied) of the call, from the two public launches"""
    D_ = a3d.diffusion
    _, _, cond, cmask, _, _ = D_.traj_condition(d["curr_gripper"], d["goal_gripper"], m.gripper_loc_bounds, d["mask"], None, G, True)
    n0 = int(cmask.sum())
    applied = D_.traj_pins(cond, cmask, None, None, pins, m.gripper_loc_bounds, d["mask"], G, True)
    assert int(cmask.sum()) == n0 + B_ * G * (9 + 3 + 6)               # a pose, a position and a rotation per trajectory
    return cond, cmask.bool(), applied


def round_trip(a3d, m, pose):
    D_ = a3d.diffusion
    return D_.signal_to_pose(D_.pose_to_signal(pose, m.gripper_loc_bounds), m.gripper_loc_bounds)


@pytest.mark.parametrize("scheduler,eta", SCHEDULERS, ids=[s for s, _ in SCHEDULERS])
@pytest.mark.parametrize("Ln", LENGTHS)
def test_every_step_in_paints_the_pins(planner, a3d, dev, Ln, scheduler, eta):
    m, _ = planner
    inp, tokens, d, tdev, pins = case(dev, Ln)
    cond, cm, applied = conditioning(a3d, m, d, pins, G_)
    final, trace = sample_group(m, d, tdev, G_, K_, scheduler, eta, return_trace=True, pins=pins)
    assert len(trace) == K_ and type(m.last_pins) is a3d.Pins
    assert torch.equal(m.last_pins.applied, applied) and applied.tolist() == [[1, 1, 1, 0]] * B_
    assert torch.equal(m.last_pins.index, pins["index"].int())
    flat = [x.reshape(B_ * G_, Ln, 9) for x in trace]
    # the terminal step returns the in-painted output: cond_data exactly, at every pinned element of every candidate
    assert torch.equal(bits(flat[-1][cm]), bits(cond[cm]))
    # every step before it: the schedule's update of the previous entry with x0 = cond_data, whatever the network returned
    sc = m.schedule(dev, K_, scheduler, eta)
    x0 = cond.double().clamp(-1, 1)
    prev = d["init_noise"].reshape(B_ * G_, Ln, 9).double() + cond.double()
    pos = (torch.arange(9, device=dev) < 3).expand_as(cond)
    worst = 0.0
    for i in range(K_ - 1):
        cf = torch.where(pos[..., None], sc.coef_pos[i].double(), sc.coef_rot[i].double())         # (B G, L, 9, 3)
        z = torch.zeros_like(prev) if sc.noise_free else d["step_noise"][i].reshape(B_ * G_, Ln, 9).double()
        a, b, c = cf[..., 0] * x0, cf[..., 1] * prev, cf[..., 2] * z
        want, bar = a + b + c, 4 * 2.0 ** -24 * (a.abs() + b.abs() + c.abs())
        err = (flat[i].double() - want).abs()
        worst = max(worst, float((err[cm] / bar[cm].clamp_min(1e-30)).max()))
        assert bool((err[cm] <= bar[cm]).all()), f"step {i}: a pinned element left the in-painted update ({worst:.2f} of the bar)"
        prev = flat[i].double()
    print(f"[parity] L={Ln} {scheduler}: pinned elements of the non-terminal entries vs the in-painted update: worst {worst:.2f} of the bar")
    # the pose-pinned row, the position-only and the rotation-only rows of the result; the untraced call returns the same
    want = round_trip(a3d, m, pins["poses"])
    assert torch.equal(final[:, :, 2], want[:, None, 0].expand(B_, G_, 7))
    assert torch.equal(final[:, :, 3, :3], want[:, None, 1, :3].expand(B_, G_, 3))
    assert not torch.equal(final[:, :, 3, 3:], want[:, None, 1, 3:].expand(B_, G_, 4))
    got = sample_group(m, d, tdev, G_, K_, scheduler, eta, pins=pins)
    scale_err(f"pins L={Ln} {scheduler} one launch vs traced", got, final, 1e-6)
    assert torch.equal(got[:, :, 2], final[:, :, 2])
    # candidates differ away from the pins
    assert not torch.equal(final[:, 0, 4], final[:, 1, 4])


@pytest.mark.parametrize("Ln", LENGTHS)
def test_both_conditioning_paths_give_the_same_bits(planner, dev, Ln):
    m, _ = planner
    inp, tokens, d, tdev, pins = case(dev, Ln)
    for G in (G_, None):
        if G is None:
            run = lambda **kw: m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"],
                                                    init_noise=d["init_noise"][:, 0].contiguous(), visual_tokens=tdev,
                                                    step_noise=d["step_noise"][:K_, :, 0].contiguous(), num_inference_steps=K_,
                                                    return_trace=True, pins=pins, **kw)
        else:
            run = lambda **kw: sample_group(m, d, tdev, G, K_, return_trace=True, pins=pins, **kw)
        (a, ta), ap = run(fused_conditioning=False), m.last_pins.applied
        (b, tb), bp = run(fused_conditioning=True), m.last_pins.applied
        assert torch.equal(bits(a), bits(b)) and torch.equal(ap, bp) and all(torch.equal(bits(x), bits(y)) for x, y in zip(ta, tb))
        (c, _) = run(fused_conditioning=True, fused=False)             # and on the expanded op-by-op path
        (e, _) = run(fused_conditioning=False, fused=False)
        assert m.last_sampler_path == "op-by-op" and torch.equal(bits(c), bits(e))


@pytest.mark.parametrize("Ln", LENGTHS)
def test_group_path_equals_the_replicated_call(planner, a3d, dev, Ln):
    m, _ = planner
    inp, tokens, d, tdev, pins = case(dev, Ln)
    got = sample_group(m, d, tdev, G_, K_, pins=pins)
    assert m.last_sampler_path == "persistent (a3d_dn_persist_group)"
    rep_pins = {k: v.repeat_interleave(G_, 0) for k, v in pins.items()}
    ref = sample_replicated(m, d, tdev, G_, K_, pins=rep_pins)
    assert m.last_pins.applied.shape == (B_ * G_, 4)
    scale_err(f"pins L={Ln} num_samples={G_} vs the replicated call", got, ref, 5e-5)
    assert torch.equal(got[:, :, 2], ref[:, :, 2])


def test_multi_round_head_keeps_the_pins(a3d, dev):
    """attn_rounds = 2 x feat_scales_to_use = 2 (tests/golden/diffusion_multi.pt): every step evaluates the full head and ends in
    a3d_ddpm_step_sched, which reads the same two tensors -- the pinned row of the result is the pin, on both conditioning paths."""
    from test_oracle_golden import load, multi_head_inputs
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
    B, Ln = inp["mask"].shape
    assert Ln - int(inp["mask"].sum(1).max()) - 1 >= 3                 # rows 1 and 2 lie before every scene's goal row
    pins = {"poses": d["trajectory"][:, [3, 4]].contiguous(), "index": torch.tensor([[2, 1]] * B, device=dev), "channels": "pose"}
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])
    kw = dict(init_noise=d["init_noise"], step_noise=d["step_noise"][:4].contiguous(), visual_tokens=[f.to(dev) for f in feats],
              num_inference_steps=4)
    got = m.compute_trajectory(*args, pins=pins, **kw)
    assert m.last_sampler_path == "multi-round" and m.last_pins.applied.tolist() == [[1, 1]] * B
    assert torch.equal(got[:, [2, 1]], round_trip(a3d, m, pins["poses"]))
    fused = m.compute_trajectory(*args, pins=pins, fused_conditioning=True, **kw)
    assert torch.equal(bits(fused), bits(got))
    plain = m.compute_trajectory(*args, **kw)
    assert m.last_pins is None and not torch.equal(plain[:, 1:3], got[:, 1:3])


def _paths_child(out_path):
    """A3D_DN_PERSIST=0 (read at import): the pinned call on the per-phase launches and on the op-by-op path (context expanded along
    the batch axis, per-scene pins expanded by the kernel)."""
    import importlib
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    assert a3d.diffusion.DN_PERSIST is False
    m, _ = make_planner(a3d, dev)
    out = {}
    for Ln in LENGTHS:
        inp, tokens, d, tdev, pins = case(dev, Ln)
        got = sample_group(m, d, tdev, G_, K_, pins=pins)
        assert m.last_sampler_path == "per-phase fused launches", m.last_sampler_path
        op = sample_group(m, d, tdev, G_, K_, pins=pins, fused=False)
        assert m.last_sampler_path == "op-by-op", m.last_sampler_path
        scale_err(f"A3D_DN_PERSIST=0 pins L={Ln} per-phase vs op-by-op", got, op, 2e-5)
        want = round_trip(a3d, m, pins["poses"])[:, None, 0].expand(B_, G_, 7)
        assert torch.equal(got[:, :, 2], want) and torch.equal(op[:, :, 2], want)
        out[Ln] = got.cpu()
    torch.save(out, out_path)
    print("paths-child ok")


def test_sampler_paths_agree_with_pins(planner, dev):
    m, _ = planner
    here = {}
    for Ln in LENGTHS:
        inp, tokens, d, tdev, pins = case(dev, Ln)
        here[Ln] = sample_group(m, d, tdev, G_, K_, pins=pins)
        assert m.last_sampler_path == "persistent (a3d_dn_persist_group)"
    env = dict(os.environ)
    env["A3D_DN_PERSIST"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        out_path = os.path.join(tmp, "per_phase.pt")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "paths-child", out_path], env=env, capture_output=True, text=True,
                           timeout=600)
        print(p.stdout)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "paths-child ok" in p.stdout
        there = torch.load(out_path)
    for Ln in LENGTHS:
        scale_err(f"pins L={Ln} persistent (group) vs per-phase (A3D_DN_PERSIST=0)", here[Ln], there[Ln], 5e-5)
        assert torch.equal(here[Ln][:, :, 2].cpu(), there[Ln][:, :, 2])


@pytest.mark.parametrize("Ln", LENGTHS)
def test_pinned_loop_vs_oracle(planner, dev, Ln):
    """The first K steps of the full chain with pins against the oracle's loop (make_conditioning + the twin's rule, head_forward,
    step_with_inpaint) on every candidate of the unpadded and the padded scene."""
    m, P = planner
    inp, tokens, d, tdev, pins = case(dev, Ln)
    final, trace = sample_group(m, d, tdev, G_, n_steps=K_, return_trace=True, pins=pins)
    got = sample_group(m, d, tdev, G_, n_steps=K_, pins=pins)
    assert m.last_sampler_path == "persistent (a3d_dn_persist_group)"
    scale_err(f"pins L={Ln} full chain, one launch vs traced", got, final, 1e-6)
    rep = {k: v.repeat_interleave(G_, 0) for k, v in inp.items() if k not in ("init_noise", "step_noise")}
    rep["init_noise"] = inp["init_noise"].reshape(B_ * G_, Ln, 9)
    rep["step_noise"] = inp["step_noise"].reshape(T, B_ * G_, Ln, 9)
    cpu = {k: v.cpu().repeat_interleave(G_, 0) for k, v in pins.items()}
    sub = list(range(B_ * G_))
    ofinal, otrace = PR.oracle_pinned_loop(P, rep, tokens.repeat_interleave(G_, 0), sub, cpu["poses"], cpu["index"], cpu["channels"], K_, H,
                                           C.DIFFUSION_BOUNDS)
    tag = f"pins L={Ln} full chain, {K_} steps"
    scale_err(tag + " last state vs oracle", trace[-1].reshape(B_ * G_, Ln, 9), otrace[-1], 3e-4)
    o = got.reshape(B_ * G_, Ln, 7).cpu()
    scale_err(tag + " sampled xyz vs oracle", o[..., :3], ofinal[..., :3], 3e-4)
    sign = torch.sign((o[..., 3:] * ofinal[..., 3:]).sum(-1, keepdim=True))
    scale_err(tag + " sampled quaternion vs oracle", o[..., 3:] * sign, ofinal[..., 3:], 3e-4)


def test_replay_needs_no_recapture(planner, dev):
    m, _ = planner
    Ln = 16
    inp, tokens, d, tdev, pins = case(dev, Ln)
    other = {"poses": inp["trajectory"][:, [7, 8]].to(dev), "index": torch.tensor([[4, 1]] * B_, device=dev), "channels": ("position", "rotation")}
    m._graph = None
    graph = None
    for name, p in (("pins A", pins), ("pins B, another P", other), ("no pins", None)):
        eager = sample_group(m, d, tdev, G_, K_, pins=p)
        eager_pins = m.last_pins
        got = sample_group(m, d, tdev, G_, K_, pins=p, use_graph=True)
        assert torch.equal(bits(got), bits(eager)), f"{name}: the replay differs from the eager call"
        assert (m.last_pins is None) == (p is None) and (p is None or torch.equal(m.last_pins.applied, eager_pins.applied))
        assert graph is None or m._graph["g"] is graph, f"{name}: the call recaptured"
        graph = m._graph["g"]
    a, b = sample_group(m, d, tdev, G_, K_, pins=pins, use_graph=True), sample_group(m, d, tdev, G_, K_, pins=other, use_graph=True)
    assert m._graph["g"] is graph and not torch.equal(a, b)
    m._graph = None


@pytest.mark.parametrize("Ln", LENGTHS)
def test_off_switch(planner, dev, Ln):
    m, _ = planner
    inp, tokens, d, tdev, pins = case(dev, Ln)
    sample_group(m, d, tdev, G_, K_, pins=pins)
    assert m.last_pins is not None
    for kw in (dict(), dict(fused_conditioning=True), dict(fused=False)):
        base = sample_group(m, d, tdev, G_, K_, **kw)
        assert m.last_pins is None
        none = sample_group(m, d, tdev, G_, K_, pins=None, **kw)
        assert m.last_pins is None and torch.equal(bits(none), bits(base))


# ------------------------------------------------------------------------------------------------ 3: the guide, the Actioner
def test_the_guide_leaves_a_position_pin_alone(planner, a3d, dev):
    """guide = 1.0: the position-pinned row 2 sits 1 cm from a point of the cloud, well inside the 5 cm margin, and is not pushed; the
    rows next to it are free and move.  (The golden cloud is dense: ~40 points within 5 cm of any place in the workspace.)"""
    m, _ = planner
    Ln = 16
    inp, tokens, d, tdev, _ = case(dev, Ln)
    poses = inp["trajectory"][:, [2]].clone()
    poses[:, 0, :3] = inp["pcd"][:, 0, :, 100, 100] + torch.tensor([0.01, 0.0, 0.0])
    pins = {"poses": poses.to(dev), "index": torch.tensor([[2]] * B_, device=dev), "channels": "position"}
    plain = sample_group(m, d, tdev, G_, K_, "ddim", 0.0, pins=pins)
    guided = sample_group(m, d, tdev, G_, K_, "ddim", 0.0, pins=pins, guide=1.0)
    near = m.last_guidance.nearest
    assert m.last_guidance.steps == (3, 4, 5) and near.shape == (B_, G_, Ln)
    want = round_trip(a3d, m, pins["poses"])[:, None, 0, :3].expand(B_, G_, 3)
    assert torch.equal(guided[:, :, 2, :3], want) and torch.equal(plain[:, :, 2, :3], want)
    assert bool((near[:, :, 2] < 0.0101).all()), "the pinned row is not inside the margin: the case shows nothing"
    pushed = near[:, :, [1, 3]] < 0.05
    print(f"[guide] nearest at the pinned row {near[:, :, 2].max().item():.4f} m; neighbours inside the margin at the last step: "
          f"{int(pushed.sum())} of {pushed.numel()}")
    assert bool(pushed.any())
    moved = (guided[:, :, [1, 3], :3] != plain[:, :, [1, 3], :3]).any(-1)
    assert bool(moved[pushed].all()), "a free neighbour inside the margin was not moved"
    # only the terminal step guided: the result is the unguided one but for the pushed rows, so every row can be held against it
    last = sample_group(m, d, tdev, G_, K_, "ddim", 0.0, pins=pins, guide={"push": 1.0, "start": 0.9})
    near = m.last_guidance.nearest
    assert m.last_guidance.steps == (K_ - 1,)
    free = torch.zeros(B_, G_, Ln, dtype=torch.bool, device=dev)
    free[0, :, 1:Ln - 1], free[1, :, 1:Ln - PAD - 1] = True, True     # clear_skip = (1, 1): all but the start and the goal row
    inside = (near < 0.05) & free
    moved = (last[..., :3] != plain[..., :3]).any(-1)
    print(f"[guide] terminal step only: {int(inside.sum())} of {int(free.sum())} free rows inside the margin, "
          f"{int(inside[:, :, [1, 3]].sum())} of them next to the pin")
    assert bool(inside[:, :, 2].all()) and not bool(moved[:, :, 2].any()), "the position-pinned row was pushed"
    inside[:, :, 2] = False
    assert bool(inside[:, :, [1, 3]].any()) and torch.equal(moved, inside), "exactly the free, unpinned rows inside the margin move"


def test_actioner_replans_with_a_committed_prefix(a3d, dev):
    """predict, then predict again from the pose two steps into the plan with rows 3..5 of the old plan pinned on rows 1..3"""
    import test_actioner_gpu as A
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        kp = A.make_keypose(a3d, dev)
        pl = A.make_planner(a3d, dev, backbone_of=kp)
        instr = torch.randn(1, 53, 512, generator=torch.Generator().manual_seed(77)).to(dev)
        o = A.observation(dev, 71, 2, 16)
        kw = dict(num_inference_steps=4, scheduler="ddim")
        act = a3d.Actioner(kp, pl, predict_trajectory=True)
        act.set_instruction(instr)
        prev = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], **kw)["trajectory"]
        assert prev.shape == (2, 16, 7) and act.last_pins is None
        gripper = o["gripper"].clone()
        gripper[:, -1, :7] = prev[:, 2]                             # where the robot is now
        out = act.predict(o["rgbs"], o["pcds"], gripper, None, o["mask"], pins=a3d.prefix_pins(prev, 2, 3), **kw)["trajectory"]
        want = round_trip(a3d, pl, prev[:, 3:6])
        assert torch.equal(out[:, 1:4], want), "the committed rows moved (max abs diff %.3e)" % (out[:, 1:4] - want).abs().max().item()
        assert act.last_pins is pl.last_pins and act.last_pins.applied.tolist() == [[1, 1, 1]] * 2
        assert act.last_pins.index.tolist() == [[1, 2, 3]] * 2
        assert not torch.equal(out[:, 4:8], prev[:, 6:10])          # the rest is sampled anew
        act.predict(o["rgbs"], o["pcds"], gripper, None, o["mask"], **kw)
        assert act.last_pins is None
    finally:
        torch.backends.cudnn.deterministic = old


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "paths-child":
    _paths_child(sys.argv[2])
