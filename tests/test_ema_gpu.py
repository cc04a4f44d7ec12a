"""EMA of the weights on the device: a3d_adamw_ema_step against a3d_adamw_step (bit for bit) and the float64
recurrence of tests/ema_ref.py, a3d_swap_f32 at every alignment, the EMA inside a replayed step graph, sampling under
`optimizer.ema_weights()`, and the keypose driver end to end with ema_decay."""
import os
import pickle
import random
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import common as C  # noqa: E402
import ema_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def within_bar(name, got, ref64, atol=1e-6, rtol=1e-6):
    """|got - ref| <= atol + rtol |ref| element-wise (the bar test_adamw_matches_torch holds p to); prints the worst ratio first."""
    err = (got.double().cpu() - ref64.cpu()).abs()
    bar = atol + rtol * ref64.cpu().abs()
    worst = (err / bar).max().item() if err.numel() else 0.0
    print(f"[parity] {name}: max_abs_err={err.max().item() if err.numel() else 0.0:.3e} worst err/bar={worst:.3f}")
    assert worst <= 1.0, f"{name}: error {worst:.3f} x the bar {atol} + {rtol} |x|"


# ------------------------------------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("decay,warmup", [(0.999, 10), (0.9, 0), (0.9999, 10)])
def test_adamw_ema_step_matches_plain_step_and_float64_recurrence(a3d, dev, decay, warmup):
    """The segment layout of test_adamw_matches_torch (a bias, a matrix with a dead row, a never-used tensor, a tensor that joins at
    step 3), lr = 1e-2 so that the average visibly lags p, 8 steps."""
    L = a3d.lib
    g = torch.Generator().manual_seed(2)
    shapes = [(37,), (40, 25), (64,), (48,)]
    sizes = [int(np.prod(s)) for s in shapes]
    off = [0]
    for k in sizes:
        off.append(off[-1] + k)
    n, nseg, steps, lr = off[-1], len(shapes), 8, 1e-2
    p0 = torch.cat([torch.randn(s, generator=g).reshape(-1) for s in shapes]).to(dev)
    seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
    seg_id = torch.repeat_interleave(torch.arange(nseg), torch.tensor(sizes)).to(dev)

    def fresh():
        return dict(p=p0.clone(), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev), step=torch.zeros(1, device=dev),
                    seg=torch.zeros((nseg, 4), device=dev))
    A, Bs = fresh(), fresh()                              # A: a3d_adamw_step, Bs: a3d_adamw_ema_step
    ema = p0.clone()
    ema_state = torch.zeros(4, device=dev)
    ema64 = p0.double()
    lag = 0.0
    for it in range(steps):
        gr = [torch.randn(s, generator=g) for s in shapes]
        gr[1][7] = 0.0
        gd = torch.cat([gr[0].reshape(-1), gr[1].reshape(-1), torch.zeros(sizes[2]),
                        gr[3].reshape(-1) if it >= 2 else torch.zeros(sizes[3])]).to(dev)
        L.call("a3d_adamw_step", A["p"].data_ptr(), gd.data_ptr(), A["m"].data_ptr(), A["v"].data_ptr(), A["step"].data_ptr(),
               seg_off.data_ptr(), A["seg"].data_ptr(), nseg, n, sizes[0], lr, 0.9, 0.999, 1e-8, 0.0, 5e-4, 1.0, L.stream())
        L.call("a3d_adamw_ema_step", Bs["p"].data_ptr(), gd.data_ptr(), Bs["m"].data_ptr(), Bs["v"].data_ptr(), ema.data_ptr(),
               Bs["step"].data_ptr(), seg_off.data_ptr(), Bs["seg"].data_ptr(), ema_state.data_ptr(), nseg, n, sizes[0], lr, 0.9, 0.999,
               1e-8, 0.0, 5e-4, 1.0, decay, float(warmup), L.stream())
        # (a) the AdamW half, bit for bit, after every step
        for k in ("p", "m", "v", "step", "seg"):
            assert torch.equal(A[k], Bs[k]), f"step {it + 1}: {k} differs from a3d_adamw_step"
        # (b) the float64 recurrence, driven by the device's own p, on the elements of active parameters
        active = Bs["seg"][:, 1][seg_id] == 1.0
        ema64 = R.ema_update(ema64, Bs["p"], it + 1, decay, warmup, active=active)
        within_bar(f"ema after step {it + 1} (decay {decay}, warm-up {warmup})", ema, ema64)
        # the weight the kernel left: the fp32 evaluation of ema_ref's formula (1 - fp32(decay) carries decay's rounding), 2 ulps
        w32 = float(np.float32(1.0) - np.float32(decay))
        if warmup:
            w32 = max(w32, float((np.float32(warmup) - np.float32(1.0)) / (np.float32(warmup) + np.float32(it + 1))))
        assert abs(ema_state[0].item() - w32) <= 2.4e-7 * w32, (ema_state[0].item(), w32)
        # (c) never used: untouched; (d) the late joiner: its p0 until step 3
        assert torch.equal(ema[off[2]:off[3]], p0[off[2]:off[3]]), "the never-used parameter's average moved"
        if it < 2:
            assert torch.equal(ema[off[3]:], p0[off[3]:]), "the late joiner's average moved before it joined"
        else:
            assert not torch.equal(ema[off[3]:], p0[off[3]:])
        lag = (ema - Bs["p"]).abs()[:off[2]].max().item()
    print(f"[parity] lag max|ema - p| after {steps} steps: {lag:.3e}")
    assert lag > 1e-3, "the average does not lag p: the check above would be vacuous"
    # (e) the EMA's own counter; slots 2, 3 stay zero
    assert ema_state[1].item() == float(steps) and ema_state[2:].abs().sum().item() == 0.0
    assert Bs["seg"][:, 0].cpu().tolist() == [8.0, 8.0, 0.0, 6.0]


# ------------------------------------------------------------------------------------------------ 2. swap
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 4097])
def test_swap_every_alignment(a3d, dev, n):
    """Base pointers 0 .. 3 floats past an aligned allocation, independently for a and b: exact exchange, guard elements on both
    sides untouched."""
    L = a3d.lib
    G = 8                                                   # guard floats on each side
    g = torch.Generator().manual_seed(n)
    for oa in range(4):
        for ob in range(4):
            bufa = torch.randn(G + 3 + n + G, generator=g).to(dev)
            bufb = torch.randn(G + 3 + n + G, generator=g).to(dev)
            assert bufa.data_ptr() % 16 == 0 and bufb.data_ptr() % 16 == 0
            a0, b0 = bufa.clone(), bufb.clone()
            sa, sb = slice(G + oa, G + oa + n), slice(G + ob, G + ob + n)
            L.call("a3d_swap_f32", bufa.data_ptr() + 4 * sa.start, bufb.data_ptr() + 4 * sb.start, n, L.stream())
            wa, wb = a0.clone(), b0.clone()
            wa[sa], wb[sb] = b0[sb], a0[sa]
            assert torch.equal(bufa, wa) and torch.equal(bufb, wb), (n, oa, ob)


# ------------------------------------------------------------------------------------------------ 3. graph replay
def test_ema_advances_inside_the_replayed_step_graph(a3d, dev):
    """The small Act3D of test_graphed_step_equals_eager_train_one_step under GraphedStep: after every replay the average obeys
    the float64 recurrence with t one further -- the decay weight is read from the device, not frozen into the capture."""
    from test_engine_gpu import _sample
    E = a3d.engine
    torch.manual_seed(0)
    m = a3d.Act3D(image_size=(128, 128), embedding_dim=60, num_attn_heads=4, gripper_loc_bounds=C.PERACT_BOUNDS,
                  num_ghost_points=128, num_ghost_points_val=128, num_sampling_level=2, sampler_seed=5).to(dev).train()
    s = _sample(2, 2, 128, dev, 33)
    crit = a3d.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    decay, warmup = 0.999, 10
    flat, opt = E.get_optimizer(m, lr=1e-4, ema_decay=decay, ema_warmup=warmup)
    seg_id = torch.repeat_interleave(torch.arange(len(flat.order)), torch.tensor([p.numel() for _, p in flat.order])).to(dev)

    def fwd_bwd(sample):
        out = m(sample["rgbs"], sample["pcds"], sample["instr"], sample["curr_gripper"], gt_action=sample["action"])
        loss = sum(crit.compute_loss(out, sample).values())
        loss.backward()
        return loss.detach()

    graphed = E.GraphedStep(fwd_bwd, opt, s, warmup=1)
    torch.cuda.synchronize()
    t = int(opt.ema_updates.item())
    assert t == 1 and opt.step_count.item() == 1.0, "one eager warm-up step, the capture itself runs nothing"
    prev = opt.ema.double()
    ws = []
    for k in range(3):
        graphed(s)
        torch.cuda.synchronize()
        t += 1
        active = opt.seg_state[:, 1][seg_id] == 1.0
        want = R.ema_update(prev, flat.flat, t, decay, warmup, active=active)
        within_bar(f"ema after replay {k + 1} (t = {t})", opt.ema, want)
        moved = (opt.ema.double() - prev).abs().max().item()
        assert moved > 0.0
        ws.append(opt.ema_state[0].item())
        assert int(opt.ema_updates.item()) == t and opt.ema_updates.item() == opt.step_count.item()
        prev = opt.ema.double()
    assert ws[0] > ws[1] > ws[2] and abs(ws[2] - 9.0 / 14.0) < 1e-6, ws


# ------------------------------------------------------------------------------------------------ 4. sampling
def _planner(a3d, dev, P):
    m = a3d.DiffusionPlanner(embedding_dim=120, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100)
    m.load_state_dict(P, strict=False)
    return m.to(dev).eval()


def test_sampling_under_ema_weights_sees_the_swap(a3d, dev):
    """compute_trajectory inside `with opt.ema_weights():` -- eager, captured, replayed -- equals a second planner that was LOADED
    with the averages; after the block the same planner (its graph captured under the averages included) samples from the raw
    weights again."""
    from test_oracle_golden import _diffusion_params, load
    E = a3d.engine
    P = _diffusion_params(load("diffusion.pt"))
    B, Ln, K = 2, 8, 4
    inp = C.trajectory_inputs(91, B, Ln, 3, 120, pad_last=3)
    tokens = C.tokens_from_maps(inp["fmap"]).to(dev)
    d = {k: v.to(dev) for k, v in inp.items()}

    def sample(model, **kw):
        return model.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"],
                                        init_noise=d["init_noise"], step_noise=d["step_noise"][:K].contiguous(), visual_tokens=tokens,
                                        num_inference_steps=K, **kw).clone()

    m = _planner(a3d, dev, P)
    flat, opt = E.get_optimizer(m, ema_decay=0.999)
    raw = sample(m)
    assert torch.isfinite(raw).all() and torch.equal(sample(m), raw), "run-to-run determinism, which everything below relies on"
    noise = torch.randn(flat.n, generator=torch.Generator().manual_seed(5)).to(dev)
    opt.ema.copy_(flat.flat * (1.0 + 0.05 * noise))
    m2 = _planner(a3d, dev, P)
    merged = {k: v.detach().clone() for k, v in m.state_dict().items()}
    merged.update(opt.ema_state_dict())
    m2.load_state_dict(merged)
    want = sample(m2)
    assert not torch.equal(want, raw), "the perturbation must change the trajectory"
    raw_flat = flat.flat.clone()
    with opt.ema_weights():
        assert opt.ema_swapped
        got = [sample(m), sample(m, use_graph=True), sample(m, use_graph=True)]
    assert not opt.ema_swapped and torch.equal(flat.flat, raw_flat)
    for name, x in zip(("eager", "capturing call", "replay"), got):
        assert torch.equal(x, want), f"{name} under ema_weights(): max abs diff {(x - want).abs().max().item():.3e}"
    assert torch.equal(sample(m, use_graph=True), raw), "the graph captured under the averages pinned them"
    assert torch.equal(sample(m), raw)
    # an exception inside the block still swaps back
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("boom")
    assert not opt.ema_swapped and torch.equal(flat.flat, raw_flat)


# ------------------------------------------------------------------------------------------------ 5. driver
def test_keypose_driver_with_ema_end_to_end(a3d, dev, tmp_path):
    """The synthetic dataset of test_keypose_train_tester_main_end_to_end with ema_decay = 0.99, ema_warmup = 0, two steps, one
    evaluation round (under the averages) and the checkpoints written after the swap back."""
    E = a3d.engine
    root = tmp_path / "data"
    for task, seed, T in (("task_a", 31, 4), ("task_b", 32, 3)):
        d = root / f"{task}+0"
        d.mkdir(parents=True)
        for e in range(2):
            ep = C.synthetic_episode(seed + 10 * e, T, ncam=2, H=128)
            lo, hi = torch.tensor(C.PERACT_BOUNDS[0]).float(), torch.tensor(C.PERACT_BOUNDS[1]).float()
            for t in range(T):
                ep[1][t][:, 1] = lo.view(1, 3, 1, 1) + (ep[1][t][:, 1] * 0.5 + 0.5) * (hi - lo).view(1, 3, 1, 1)
                for lst in (ep[2], ep[4]):
                    lst[t][:, :3] = lo + torch.sigmoid(lst[t][:, :3]) * (hi - lo)
            with open(d / f"ep{e}.pkl", "wb") as f:
                pickle.dump(ep, f)
    rs = np.random.RandomState(3)
    with open(tmp_path / "instructions.pkl", "wb") as f:
        pickle.dump({"task_a": {0: C.rs_tensor(rs, (2, 53, 512))}, "task_b": {0: C.rs_tensor(rs, (2, 53, 512))}}, f)
    log_dir = tmp_path / "logs"
    log_dir.mkdir()
    args = types.SimpleNamespace(
        local_rank=0, cameras=C.DATASET_CAMERAS, image_size="128,128", max_episodes_per_task=100,
        instructions=str(tmp_path / "instructions.pkl"), seed=0, tasks=("task_a", "task_b"), variations=(0,), checkpoint=None,
        accumulate_grad_batches=1, val_freq=2, gripper_loc_bounds=C.PERACT_BOUNDS, eval_only=0, dataset=str(root),
        valset=str(root), log_dir=log_dir, num_workers=0, batch_size=2, batch_size_val=2, cache_size=0, cache_size_val=0,
        lr=1e-4, train_iters=2, max_episode_length=5, image_rescale="0.75,1.25", point_cloud_rotate_yaw_range=0.0,
        position_prediction_only=0, position_loss="ce", ground_truth_gaussian_spread=0.01, compute_loss_at_all_layers=0,
        position_loss_coeff=1.0, position_offset_loss_coeff=10000.0, rotation_loss_coeff=10.0, symmetric_rotation_loss=0,
        gripper_loss_coeff=1.0, label_smoothing=0.0, regress_position_offset=0, num_sampling_level=2,
        fine_sampling_ball_diameter=0.16, weight_tying=1, gp_emb_tying=1, num_ghost_points=200, num_ghost_points_val=400,
        use_ground_truth_position_for_sampling_train=1, backbone="clip", embedding_dim=60,
        num_ghost_point_cross_attn_layers=2, num_query_cross_attn_layers=2, num_vis_ins_attn_layers=2,
        rotation_parametrization="quat_from_query", use_instruction=1, ema_decay=0.99, ema_warmup=0)
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    tt = a3d.KeyposeTrainTester(args)
    seen = {}
    build = tt.get_optimizer

    def get_optimizer(model):                               # keep the optimizer main() builds, and the weights it starts from
        opt = build(model)
        seen["opt"], seen["p0"] = opt, opt.flat.flat.detach().clone()
        return opt
    tt.get_optimizer = get_optimizer
    model = tt.main(collate_fn=a3d.data.keypose_collate_fn)
    torch.cuda.synchronize()
    opt, p0 = seen["opt"], seen["p0"].cpu()
    flat = opt.flat
    assert opt.ema is not None and opt.ema_decay == 0.99 and opt.ema_warmup == 0.0
    assert opt.ema_swapped is False
    assert "val-losses/mean/pos_l2_final" in tt.scalars
    ck = torch.load(log_dir / "last.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"weight", "optimizer", "iter", "best_loss", "ema"} and ck["iter"] == 2
    assert ck["ema"]["updates"] == 2 and ck["ema"]["decay"] == 0.99 and ck["ema"]["warmup"] == 0
    assert set(ck["ema"]["weight"]) == {"module." + n for n, _ in flat.order}
    # the model holds the raw weights: what "weight" recorded, and what the flat buffer holds
    for n, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), ck["weight"]["module." + n]), n
    steps = opt.param_steps.cpu()
    trained = [n for (n, _), st in zip(flat.order, steps) if st > 0]
    assert len(trained) > 10
    lr = args.lr
    n_checked = 0
    for n in trained:
        a, b = flat.slices[n]
        w0, w2 = p0[a:b].double(), ck["weight"]["module." + n].reshape(-1).double()
        e = ck["ema"]["weight"]["module." + n].reshape(-1).double()
        assert not torch.equal(e, w2), n
        # "moved": by at least half a learning-rate step (relative for large weights).  After two AdamW steps d1, d2 the average sits
        # at p0 + 0.0199 d1 + 0.01 d2 and d2 / d1 > -0.75 (bias-corrected moments of two gradients), so it is at least 1.2 % and at
        # most 76 % of the way from p0 to p2: both margins are tens of fp32 ulps for a move this large.
        moved = (w2 - w0).abs() > 0.5 * lr * w0.abs().clamp(min=1.0)
        lo_, hi_ = torch.minimum(w0, w2), torch.maximum(w0, w2)
        ok = (e > lo_) & (e < hi_)
        assert bool(ok[moved].all()), f"{n}: {int((~ok & moved).sum())} of {int(moved.sum())} moved elements not strictly between"
        n_checked += int(moved.sum())
    print(f"[ema] {n_checked} moved elements of {len(trained)} trained tensors lie strictly between initial and final weight")
    assert n_checked > 0
    # deployment: a fresh model loaded with the averages
    m2 = tt.get_model().to(dev)
    E.load_checkpoint(str(log_dir / "last.pth"), m2, weights="ema")
    sd2 = m2.state_dict()
    for n, _ in flat.order:
        assert torch.equal(sd2[n].cpu(), ck["ema"]["weight"]["module." + n]), n
    # every other entry is "weight"'s (a tied parameter appears under several names in state_dict and under ONE in the flat buffer:
    # its other names alias the averaged tensor, so "other" goes by storage, not by name)
    averaged = {sd2[n].data_ptr() for n, _ in flat.order}
    others = [k for k in ck["weight"] if sd2[k[7:]].data_ptr() not in averaged]
    assert any(k.startswith("module.backbone") for k in others)
    for k in others:
        assert torch.equal(sd2[k[7:]].cpu(), ck["weight"][k]), k
