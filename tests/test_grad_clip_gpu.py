"""Gradient-norm clipping and the non-finite step skip of the fused AdamW on the device: the norm of a3d_adamw_clip_step
against the float64 reference of tests/grad_clip_ref.py at every size class and alignment, the clipped step against the existing
entries called with the scale the device chose (bit for bit), the skip, the decision inside a replayed step graph, and the keypose
driver end to end with max_grad_norm."""
import math
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
import grad_clip_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
# double accumulation + at most two fp32 roundings at two ulps each (the bar test_ema_gpu.py holds the EMA weight to)
REL = 2.4e-7
HYPER = (1e-2, 0.9, 0.999, 1e-8, 0.0, 5e-4)                   # lr, beta1, beta2, eps, wd_nodecay, wd_decay


def close(name, got, want, rel=REL):
    err = abs(got - want) / abs(want) if want != 0.0 else abs(got)
    print(f"[clip] {name}: got {got!r} want {want!r} rel err {err:.3e} (bar {rel:.1e})")
    assert err <= rel, f"{name}: {got!r} vs {want!r}: relative error {err:.3e} above {rel:.1e}"


class State:
    """p, m, v, step, seg_state (+ ema, ema_state) of one flat buffer, steppable by each of the three entries."""

    def __init__(self, L, dev, p0, off, ema, n_nodecay):
        self.L, self.n, self.nseg, self.n_nodecay = L, off[-1], len(off) - 1, n_nodecay
        self.seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
        z = lambda *s: torch.zeros(*s, device=dev)
        self.t = dict(p=p0.clone(), m=z(self.n), v=z(self.n), step=z(1), seg=z(self.nseg, 4))
        if ema:
            self.t.update(ema=p0.clone(), ema_state=z(4))
        self.clip_state = z(8)
        self.clip_ws = torch.zeros(L.ADAMW_CLIP_WS_DOUBLES, device=dev, dtype=torch.float64)

    @property
    def has_ema(self):
        return "ema" in self.t

    def clone_tensors(self):
        return {k: v.clone() for k, v in self.t.items()}

    def clip_step(self, g_ptr, gscale, max_norm, decay=0.9, warmup=0.0):
        t, L = self.t, self.L
        L.call("a3d_adamw_clip_step", t["p"].data_ptr(), g_ptr, t["m"].data_ptr(), t["v"].data_ptr(),
               t["ema"].data_ptr() if self.has_ema else None, t["step"].data_ptr(), self.seg_off.data_ptr(), t["seg"].data_ptr(),
               t["ema_state"].data_ptr() if self.has_ema else None, self.clip_state.data_ptr(), self.clip_ws.data_ptr(), self.nseg,
               self.n, self.n_nodecay, *HYPER, gscale, decay, warmup, max_norm, L.stream())
        return self.clip_state.cpu().tolist()

    def plain_step(self, g_ptr, gscale, decay=0.9, warmup=0.0):
        """the entries that exist without clipping: a3d_adamw_ema_step with an average, a3d_adamw_step without"""
        t, L = self.t, self.L
        if self.has_ema:
            L.call("a3d_adamw_ema_step", t["p"].data_ptr(), g_ptr, t["m"].data_ptr(), t["v"].data_ptr(), t["ema"].data_ptr(),
                   t["step"].data_ptr(), self.seg_off.data_ptr(), t["seg"].data_ptr(), t["ema_state"].data_ptr(), self.nseg, self.n,
                   self.n_nodecay, *HYPER, gscale, decay, warmup, L.stream())
        else:
            L.call("a3d_adamw_step", t["p"].data_ptr(), g_ptr, t["m"].data_ptr(), t["v"].data_ptr(), t["step"].data_ptr(),
                   self.seg_off.data_ptr(), t["seg"].data_ptr(), self.nseg, self.n, self.n_nodecay, *HYPER, gscale, L.stream())


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        # NaN never occurs in these states, so torch.equal is a bit comparison up to the sign of zero
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max abs diff {(a[k] - b[k]).abs().max().item():.3e})"


# ------------------------------------------------------------------------------------------------ 1. norm sweep
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 4097, "sweep+5"])
def test_norm_matches_float64_at_every_size_and_alignment(a3d, dev, n):
    """One segment; the gradient pointer 0 .. 3 floats past an aligned allocation (the float4 body then starts 0 .. 3 elements in);
    "sweep+5" is one full sweep of the norm grid (grid x 256 threads x 4 elements) plus 5.  max_norm = +inf: measure only."""
    L = a3d.lib
    if n == "sweep+5":
        n = L.ADAMW_CLIP_WS_DOUBLES * 256 * 4 + 5            # the norm grid = one partial per workgroup
    gen = torch.Generator().manual_seed(n)
    for o in range(4):
        scale = (1.0, 0.5, -0.25, 3.0)[o]
        st = State(L, dev, torch.randn(n, generator=gen).to(dev), [0, n], ema=False, n_nodecay=0)
        st.clip_ws.fill_(1e300)                                # whatever an earlier, larger call left must not be read
        gbuf = (torch.randn(n + 8, generator=gen) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=gen))).to(dev)
        assert gbuf.data_ptr() % 16 == 0
        g = gbuf[o:o + n]
        want = R.grad_norm(g, scale)
        cs1 = st.clip_step(g.data_ptr(), scale, INF)
        cs2 = st.clip_step(g.data_ptr(), scale, INF)
        close(f"norm n={n} offset={o} scale={scale}", cs1[1], want)
        assert cs1[1] == cs2[1], "two calls on the same input must give the same bits"
        assert cs1[2] == 1.0 and cs1[0] == scale and cs1[3:] == [0.0] * 5, cs1
        assert st.t["step"].item() == 2.0 and torch.isfinite(st.t["p"]).all()


# ------------------------------------------------------------------------------------------------ 2. step parity
SHAPES = [(37,), (40, 25), (64,), (48,)]                      # a bias, a matrix with a dead row, a never-used tensor, a late joiner
SIZES = [int(np.prod(s)) for s in SHAPES]
OFF = [0, 37, 1037, 1101, 1149]
AMPS = [1.0, 0.1, 1.0, 0.1, 3.0, 0.05, 1.0, 0.15]             # per-step gradient amplitude: large steps clip, small ones do not


def _gradients(dev, seed=2):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.cat([torch.randn(s, generator=g).reshape(-1) for s in SHAPES]).to(dev)
    grads = []
    for it, amp in enumerate(AMPS):
        gr = [torch.randn(s, generator=g) * amp for s in SHAPES]
        gr[1][7] = 0.0
        grads.append(torch.cat([gr[0].reshape(-1), gr[1].reshape(-1), torch.zeros(SIZES[2]),
                                gr[3].reshape(-1) if it >= 2 else torch.zeros(SIZES[3])]).to(dev))
    return p0, grads


@pytest.mark.parametrize("finite", [True, False], ids=["max_norm=14s", "max_norm=inf"])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_clip_step_equals_existing_step_with_the_device_scale(a3d, dev, ema, gscale, finite):
    """8 steps.  The unit-amplitude gradients have norm ~ sqrt(1037 .. 1085) ~ 33 gscale, the small ones at most 0.15 of that:
    max_norm = 14 gscale puts every step's norm / max_norm outside [0.5, 2] (asserted on the float64 reference), so no fp32
    rounding can flip a branch."""
    L = a3d.lib
    p0, grads = _gradients(dev)
    max_norm = 14.0 * gscale if finite else INF
    ref = [R.grad_norm(g, gscale) for g in grads]
    R.assert_margin(ref, 14.0 * gscale)
    want_clip = [finite and x > max_norm for x in ref]
    assert not finite or (any(want_clip) and not all(want_clip)), "some steps must clip and some must not"
    live = State(L, dev, p0, OFF, ema, SIZES[0])              # a3d_adamw_clip_step
    twin = State(L, dev, p0, OFF, ema, SIZES[0])              # the existing entry, fed the scale the device chose
    clipped = 0
    for it, g in enumerate(grads):
        cs = live.clip_step(g.data_ptr(), gscale, max_norm, decay=0.999, warmup=10.0)
        e, norm, coef = cs[0], cs[1], cs[2]
        close(f"step {it + 1} norm", norm, ref[it])
        f32 = np.float32
        coef32 = float(min(f32(1.0), f32(max_norm) / (f32(norm) + f32(1e-6))))
        close(f"step {it + 1} coef", coef, coef32)
        if want_clip[it]:
            clipped += 1
            assert coef < 1.0
            assert e == float(f32(gscale) * f32(coef)), (it, cs)
            # REL for the device's norm against the reference's + REL for the fp32 formula on that norm
            close(f"step {it + 1} coef vs float64", coef, R.clip_coef(ref[it], max_norm), rel=2 * REL)
        else:
            assert coef == 1.0 and e == gscale, (it, cs)
        assert cs[3] == float(clipped) and cs[4] == 0.0 and cs[5] == 0.0 and cs[6:] == [0.0, 0.0], (it, cs)
        twin.plain_step(g.data_ptr(), e, decay=0.999, warmup=10.0)
        assert_same(live.t, twin.t, f"step {it + 1}")
    assert clipped == (sum(want_clip) if finite else 0)
    assert live.t["seg"][:, 0].cpu().tolist() == [8.0, 8.0, 0.0, 6.0]
    assert not torch.equal(live.t["p"], p0)


# ------------------------------------------------------------------------------------------------ 3. skip
def _poison(g, kind):
    g = g.clone()
    if kind == "overflow":                                     # every element finite, the norm beyond fp32
        g[OFF[1]:OFF[2]] = 3.0e38
    else:
        g[5] = {"nan": float("nan"), "inf": INF}[kind]
    return g


@pytest.mark.parametrize("kind", ["nan", "inf", "overflow"])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_non_finite_step_is_skipped_and_leaves_no_trace(a3d, dev, ema, kind):
    """The bad element arrives in step 3, together with the late joiner's first gradient."""
    L = a3d.lib
    p0, grads = _gradients(dev)
    max_norm = 14.0
    live = State(L, dev, p0, OFF, ema, SIZES[0])
    twin = State(L, dev, p0, OFF, ema, SIZES[0])              # never sees the bad step
    for it in range(2):
        live.clip_step(grads[it].data_ptr(), 1.0, max_norm)
        twin.clip_step(grads[it].data_ptr(), 1.0, max_norm)
    before = live.clone_tensors()
    cs0 = live.clip_state.cpu().tolist()
    bad = _poison(grads[2], kind)
    assert bool((bad[OFF[3]:] != 0).any()), "the late joiner's first gradient is in this step"
    cs = live.clip_step(bad.data_ptr(), 1.0, max_norm)
    assert_same(live.t, before, f"skipped step ({kind})")
    assert live.t["seg"][3, 0].item() == 0.0, "the late joiner must not join on a skipped step"
    assert not math.isfinite(cs[1]) and cs[0] == 0.0, cs
    assert cs[3] == cs0[3] and cs[4] == cs0[4] + 1.0 and cs[5] == 1.0 and cs[6:] == [0.0, 0.0], (cs0, cs)
    # the next finite step: as if the bad one had never happened
    cs = live.clip_step(grads[2].data_ptr(), 1.0, max_norm)
    cst = twin.clip_step(grads[2].data_ptr(), 1.0, max_norm)
    assert_same(live.t, twin.t, "the step after the skip")
    assert cs[5] == 0.0 and cs[4] == 1.0 and cs[:4] == cst[:4] and math.isfinite(cs[1]), (cs, cst)
    assert live.t["seg"][:, 0].cpu().tolist() == [3.0, 3.0, 0.0, 1.0] and live.t["step"].item() == 3.0
    if ema:
        assert live.t["ema_state"][1].item() == 3.0


# ------------------------------------------------------------------------------------------------ 4. graph replay
def test_clip_decision_is_made_inside_the_replayed_step_graph(a3d, dev):
    """The small Act3D of test_ema_advances_inside_the_replayed_step_graph under GraphedStep(warmup=1), with ema_decay.  max_norm
    is a host float, frozen into the capture like lr: it is set after one eager measuring step (max_grad_norm = +inf) to half the
    norm that step found, before GraphedStep runs its own warm-up step and captures.  Every replay then clips, by a coefficient
    that follows the replay's own gradient: the twin is stepped by a3d_adamw_ema_step from the same gradient buffer (zero_grad is
    at the graph's head, so flat.grad still holds it) with the scale read back from the device."""
    from test_engine_gpu import _sample
    E, L = a3d.engine, a3d.lib
    torch.manual_seed(0)
    m = a3d.Act3D(image_size=(128, 128), embedding_dim=60, num_attn_heads=4, gripper_loc_bounds=C.PERACT_BOUNDS,
                  num_ghost_points=128, num_ghost_points_val=128, num_sampling_level=2, sampler_seed=5).to(dev).train()
    s = _sample(2, 2, 128, dev, 33)
    crit = a3d.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    decay, warmup = 0.999, 10
    flat, opt = E.get_optimizer(m, lr=1e-4, ema_decay=decay, ema_warmup=warmup, max_grad_norm=INF)

    def fwd_bwd(sample):
        out = m(sample["rgbs"], sample["pcds"], sample["instr"], sample["curr_gripper"], gt_action=sample["action"])
        loss = sum(crit.compute_loss(out, sample).values())
        loss.backward()
        return loss.detach()

    opt.zero_grad()
    fwd_bwd(s)
    opt.step()
    torch.cuda.synchronize()
    norm0 = opt.grad_norm.item()
    close("measuring step: grad_norm", norm0, R.grad_norm(flat.grad))
    assert opt.clip_scale.item() == 1.0 and opt.clipped_steps.item() == 0.0 and norm0 > 0.0
    opt.max_grad_norm = 0.5 * norm0
    graphed = E.GraphedStep(fwd_bwd, opt, s, warmup=1)
    torch.cuda.synchronize()
    assert opt.step_count.item() == 2.0 and opt.clipped_steps.item() == 1.0, "one eager warm-up step, clipped; the capture runs nothing"
    hyper = (1e-4, 0.9, 0.999, 1e-8, 0.0, 5e-4)
    for k in range(3):
        twin = dict(p=flat.flat.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), step=opt.step_count.clone(),
                    seg=opt.seg_state.clone(), ema=opt.ema.clone(), ema_state=opt.ema_state.clone())
        clipped = opt.clipped_steps.item()
        graphed(s)
        torch.cuda.synchronize()
        assert bool((flat.grad != 0).any())
        want = R.grad_norm(flat.grad)
        close(f"replay {k + 1}: grad_norm", opt.grad_norm.item(), want)
        assert want > opt.max_grad_norm, "the replay's norm fell below max_norm: nothing to clip"
        assert opt.clipped_steps.item() == clipped + 1.0 and opt.skipped_steps.item() == 0.0 and opt.last_step_skipped.item() == 0.0
        e = opt.clip_scale.item()
        close(f"replay {k + 1}: clip_scale", e, R.clip_coef(want, opt.max_grad_norm), rel=2 * REL)   # norm's REL + the formula's
        L.call("a3d_adamw_ema_step", twin["p"].data_ptr(), flat.grad.data_ptr(), twin["m"].data_ptr(), twin["v"].data_ptr(),
               twin["ema"].data_ptr(), twin["step"].data_ptr(), opt.seg_off.data_ptr(), twin["seg"].data_ptr(),
               twin["ema_state"].data_ptr(), len(flat.order), flat.n, flat.n_nodecay, *hyper, e, decay, float(warmup), L.stream())
        live = dict(p=flat.flat, m=opt.exp_avg, v=opt.exp_avg_sq, step=opt.step_count, seg=opt.seg_state, ema=opt.ema,
                    ema_state=opt.ema_state)
        assert_same(live, twin, f"replay {k + 1}")
    assert opt.step_count.item() == 5.0 and opt.ema_updates.item() == 5.0


# ------------------------------------------------------------------------------------------------ 5. driver
def test_keypose_driver_with_max_grad_norm_end_to_end(a3d, dev, tmp_path):
    """The synthetic two-task dataset of test_keypose_driver_with_ema_end_to_end with max_grad_norm = 1.0, two steps: the three
    train-stats scalars are logged (at the val_freq boundary, with the other training scalars), nothing was skipped, and the
    checkpoint has the keys it has without clipping."""
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
        rotation_parametrization="quat_from_query", use_instruction=1, max_grad_norm=1.0)
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    tt = a3d.KeyposeTrainTester(args)
    seen = {}
    build = tt.get_optimizer

    def get_optimizer(model):                               # keep the optimizer main() builds
        seen["opt"] = build(model)
        return seen["opt"]
    tt.get_optimizer = get_optimizer
    tt.main(collate_fn=a3d.data.keypose_collate_fn)
    torch.cuda.synchronize()
    opt = seen["opt"]
    assert opt.max_grad_norm == 1.0 and opt.ema is None
    for key in ("train-stats/grad_norm", "train-stats/clip_scale", "train-stats/skipped_steps"):
        assert key in tt.scalars, sorted(tt.scalars)
        value, step = tt.scalars[key]
        assert math.isfinite(value) and step == 1, (key, value, step)
    norm, scale, skipped = (tt.scalars["train-stats/" + k][0] for k in ("grad_norm", "clip_scale", "skipped_steps"))
    print(f"[clip] driver: grad_norm {norm:.4f} clip_scale {scale:.4f} skipped {skipped}")
    assert skipped == 0.0 and opt.skipped_steps.item() == 0.0 and opt.step_count.item() == 2.0
    assert norm > 0.0 and 0.0 < scale <= 1.0
    close("driver: clip_scale from the logged norm", scale, R.clip_coef(norm, 1.0))
    assert norm == opt.grad_norm.item() and scale == opt.clip_scale.item(), "the scalars are the device state of the last step"
    ck = torch.load(log_dir / "last.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"weight", "optimizer", "iter", "best_loss"} and ck["iter"] == 2
    assert set(ck["optimizer"]) == {"state", "param_groups"}
