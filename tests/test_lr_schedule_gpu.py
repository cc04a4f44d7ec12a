"""The device-resident learning-rate schedule of the fused AdamW on the device: a3d_adamw_sched_step against the
existing entries called with the rate the device reported (bit for bit, all four {EMA} x {clip} selections), the rate against the
float64 reference of tests/lr_schedule_ref.py, the skipped step, the schedule inside a replayed graph with a changed base rate,
resume from state_dict(), and the keypose driver end to end with lr_schedule."""
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
import lr_schedule_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(37,), (40, 25), (64,), (48,)]                      # a bias, a matrix with a dead row, a never-used tensor, a late joiner
SIZES = [int(np.prod(s)) for s in SHAPES]
OFF = [0, 37, 1037, 1101, 1149]
HYPER = (0.9, 0.999, 1e-8, 0.0, 5e-4)                         # beta1, beta2, eps, wd_nodecay, wd_decay
BASE = float(np.float32(1e-2))                                # the base rate as the device holds it (lr_state[3] is an fp32)
W, N, RATIO, STEPS = 3, 10, 0.1, 14                           # warm-up, the knot, the decay and the clamp past N
MAX_NORM = 14.0                                               # the unit-amplitude gradients have norm ~ 33, the small ones ~ 3 .. 5
AMPS = [1.0, 0.1, 1.0, 0.1, 3.0, 0.05, 1.0, 0.15, 1.0, 0.1, 2.0, 0.1, 1.0, 0.12]


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


class State:
    """p, m, v, step, seg_state (+ ema, ema_state, + clip_state) of the flat buffer, steppable by the scheduled entry and by the
    entry that exists without a schedule."""

    def __init__(self, L, dev, p0, ema, clip):
        self.L, self.n, self.nseg, self.n_nodecay, self.clip = L, OFF[-1], len(OFF) - 1, SIZES[0], clip
        self.seg_off = torch.tensor(OFF, dtype=torch.int64, device=dev)
        z = lambda *s: torch.zeros(*s, device=dev)
        self.t = dict(p=p0.clone(), m=z(self.n), v=z(self.n), step=z(1), seg=z(self.nseg, 4))
        if ema:
            self.t.update(ema=p0.clone(), ema_state=z(4))
        if clip:
            self.t.update(clip_state=z(8))
        self.clip_ws = torch.zeros(L.ADAMW_CLIP_WS_DOUBLES, device=dev, dtype=torch.float64)
        self.lr_state = z(8)
        self.lr_state[3] = BASE

    def _ptr(self, k):
        return self.t[k].data_ptr() if k in self.t else None

    def clone_tensors(self):
        return {k: v.clone() for k, v in self.t.items()}

    def sched_step(self, g, kind, warmup=W, total=N, ratio=RATIO, gscale=1.0):
        L = self.L
        L.call("a3d_adamw_sched_step", self._ptr("p"), g.data_ptr(), self._ptr("m"), self._ptr("v"), self._ptr("ema"), self._ptr("step"),
               self.seg_off.data_ptr(), self._ptr("seg"), self._ptr("ema_state"), self._ptr("clip_state"),
               self.clip_ws.data_ptr() if self.clip else None, self.lr_state.data_ptr(), self.nseg, self.n, self.n_nodecay,
               L.LR_DECAY_KINDS[kind], float(warmup), float(total), ratio, *HYPER, gscale, 0.999, 10.0, MAX_NORM, L.stream())
        return self.lr_state.cpu().numpy()

    def existing_step(self, g, lr, gscale=1.0):
        """a3d_adamw_clip_step with clipping, else a3d_adamw_ema_step with an average, else a3d_adamw_step: called with lr"""
        L, ema = self.L, "ema" in self.t
        if self.clip:
            L.call("a3d_adamw_clip_step", self._ptr("p"), g.data_ptr(), self._ptr("m"), self._ptr("v"), self._ptr("ema"),
                   self._ptr("step"), self.seg_off.data_ptr(), self._ptr("seg"), self._ptr("ema_state"), self._ptr("clip_state"),
                   self.clip_ws.data_ptr(), self.nseg, self.n, self.n_nodecay, lr, *HYPER, gscale, 0.999, 10.0, MAX_NORM, L.stream())
        elif ema:
            L.call("a3d_adamw_ema_step", self._ptr("p"), g.data_ptr(), self._ptr("m"), self._ptr("v"), self._ptr("ema"),
                   self._ptr("step"), self.seg_off.data_ptr(), self._ptr("seg"), self._ptr("ema_state"), self.nseg, self.n,
                   self.n_nodecay, lr, *HYPER, gscale, 0.999, 10.0, L.stream())
        else:
            L.call("a3d_adamw_step", self._ptr("p"), g.data_ptr(), self._ptr("m"), self._ptr("v"), self._ptr("step"),
                   self.seg_off.data_ptr(), self._ptr("seg"), self.nseg, self.n, self.n_nodecay, lr, *HYPER, gscale, L.stream())


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        # NaN never occurs in these states, so torch.equal is a bit comparison up to the sign of zero
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max abs diff {(a[k] - b[k]).abs().max().item():.3e})"


def check_rate(name, got, t, kind, base=BASE, warmup=W, total=N, ratio=RATIO, exact=False):
    """lr_t within one fp32 ulp of fp32(reference): the device's and the host's double cos may differ in the last double ulp, and
    one fp32 rounding follows.  Returns the distance in ulps."""
    want = R.rate(t, base, kind, warmup, total, ratio)
    d = R.ulps(got, want)
    print(f"[lr] {name}: t={t} got {float(got)!r} want {float(want)!r} ulps {d} (bar {0 if exact else 1})")
    assert d <= (0 if exact else 1), f"{name}: t={t}: {float(got)!r} vs {float(want)!r}: {d} ulps"
    return d


# ------------------------------------------------------------------------------------------------ 1. step parity
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_sched_step_equals_existing_step_with_the_device_rate(a3d, dev, ema, clip, kind):
    """14 steps, W = 3, N = 10, r = 0.1, base rate 1e-2.  The twin is stepped by the entry that exists without a schedule, with
    lr = lr_state[0] as read back after the live step."""
    L = a3d.lib
    p0, grads = _gradients(dev)
    live, twin = State(L, dev, p0, ema, clip), State(L, dev, p0, ema, clip)
    for it, g in enumerate(grads):
        ls = live.sched_step(g, kind)
        check_rate(f"{kind} step {it + 1}", ls[0], it, kind)
        assert ls[1] == float(it + 1), "the position counts the applied steps"
        twin.existing_step(g, float(ls[0]))
        assert_same(live.t, twin.t, f"step {it + 1}")
        if it == 0:                                              # t = 0 in a warm-up: the rate is exactly 0
            assert ls[0] == 0.0 and ls[2] == 0.0
            assert torch.equal(live.t["p"], p0), "a step at rate 0 leaves p as it was"
            assert bool((live.t["m"] != 0).any()) and bool((live.t["v"] != 0).any()), "... and moves the moments"
    assert live.t["seg"][:, 0].cpu().tolist() == [14.0, 14.0, 0.0, 12.0] and live.t["step"].item() == 14.0
    assert not torch.equal(live.t["p"], p0)
    if clip:
        assert 0.0 < live.t["clip_state"][3].item() < 14.0 and live.t["clip_state"][4].item() == 0.0, "some steps clip, none skips"


# ------------------------------------------------------------------------------------------------ 2. rate accuracy
@pytest.mark.parametrize("cfg", [(3, 10, 0.1), (0, 7, 0.25), (5, 6, 1.0)], ids=lambda c: "W%d-N%d-r%g" % c)
@pytest.mark.parametrize("kind", R.KINDS)
def test_rate_follows_the_float64_reference(a3d, dev, kind, cfg):
    """lr_state after every step: [0] within one ulp of fp32(reference) -- exactly equal at t = 0 of a warm-up and wherever f is 1
    (the constant kind after its warm-up) --, [1] the position, [2] f(t) to one ulp, [3] the base rate untouched, [4..7] zero.
    Every r here is > 0: at r = 0 the cosine ends in a cancellation, 1 + cos(pi), where a last-place difference of the two cos is
    an absolute error, not a relative one, and an ulp count says nothing."""
    warmup, total, ratio = cfg
    L = a3d.lib
    p0, grads = _gradients(dev)
    st = State(L, dev, p0, ema=False, clip=False)
    worst = 0
    for it, g in enumerate(grads):
        ls = st.sched_step(g, kind, warmup, total, ratio)
        exact = (it == 0 and warmup > 0) or (kind == "constant" and it >= warmup)
        worst = max(worst, check_rate(f"{kind} W={warmup} N={total} r={ratio}", ls[0], it, kind, BASE, warmup, total, ratio, exact))
        assert R.ulps(ls[2], np.float32(R.factor(it, kind, warmup, total, ratio))) <= (0 if exact else 1), (it, ls)
        assert ls[1] == float(it + 1) and ls[3] == np.float32(BASE) and not ls[4:].any(), (it, ls)
        if kind == "constant" and it >= warmup:
            assert ls[0] == np.float32(BASE) and ls[2] == 1.0
    print(f"[lr] {kind} W={warmup} N={total} r={ratio}: worst {worst} ulps over {STEPS} steps")
    if kind != "constant":
        assert R.ulps(ls[0], np.float32(BASE * ratio)) <= 1, "past N the rate stays at r lr"


# ------------------------------------------------------------------------------------------------ 3. skip
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_skipped_step_leaves_the_schedule_alone(a3d, dev, ema):
    """Clipping on, a NaN in the gradient of step 5: nothing but clip_state changes, lr_state keeps its bits, and the next finite step
    runs at the rate the skipped one would have used."""
    L = a3d.lib
    kind = "cosine"
    p0, grads = _gradients(dev)
    live, twin = State(L, dev, p0, ema, True), State(L, dev, p0, ema, True)       # the twin never sees the bad step
    for it in range(4):
        live.sched_step(grads[it], kind)
        twin.sched_step(grads[it], kind)
    before, lr0, cs0 = live.clone_tensors(), live.lr_state.clone(), live.t["clip_state"].cpu().tolist()
    bad = grads[4].clone()
    bad[5] = float("nan")
    live.sched_step(bad, kind)
    after = live.clone_tensors()
    cs = after.pop("clip_state").cpu().tolist()
    before.pop("clip_state")
    assert_same(after, before, "skipped step")
    assert torch.equal(live.lr_state.view(torch.int32), lr0.view(torch.int32)), "lr_state is bit-equal before and after"
    assert math.isnan(cs[1]) and cs[0] == 0.0 and cs[4] == cs0[4] + 1.0 and cs[5] == 1.0, (cs0, cs)
    assert live.lr_state[1].item() == 4.0 and live.t["step"].item() == 4.0
    ls = live.sched_step(grads[4], kind)
    lt = twin.sched_step(grads[4], kind)
    check_rate("the step after the skip", ls[0], 4, kind)
    assert ls[1] == 5.0 and ls.tobytes() == lt.tobytes()
    live.t["clip_state"][4] = 0.0                               # the skip counter is the one trace
    assert_same(live.t, twin.t, "the step after the skip")


# ------------------------------------------------------------------------------------------------ 4. graph, 5. resume
class _Buffer(torch.nn.Module):
    """The four tensors of SHAPES as parameters, in FlatParams' order: the "bias" group first."""

    def __init__(self, p0):
        super().__init__()
        parts = [p0[a:b].clone().view(s) for a, b, s in zip(OFF[:-1], OFF[1:], SHAPES)]
        self.a_bias, self.w, self.unused, self.late = (torch.nn.Parameter(x) for x in parts)


def _optimizer(a3d, p0, total=N, **kw):
    flat, opt = a3d.engine.get_optimizer(_Buffer(p0), lr=1e-2, lr_schedule=dict(decay="cosine", warmup=W, total=total, min_ratio=RATIO),
                                         **kw)
    assert [n for n, _ in flat.order] == ["a_bias", "w", "unused", "late"] and flat.n == OFF[-1] and flat.n_nodecay == SIZES[0]
    assert torch.equal(flat.flat, p0)
    return flat, opt


def _tensors(flat, opt):
    t = dict(p=flat.flat, m=opt.exp_avg, v=opt.exp_avg_sq, step=opt.step_count, seg=opt.seg_state, lr_state=opt.lr_state)
    if opt.ema is not None:
        t.update(ema=opt.ema, ema_state=opt.ema_state)
    if opt.clip_state is not None:
        t.update(clip_state=opt.clip_state)
    return t


def test_schedule_advances_inside_the_replayed_graph_and_follows_a_changed_base_rate(a3d, dev):
    """One optimizer step (EMA + clipping + schedule: three launches) captured once; every replay takes its gradient from the static
    buffer flat.grad.  Cosine, W = 3, N = 14: one eager step (t = 0), ten replays (t = 1 .. 10), then optimizer.lr = 2e-2 and two
    more.  The twin is the same optimizer stepped eagerly."""
    p0, grads = _gradients(dev)
    kw = dict(ema_decay=0.999, ema_warmup=10, max_grad_norm=MAX_NORM)
    flat, opt = _optimizer(a3d, p0, total=14, **kw)
    flat2, twin = _optimizer(a3d, p0, total=14, **kw)
    for f, o in ((flat, opt), (flat2, twin)):
        f.grad.copy_(grads[0])
        o.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert opt.schedule_step.item() == 1.0, "the capture runs nothing"
    base = BASE
    for t in range(1, 13):
        if t == 11:
            opt.lr = twin.lr = 2e-2                             # between two replays: reaches the graph through lr_state[3]
            base = float(np.float32(2e-2))
        flat.grad.copy_(grads[t])
        flat2.grad.copy_(grads[t])
        graph.replay()
        twin.step()
        torch.cuda.synchronize()
        check_rate(f"replay {t}", opt.current_lr.item(), t, "cosine", base, W, 14, RATIO)
        assert R.ulps(opt.lr_factor.item(), np.float32(R.factor(t, "cosine", W, 14, RATIO))) <= 1
        assert opt.schedule_step.item() == float(t + 1) and opt.step_count.item() == float(t + 1)
        assert_same(_tensors(flat, opt), _tensors(flat2, twin), f"replay {t}")
    assert opt.lr == 2e-2 and opt.clipped_steps.item() > 0.0


def test_resume_continues_the_schedule_and_reset_state_restarts_it(a3d, dev):
    p0, grads = _gradients(dev)
    flat, opt = _optimizer(a3d, p0)
    for t in range(5):
        flat.grad.copy_(grads[t])
        opt.step()
    sd = opt.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == [1e-2, 1e-2] and set(sd) == {"state", "param_groups"}
    flat2, opt2 = _optimizer(a3d, flat.flat.detach().clone())
    opt2.load_state_dict(sd)
    assert opt2.schedule_step.item() == 5.0 and opt2.step_count.item() == 5.0 and opt2.current_lr.item() == 0.0
    for f, o in ((flat, opt), (flat2, opt2)):
        f.grad.copy_(grads[5])
        o.step()
    torch.cuda.synchronize()
    assert opt2.schedule_step.item() == 6.0
    check_rate("resumed", opt2.current_lr.item(), 5, "cosine")
    assert_same(_tensors(flat, opt), _tensors(flat2, opt2), "the step after the resume")
    assert opt.param_steps.cpu().tolist() == [6.0, 6.0, 0.0, 4.0]
    opt.reset_state()
    assert opt.lr_state.cpu().tolist() == [0.0, 0.0, 0.0, BASE, 0.0, 0.0, 0.0, 0.0]
    kept = flat.flat.clone()
    opt.step()
    assert opt.schedule_step.item() == 1.0 and opt.current_lr.item() == 0.0 and torch.equal(flat.flat, kept), "t = 0 again: rate 0"
    opt.schedule_step = 8
    opt.step()
    check_rate("after schedule_step = 8", opt.current_lr.item(), 8, "cosine")
    assert opt.schedule_step.item() == 9.0


# ------------------------------------------------------------------------------------------------ 6. driver
def test_keypose_driver_with_lr_schedule_end_to_end(a3d, dev, tmp_path):
    """The synthetic two-task dataset and configuration of test_keypose_driver_with_max_grad_norm_end_to_end with a cosine schedule
    (warm-up 2, total 6, min_ratio 0.1): two steps, then a second main() from the written checkpoint for two more.  The `lr`
    scalars, logged every val_freq = 2 steps, are the reference's rates at t = 1 and t = 3."""
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
    sched = dict(lr_schedule="cosine", lr_warmup=2, lr_total=6, lr_min_ratio=0.1)
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
        rotation_parametrization="quat_from_query", use_instruction=1, **sched)
    base = float(np.float32(1e-4))
    ref = dict(decay="cosine", warmup=2, total=6, min_ratio=0.1)

    def run(checkpoint, train_iters):
        args.checkpoint, args.train_iters = checkpoint, train_iters
        random.seed(0)
        np.random.seed(0)
        torch.manual_seed(0)
        tt = a3d.KeyposeTrainTester(args)
        seen, logged = {}, []
        build, add = tt.get_optimizer, tt.writer.add_scalar

        def get_optimizer(model):                           # keep the optimizer main() builds
            seen["opt"] = build(model)
            return seen["opt"]

        def add_scalar(key, value, step):                   # and every scalar it logs, not only the last one per key
            add(key, value, step)
            logged.append((key, tt.scalars[key][0], step))
        tt.get_optimizer, tt.writer.add_scalar = get_optimizer, add_scalar
        tt.main(collate_fn=a3d.data.keypose_collate_fn)
        torch.cuda.synchronize()
        return seen["opt"], logged

    opt, logged = run(None, 2)
    assert opt.lr_schedule == ref and opt.schedule_step.item() == 2.0 and opt.step_count.item() == 2.0
    rates = [(v, s) for k, v, s in logged if k == "lr"]
    factors = [(v, s) for k, v, s in logged if k == "train-stats/lr_factor"]
    assert [s for _, s in rates] == [1] and [s for _, s in factors] == [1], logged
    check_rate("driver, first run", np.float32(rates[0][0]), 1, base=base, kind="cosine", warmup=2, total=6, ratio=0.1)
    assert factors[0][0] == 0.5
    ck = torch.load(log_dir / "last.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"weight", "optimizer", "iter", "best_loss"} and ck["iter"] == 2
    assert set(ck["optimizer"]) == {"state", "param_groups"} and ck["optimizer"]["param_groups"][0]["lr"] == 1e-4
    # the second run: position from the checkpoint's step count, base rate from args.lr
    opt, logged = run(str(log_dir / "last.pth"), 4)
    assert opt.schedule_step.item() == 4.0 and opt.step_count.item() == 4.0 and opt.lr == 1e-4
    rates = [(v, s) for k, v, s in logged if k == "lr"]
    assert [s for _, s in rates] == [3], logged
    check_rate("driver, resumed run", np.float32(rates[0][0]), 3, base=base, kind="cosine", warmup=2, total=6, ratio=0.1)
    assert rates[0][0] == opt.current_lr.item(), "the scalar is the device state of the last step"
