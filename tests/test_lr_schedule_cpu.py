"""The device-resident learning-rate schedule of the fused AdamW, the parts that need no GPU: the float64 reference
(tests/lr_schedule_ref.py) against known answers and torch's LambdaLR, the argument checks of a3d_adamw_sched_step (they run on the
host before any launch), FlatAdamW's bookkeeping on CPU tensors (nothing is launched), the checkpoint format and the drivers'
arguments."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lr_schedule_ref as R  # noqa: E402

INF, NAN = float("inf"), float("nan")
W, N = 4, 12                                                   # the midpoint of the decay, t = 8, is a step


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("r", [0.0, 0.1])
def test_reference_known_answers(r):
    for kind in R.KINDS:
        f = lambda t: float(R.factor(t, kind, W, N, r))
        assert f(0) == 0.0 and f(W - 1) == 0.75 and f(W) == 1.0, kind
        if kind == "constant":
            assert f(8) == f(N) == f(N + 5) == 1.0
            continue
        mid = 1.0 - (1.0 - r) / 2.0 if kind == "linear" else r + (1.0 - r) / 2.0
        assert math.isclose(f(8), mid, rel_tol=1e-15), (kind, f(8), mid)
        # the decay ends at r and stays there (u is clamped); the linear form 1 - (1 - r) is r up to one rounding
        assert f(N) == (1.0 - (1.0 - r) if kind == "linear" else r) and math.isclose(f(N), r, rel_tol=0.0, abs_tol=1e-16)
        assert f(N + 5) == f(N)
    assert float(R.factor(0, "cosine", 0, N, r)) == 1.0, "without a warm-up the first step runs at the base rate"
    # lr_t = fp32(lr f): one rounding of the double product
    assert R.rate(8, 1e-2, "linear", W, N, r) == np.float32(1e-2 * (1.0 - (1.0 - r) / 2.0))
    assert R.rate(0, 1e-2, "linear", W, N, r) == 0.0 and R.rate(N + 5, 1e-2, "cosine", W, N, r) == np.float32(1e-2 * r)
    assert R.rate(3, 1e-2, "constant", W).dtype == np.float32


def test_reference_shape():
    for kind in R.KINDS:
        f = [float(R.factor(t, kind, 7, 30, 0.1)) for t in range(40)]
        assert all(b > a for a, b in zip(f[:7], f[1:8])), "monotone warm-up"
        assert all(b <= a for a, b in zip(f[7:], f[8:])), "no rise after the warm-up, past N included"
        assert f[30:] == [f[30]] * 10 and all(0.0 <= x <= 1.0 for x in f)
    with pytest.raises(ValueError):
        R.factor(5, "linear", 3, None)
    with pytest.raises(ValueError):
        R.factor(5, "cosine", 3, 3)
    with pytest.raises(ValueError):
        R.factor(5, "exponential", 3, 10)
    assert R.ulps(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1 and R.ulps(0.0, -0.0) == 0
    assert R.ulps(np.float32(1e-2), np.float32(1e-2)) == 0 and R.ulps(1.0, -1.0) == INF


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_is_lambda_lr(kind):
    """LambdaLR computes base_lr * f in Python floats: exact equality with the reference's double product, 14 steps with W = 3,
    N = 10 (warm-up, knot, decay, clamp).  With r = 0 and t <= N the factor is the published lambda of that name."""
    Wl, Nl, base = 3, 10, 1e-2
    published = {"constant": lambda t: 1.0,
                 "linear": lambda t: max(0.0, (Nl - t) / max(1, Nl - Wl)),
                 "cosine": lambda t: max(0.0, 0.5 * (1.0 + math.cos(math.pi * 2.0 * 0.5 * (t - Wl) / max(1, Nl - Wl))))}[kind]
    for r in (0.0, 0.1):
        opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=base)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda t: R.factor(t, kind, Wl, Nl, r))
        for t in range(14):
            lr = opt.param_groups[0]["lr"]
            assert float(lr) == float(np.float64(base) * R.factor(t, kind, Wl, Nl, r)), (kind, r, t)
            assert np.float32(lr) == R.rate(t, base, kind, Wl, Nl, r)
            if r == 0.0 and t <= Nl:
                want = t / max(1.0, Wl) if t < Wl else published(t)
                assert math.isclose(float(R.factor(t, kind, Wl, Nl, r)), want, rel_tol=0.0, abs_tol=1e-15), (kind, t)
            opt.step()
            sched.step()


# ------------------------------------------------------------------------------------------------ C-ABI
def test_symbol_exported_with_signature(a3d):
    lib = a3d.lib.load()
    assert "a3d_adamw_sched_step" in a3d.lib.SIGNATURES and hasattr(lib, "a3d_adamw_sched_step")
    res, args = a3d.lib.SIGNATURES["a3d_adamw_sched_step"]
    header = open(os.path.join(os.path.dirname(HERE), "include", "act3d_hip.h")).read()
    decl = header[header.index("int a3d_adamw_sched_step("):]
    decl = decl[:decl.index(";")]
    assert res is ctypes.c_int and len(args) == decl.count(",") + 1 == 29
    assert " lr," not in decl and "float lr" not in decl, "the entry takes no lr argument"
    for kind, value in a3d.lib.LR_DECAY_KINDS.items():
        assert "#define A3D_LR_%s %d" % (kind.upper(), value) in header
    assert sorted(a3d.lib.LR_DECAY_KINDS) == sorted(R.KINDS)


def _sched_step_args(**over):
    """A valid argument list over host memory that is never dereferenced: every case below must be rejected before a launch."""
    buf = (ctypes.c_double * 512)()
    p = ctypes.addressof(buf)
    a = dict(p=p, g=p, m=p, v=p, ema=p, step=p, seg_off=p, seg_state=p, ema_state=p, clip_state=p, clip_ws=p, lr_state=p, nseg=1,
             n=16, n_nodecay=0, decay_kind=2, warmup=3.0, total=10.0, min_ratio=0.1, beta1=0.9, beta2=0.999, eps=1e-8, wd0=0.0,
             wd1=5e-4, gscale=1.0, ema_decay=0.999, ema_warmup=10.0, max_norm=1.0, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over", [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(step=None), dict(seg_off=None),
                                  dict(seg_state=None), dict(lr_state=None),
                                  dict(ema=None), dict(ema_state=None), dict(clip_state=None), dict(clip_ws=None),   # half a pair
                                  dict(nseg=0), dict(nseg=-3),
                                  dict(decay_kind=3), dict(decay_kind=-1),
                                  dict(warmup=-1.0), dict(warmup=2.5), dict(warmup=NAN), dict(warmup=INF), dict(warmup=2.0 ** 24),
                                  dict(total=3.0), dict(total=2.0), dict(total=10.5), dict(total=NAN), dict(total=INF),
                                  dict(total=2.0 ** 24), dict(decay_kind=1, total=3.0),
                                  dict(min_ratio=-0.1), dict(min_ratio=1.5), dict(min_ratio=NAN), dict(min_ratio=INF),
                                  dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=NAN),
                                  dict(ema_decay=1.0), dict(ema_decay=NAN), dict(ema_warmup=0.5), dict(ema_warmup=INF)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_adamw_sched_step_rejects_bad_arguments(a3d, over):
    lib = a3d.lib.load()
    keep, args = _sched_step_args(**over)
    assert lib.a3d_adamw_sched_step(*args) == -22
    assert "a3d_adamw_sched_step" in a3d.lib.last_error()
    del keep


def test_adamw_sched_step_empty_buffer_is_a_no_op(a3d):
    """n == 0 returns 0 after the checks and before any launch, for each of the four {EMA} x {clip} selections (the hyper-parameters
    of an absent part are not looked at, nor is total_steps of the constant kind)."""
    lib = a3d.lib.load()
    for over in (dict(n=0), dict(n=0, ema=None, ema_state=None, ema_decay=7.0, ema_warmup=-1.0),
                 dict(n=0, clip_state=None, clip_ws=None, max_norm=-1.0),
                 dict(n=0, ema=None, ema_state=None, clip_state=None, clip_ws=None, max_norm=0.0, ema_decay=NAN),
                 dict(n=0, decay_kind=0, total=0.0), dict(n=0, decay_kind=0, warmup=0.0, total=NAN),
                 dict(n=0, min_ratio=0.0), dict(n=0, min_ratio=1.0), dict(n=0, warmup=0.0, total=1.0), dict(n=0, max_norm=INF)):
        keep, args = _sched_step_args(**over)
        assert lib.a3d_adamw_sched_step(*args) == 0, (over, a3d.lib.last_error())
        del keep
    for over in (dict(n=0, min_ratio=2.0), dict(n=0, total=3.0), dict(n=0, decay_kind=7)):
        keep, args = _sched_step_args(**over)
        assert lib.a3d_adamw_sched_step(*args) == -22, "the checks come before the n == 0 return"
        del keep


# ------------------------------------------------------------------------------------------------ optimizer
def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 3))


@pytest.mark.parametrize("bad", ["exponential", "", 3, ("cosine", 10), "linear", "cosine", dict(decay="cosine"),
                                 dict(decay="step", total=10), dict(decay="linear", total=10, gamma=0.5),
                                 dict(decay="linear", warmup=10, total=10), dict(decay="cosine", warmup=3, total=2),
                                 dict(warmup=-1), dict(warmup=2.5), dict(warmup=NAN), dict(warmup=INF), dict(warmup=2 ** 24),
                                 dict(warmup="3"), dict(warmup=True),
                                 dict(decay="linear", total=10.5), dict(decay="cosine", total=2 ** 24), dict(decay="cosine", total=NAN),
                                 dict(min_ratio=-0.1), dict(min_ratio=1.5), dict(min_ratio=NAN), dict(min_ratio="0.1")],
                         ids=repr)
def test_bad_keywords_raise(a3d, bad):
    E = a3d.engine
    m = _model()
    before = [p.data_ptr() for p in m.parameters()]
    with pytest.raises(ValueError, match="lr_schedule"):
        E.get_optimizer(m, lr_schedule=bad)
    assert [p.data_ptr() for p in m.parameters()] == before, "the value is checked before the parameters are re-homed"
    flat = E.FlatParams(_model())
    with pytest.raises(ValueError, match="lr_schedule"):
        E.FlatAdamW(flat, lr_schedule=bad)


def test_accepted_keywords(a3d):
    E = a3d.engine
    assert E.get_optimizer(_model(), lr_schedule="constant")[1].lr_schedule == dict(decay="constant", warmup=0, total=None, min_ratio=0.0)
    assert E.get_optimizer(_model(), lr_schedule=dict(warmup=5.0))[1].lr_schedule == dict(decay="constant", warmup=5, total=None,
                                                                                          min_ratio=0.0)
    sc = E.get_optimizer(_model(), lr_schedule=dict(decay="cosine", warmup=3, total=10, min_ratio=1))[1].lr_schedule
    assert sc == dict(decay="cosine", warmup=3, total=10, min_ratio=1.0) and isinstance(sc["min_ratio"], float)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args):
        self.calls.append((name, args))


def test_schedule_off_is_todays_optimizer(a3d, monkeypatch):
    """Without the keyword step() makes the calls it made before the schedule existed: the same entries, the same argument lists,
    the rate by value.  (This test needs nothing of the feature: it passes without it.)"""
    E = a3d.engine
    rec = _Recorder()
    monkeypatch.setattr(E.L, "call", rec)
    monkeypatch.setattr(E.L, "stream", lambda: None)
    for kw in (dict(), dict(ema_decay=0.9), dict(max_grad_norm=1.0), dict(max_grad_norm=1.0, ema_decay=0.9)):
        flat, opt = E.get_optimizer(_model(), **kw)
        assert getattr(opt, "lr_state", None) is None, "no state is allocated"
        opt.step(grad_scale=0.5)
        opt.lr = 3e-4                                           # no device state to write
        assert opt.lr == 3e-4
        opt.step()
        opt.reset_state()
    names = ["a3d_adamw_step", "a3d_adamw_ema_step", "a3d_adamw_clip_step", "a3d_adamw_clip_step"]
    assert [c[0] for c in rec.calls] == [n for n in names for _ in range(2)]
    assert [len(c[1]) for c in rec.calls] == [18, 18, 22, 22, 25, 25, 25, 25], "the argument lists of before"
    lr_at = {18: 10, 22: 12, 25: 14}
    assert [c[1][lr_at[len(c[1])]] for c in rec.calls] == [1e-4, 3e-4] * 4, "the rate travels by value"


def test_schedule_off_explicitly_and_the_views_raise(a3d, monkeypatch):
    E = a3d.engine
    rec = _Recorder()
    monkeypatch.setattr(E.L, "call", rec)
    monkeypatch.setattr(E.L, "stream", lambda: None)
    for kw in (dict(), dict(lr_schedule=None), dict(max_grad_norm=1.0, ema_decay=0.9, lr_schedule=None)):
        flat, opt = E.get_optimizer(_model(), **kw)
        assert opt.lr_schedule is None and opt.lr_state is None
        opt.step()
        for name in ("current_lr", "lr_factor", "schedule_step"):
            with pytest.raises(RuntimeError, match="lr_schedule"):
                getattr(opt, name)
        with pytest.raises(RuntimeError, match="lr_schedule"):
            opt.schedule_step = 3
    assert [c[0] for c in rec.calls] == ["a3d_adamw_step", "a3d_adamw_step", "a3d_adamw_clip_step"]


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_schedule_on_calls_the_new_entry_with_the_right_null_pairs(a3d, monkeypatch, ema, clip):
    E = a3d.engine
    rec = _Recorder()
    monkeypatch.setattr(E.L, "call", rec)
    monkeypatch.setattr(E.L, "stream", lambda: None)
    kw = dict(ema_decay=0.9, ema_warmup=0) if ema else {}
    if clip:
        kw["max_grad_norm"] = 2.5
    flat, opt = E.get_optimizer(_model(), lr=1e-2, lr_schedule=dict(decay="cosine", warmup=3, total=10, min_ratio=0.1), **kw)
    assert opt.lr_state.shape == (8,) and opt.lr_state.dtype == torch.float32
    assert opt.lr_state.tolist() == [0.0, 0.0, 0.0, float(np.float32(1e-2)), 0.0, 0.0, 0.0, 0.0]
    opt.step(grad_scale=0.25)
    assert [c[0] for c in rec.calls] == ["a3d_adamw_sched_step"]
    a = rec.calls[0][1]
    assert len(a) == len(a3d.lib.SIGNATURES["a3d_adamw_sched_step"][1]) == 29
    assert a[0] == flat.flat.data_ptr() and a[1] == flat.grad.data_ptr() and a[5] == opt.step_count.data_ptr()
    assert (a[4], a[8]) == ((opt.ema.data_ptr(), opt.ema_state.data_ptr()) if ema else (None, None))
    assert (a[9], a[10]) == ((opt.clip_state.data_ptr(), opt.clip_ws.data_ptr()) if clip else (None, None))
    assert a[11] == opt.lr_state.data_ptr() and a[12] == len(flat.order) and a[13] == flat.n and a[14] == flat.n_nodecay
    assert a[15:19] == (a3d.lib.LR_DECAY_KINDS["cosine"], 3.0, 10.0, 0.1)
    assert a[19:24] == (0.9, 0.999, 1e-8, 0.0, 5e-4) and a[24] == 0.25
    assert a[25:28] == ((0.9, 0.0) if ema else (0.0, 0.0)) + ((2.5,) if clip else (0.0,))
    assert 1e-2 not in a, "no rate among the arguments"
    # the accessors are views of the device state: no copy, no synchronisation
    for k, name in ((0, "current_lr"), (1, "schedule_step"), (2, "lr_factor")):
        assert getattr(opt, name).data_ptr() == opt.lr_state.data_ptr() + 4 * k, name
    # optimizer.lr = x reaches the device state; the position can be set; reset_state() restarts the schedule and keeps the base rate
    opt.lr = 2e-2
    assert opt.lr == 2e-2 and opt.lr_state[3].item() == float(np.float32(2e-2))
    assert [g["lr"] for g in opt.param_groups] == [2e-2, 2e-2]
    opt.lr_state[0], opt.lr_state[2] = 1.0, 0.5
    opt.schedule_step = 7
    assert opt.schedule_step.item() == 7.0 and opt.lr_state[1].item() == 7.0
    opt.reset_state()
    assert opt.lr_state.tolist() == [0.0, 0.0, 0.0, float(np.float32(2e-2)), 0.0, 0.0, 0.0, 0.0]
    if ema:                                                     # the swapped-EMA guard still applies
        opt.ema_swapped = True
        with pytest.raises(RuntimeError, match="swapped"):
            opt.step()
        assert len(rec.calls) == 1


def test_constant_schedule_passes_no_total(a3d, monkeypatch):
    E = a3d.engine
    rec = _Recorder()
    monkeypatch.setattr(E.L, "call", rec)
    monkeypatch.setattr(E.L, "stream", lambda: None)
    flat, opt = E.get_optimizer(_model(), lr_schedule=dict(warmup=5))
    opt.step()
    assert rec.calls[0][1][15:19] == (a3d.lib.LR_DECAY_KINDS["constant"], 5.0, 0.0, 0.0)


def test_checkpoint_keys_are_unchanged_and_the_position_is_the_step_count(a3d, tmp_path):
    E = a3d.engine
    sched = dict(decay="linear", warmup=2, total=20)
    sds = []
    for kw in (dict(), dict(lr_schedule=sched), dict(lr_schedule=sched, max_grad_norm=1.0)):
        m = _model(1)
        flat, opt = E.get_optimizer(m, lr=1e-3, **kw)
        opt.seg_state[:, 0] = torch.tensor([5.0, 5.0, 0.0, 3.0])  # per-parameter step counts worth persisting
        opt.step_count.fill_(5.0)
        if opt.lr_state is not None:
            opt.lr_state[:3] = torch.tensor([7e-4, 5.0, 0.7])
        path = str(tmp_path / ("ck%d.pth" % len(sds)))
        E.save_checkpoint(path, m, opt, 4, best_loss=0.25)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert set(ck) == {"weight", "optimizer", "iter", "best_loss"}, kw
        assert set(ck["optimizer"]) == {"state", "param_groups"}
        assert [g["lr"] for g in ck["optimizer"]["param_groups"]] == [1e-3, 1e-3], "the base rate, not the scheduled one"
        sds.append(ck["optimizer"])
        # a scheduled optimizer resumes from any of them: the position is the loaded step count, the base rate the loaded one
        m2 = _model(2)
        flat2, opt2 = E.get_optimizer(m2, lr=5e-5, lr_schedule=sched)
        opt2.lr_state[:3] = 9.0
        assert E.load_checkpoint(path, m2, opt2) == (5, 0.25)
        assert opt2.step_count.item() == 5.0 and opt2.schedule_step.item() == 5.0
        assert opt2.lr_state.tolist() == [0.0, 5.0, 0.0, float(np.float32(1e-3)), 0.0, 0.0, 0.0, 0.0] and opt2.lr == 1e-3
        # and an optimizer without a schedule loads what a scheduled one wrote
        flat3, opt3 = E.get_optimizer(_model(3), lr=5e-5)
        assert E.load_checkpoint(path, _model(3), None) == (5, 0.25)
        opt3.load_state_dict(ck["optimizer"])
        assert opt3.step_count.item() == 5.0 and opt3.lr_state is None
    assert sds[0]["param_groups"] == sds[1]["param_groups"] == sds[2]["param_groups"]
    assert sorted(sds[0]["state"]) == sorted(sds[1]["state"]) == sorted(sds[2]["state"])
    for a, b in zip(sds[0]["state"].values(), sds[1]["state"].values()):
        assert sorted(a) == sorted(b) == ["exp_avg", "exp_avg_sq", "step"]
    # an empty state restarts the schedule
    flat4, opt4 = E.get_optimizer(_model(4), lr_schedule=sched)
    opt4.schedule_step = 9
    opt4.load_state_dict(E.get_optimizer(_model(4))[1].state_dict())
    assert opt4.schedule_step.item() == 0.0


def test_drivers_read_the_schedule_arguments(a3d):
    """absent, None and "" mean off; lr_total defaults to ceil(train_iters / accumulate_grad_batches)"""
    get = a3d.trainers.BaseTrainTester.get_optimizer
    ns = types.SimpleNamespace
    for args in (ns(lr=1e-4), ns(lr=1e-4, lr_schedule=None), ns(lr=1e-4, lr_schedule=""),
                 ns(lr=1e-4, lr_schedule=None, lr_warmup=5, lr_min_ratio=0.1, lr_total=100)):
        opt = get(ns(args=args), _model())
        assert opt.lr_schedule is None and opt.lr_state is None
    opt = get(ns(args=ns(lr=1e-4, lr_schedule="cosine", lr_warmup=5, lr_min_ratio=0.1, train_iters=101, accumulate_grad_batches=4,
                         max_grad_norm=0.5, ema_decay=0.9)), _model())
    assert opt.lr_schedule == dict(decay="cosine", warmup=5, total=26, min_ratio=0.1)
    assert opt.clip_state is not None and opt.ema is not None and opt.lr_state[3].item() == float(np.float32(1e-4))
    opt = get(ns(args=ns(lr=1e-4, lr_schedule="linear", lr_total=40, train_iters=100)), _model())
    assert opt.lr_schedule == dict(decay="linear", warmup=0, total=40, min_ratio=0.0)
    opt = get(ns(args=ns(lr=1e-4, lr_schedule="constant", lr_warmup=8)), _model())
    assert opt.lr_schedule == dict(decay="constant", warmup=8, total=None, min_ratio=0.0)
    with pytest.raises(ValueError, match="lr_schedule"):
        get(ns(args=ns(lr=1e-4, lr_schedule="cosine", lr_warmup=50, train_iters=40)), _model())


def test_drivers_log_the_scheduled_rate(a3d, tmp_path):
    """With a schedule the `lr` scalar is optimizer.current_lr and train-stats/lr_factor is logged, at the val_freq boundary only;
    without one the line is the constant args.lr."""
    T = a3d.trainers
    ns = types.SimpleNamespace
    tt = T.BaseTrainTester(ns(lr=1e-4, val_freq=2, log_dir=str(tmp_path)))
    opt = T.BaseTrainTester.get_optimizer(ns(args=ns(lr=1e-4, lr_schedule="linear", lr_total=10)), _model())
    opt.lr_state[0], opt.lr_state[2] = 7e-5, 0.7
    tt._log_train(torch.tensor(1.0), 0, opt)
    assert "lr" not in tt.scalars
    tt._log_train(torch.tensor(1.0), 1, opt)
    assert tt.scalars["lr"] == (float(np.float32(7e-5)), 1) and tt.scalars["train-stats/lr_factor"] == (float(np.float32(0.7)), 1)
    tt2 = T.BaseTrainTester(ns(lr=1e-4, val_freq=2, log_dir=str(tmp_path)))
    tt2._log_train(torch.tensor(1.0), 1, T.BaseTrainTester.get_optimizer(ns(args=ns(lr=1e-4)), _model()))
    assert tt2.scalars["lr"] == (1e-4, 1) and "train-stats/lr_factor" not in tt2.scalars
