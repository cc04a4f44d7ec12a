"""Gradient-norm clipping of the fused AdamW, the parts that need no GPU: the argument checks of a3d_adamw_clip_step (they run on
the host before any launch), FlatAdamW's bookkeeping on CPU tensors (nothing is launched), the checkpoint format, and the float64
reference (tests/grad_clip_ref.py) against torch.nn.utils.clip_grad_norm_."""
import ctypes
import math
import os
import re
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import grad_clip_ref as R  # noqa: E402

INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------ C-ABI
def test_symbol_exported_with_signature_and_workspace_constant(a3d):
    lib = a3d.lib.load()
    assert "a3d_adamw_clip_step" in a3d.lib.SIGNATURES and hasattr(lib, "a3d_adamw_clip_step")
    res, args = a3d.lib.SIGNATURES["a3d_adamw_clip_step"]
    assert res is ctypes.c_int and len(args) == 25
    header = open(os.path.join(os.path.dirname(HERE), "include", "act3d_hip.h")).read()
    assert "int a3d_adamw_clip_step(" in header
    m = re.search(r"#define\s+A3D_ADAMW_CLIP_WS_DOUBLES\s+(\d+)", header)
    assert m and int(m.group(1)) == a3d.lib.ADAMW_CLIP_WS_DOUBLES


def _clip_step_args(**over):
    """A valid argument list over host memory that is never dereferenced: every case below must be rejected before a launch."""
    buf = (ctypes.c_double * 512)()
    p = ctypes.addressof(buf)
    a = dict(p=p, g=p, m=p, v=p, ema=p, step=p, seg_off=p, seg_state=p, ema_state=p, clip_state=p, clip_ws=p, nseg=1, n=16,
             n_nodecay=0, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd0=0.0, wd1=5e-4, gscale=1.0, ema_decay=0.999, ema_warmup=10.0,
             max_norm=1.0, stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over", [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(step=None), dict(seg_off=None),
                                  dict(seg_state=None), dict(clip_state=None), dict(clip_ws=None),
                                  dict(ema=None), dict(ema_state=None),                    # exactly one of the two
                                  dict(nseg=0), dict(nseg=-3),
                                  dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=NAN), dict(max_norm=-INF),
                                  dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=NAN), dict(ema_decay=INF),
                                  dict(ema_warmup=0.5), dict(ema_warmup=-1.0), dict(ema_warmup=NAN), dict(ema_warmup=INF)],
                         ids=lambda o: "%s=%s" % next(iter(o.items())))
def test_adamw_clip_step_rejects_bad_arguments(a3d, over):
    lib = a3d.lib.load()
    keep, args = _clip_step_args(**over)
    assert lib.a3d_adamw_clip_step(*args) == -22
    assert "a3d_adamw_clip_step" in a3d.lib.last_error()
    del keep


def test_adamw_clip_step_empty_buffer_is_a_no_op(a3d):
    """n == 0 returns 0 after the checks and before any launch -- with an average, and without one (whose ema_decay / ema_warmup
    are then not looked at); max_norm = +inf is a legal value."""
    lib = a3d.lib.load()
    for over in (dict(n=0), dict(n=0, ema=None, ema_state=None, ema_decay=7.0, ema_warmup=-1.0), dict(n=0, max_norm=INF)):
        keep, args = _clip_step_args(**over)
        assert lib.a3d_adamw_clip_step(*args) == 0, over
        del keep
    keep, args = _clip_step_args(n=0, max_norm=0.0)
    assert lib.a3d_adamw_clip_step(*args) == -22, "the checks come before the n == 0 return"
    del keep


# ------------------------------------------------------------------------------------------------ optimizer
def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 3))


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, NAN, -INF, 1e-60])
def test_bad_keywords_raise(a3d, bad):
    E = a3d.engine
    m = _model()
    before = [p.data_ptr() for p in m.parameters()]
    with pytest.raises(ValueError):
        E.get_optimizer(m, max_grad_norm=bad)
    assert [p.data_ptr() for p in m.parameters()] == before, "the value is checked before the parameters are re-homed"
    flat = E.FlatParams(_model())
    with pytest.raises(ValueError):
        E.FlatAdamW(flat, max_grad_norm=bad)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args):
        self.calls.append((name, args))


def test_clipping_off_is_todays_optimizer(a3d, monkeypatch):
    E = a3d.engine
    rec = _Recorder()
    monkeypatch.setattr(E.L, "call", rec)
    monkeypatch.setattr(E.L, "stream", lambda: None)
    flat, opt = E.get_optimizer(_model())
    assert opt.max_grad_norm is None and opt.clip_state is None and opt.clip_ws is None
    opt.step(grad_scale=0.5)
    flat2, opt2 = E.get_optimizer(_model(), ema_decay=0.9)
    opt2.step()
    assert [c[0] for c in rec.calls] == ["a3d_adamw_step", "a3d_adamw_ema_step"], "clipping off: the entries of today"
    assert len(rec.calls[0][1]) == 18 and len(rec.calls[1][1]) == 22
    for name in ("grad_norm", "clip_scale", "clipped_steps", "skipped_steps", "last_step_skipped"):
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            getattr(opt, name)
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            getattr(opt2, name)


def test_clipping_on_calls_the_new_entry_with_and_without_ema(a3d, monkeypatch):
    E = a3d.engine
    rec = _Recorder()
    monkeypatch.setattr(E.L, "call", rec)
    monkeypatch.setattr(E.L, "stream", lambda: None)
    flat, opt = E.get_optimizer(_model(), max_grad_norm=2.5)
    assert opt.max_grad_norm == 2.5 and opt.ema is None
    assert opt.clip_state.shape == (8,) and opt.clip_state.dtype == torch.float32 and float(opt.clip_state.abs().sum()) == 0.0
    assert opt.clip_ws.shape == (a3d.lib.ADAMW_CLIP_WS_DOUBLES,) and opt.clip_ws.dtype == torch.float64
    opt.step(grad_scale=0.25)
    flat2, opt2 = E.get_optimizer(_model(), ema_decay=0.9, ema_warmup=0, max_grad_norm=INF)
    opt2.step()
    assert [c[0] for c in rec.calls] == ["a3d_adamw_clip_step", "a3d_adamw_clip_step"]
    a = rec.calls[0][1]
    assert len(a) == 25
    assert a[0] == flat.flat.data_ptr() and a[1] == flat.grad.data_ptr() and a[4] is None and a[8] is None, "no EMA: both null"
    assert a[9] == opt.clip_state.data_ptr() and a[10] == opt.clip_ws.data_ptr()
    assert a[11] == len(flat.order) and a[12] == flat.n and a[20] == 0.25 and a[23] == 2.5
    b = rec.calls[1][1]
    assert b[4] == opt2.ema.data_ptr() and b[8] == opt2.ema_state.data_ptr() and b[21] == 0.9 and b[22] == 0.0 and b[23] == INF
    # the accessors are views of the device state: no copy, no synchronisation
    for k, name in ((1, "grad_norm"), (0, "clip_scale"), (3, "clipped_steps"), (4, "skipped_steps"), (5, "last_step_skipped")):
        assert getattr(opt, name).data_ptr() == opt.clip_state.data_ptr() + 4 * k, name
    # the swapped-EMA guard still applies
    opt2.ema_swapped = True
    with pytest.raises(RuntimeError, match="swapped"):
        opt2.step()
    assert len(rec.calls) == 2


def test_reset_state_zeroes_the_clip_state(a3d):
    E = a3d.engine
    flat, opt = E.get_optimizer(_model(), max_grad_norm=1.0, ema_decay=0.9)
    opt.clip_state.copy_(torch.arange(1.0, 9.0))
    assert float(opt.skipped_steps) == 5.0 and float(opt.grad_norm) == 2.0
    opt.reset_state()
    assert float(opt.clip_state.abs().sum()) == 0.0
    assert float(opt.ema_updates) == 0.0


def test_checkpoint_keys_are_unchanged_by_clipping(a3d, tmp_path):
    E = a3d.engine
    sds = []
    for kw, keys in ((dict(), {"weight", "optimizer", "iter", "best_loss"}),
                     (dict(max_grad_norm=1.0), {"weight", "optimizer", "iter", "best_loss"}),
                     (dict(max_grad_norm=1.0, ema_decay=0.99), {"weight", "optimizer", "iter", "best_loss", "ema"})):
        m = _model(1)
        flat, opt = E.get_optimizer(m, **kw)
        if opt.clip_state is not None:
            opt.clip_state.copy_(torch.arange(1.0, 9.0))                 # a state worth persisting, if anything persisted it
        path = str(tmp_path / ("ck%d.pth" % len(sds)))
        E.save_checkpoint(path, m, opt, 3, best_loss=0.25)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert set(ck) == keys, kw
        if "ema" in ck:
            assert set(ck["ema"]) == {"weight", "decay", "warmup", "updates"}
        assert set(ck["optimizer"]) == {"state", "param_groups"}
        sds.append(ck["optimizer"])
        # a clipping optimizer resumes from it; its clip state starts from zero (load_state_dict resets the optimizer state)
        m2 = _model(2)
        flat2, opt2 = E.get_optimizer(m2, max_grad_norm=3.0)
        opt2.clip_state.fill_(1.0)
        assert E.load_checkpoint(path, m2, opt2) == (4, 0.25)
        assert torch.equal(flat2.flat, flat.flat) and float(opt2.clip_state.abs().sum()) == 0.0
    assert sds[0]["param_groups"] == sds[1]["param_groups"] == sds[2]["param_groups"] and sds[1]["state"] == {}


def test_drivers_read_args_max_grad_norm(a3d):
    """absent, None and 0 mean off; a value reaches the optimizer"""
    get = a3d.trainers.BaseTrainTester.get_optimizer
    for ns in (types.SimpleNamespace(lr=1e-4), types.SimpleNamespace(lr=1e-4, max_grad_norm=None),
               types.SimpleNamespace(lr=1e-4, max_grad_norm=0), types.SimpleNamespace(lr=1e-4, max_grad_norm=0.0)):
        opt = get(types.SimpleNamespace(args=ns), _model())
        assert opt.max_grad_norm is None and opt.clip_state is None
    opt = get(types.SimpleNamespace(args=types.SimpleNamespace(lr=1e-4, max_grad_norm=0.5, ema_decay=0.9)), _model())
    assert opt.max_grad_norm == 0.5 and opt.clip_state is not None and opt.ema is not None


# ------------------------------------------------------------------------------------------------ reference
def test_reference_is_torch_clip_grad_norm():
    g = torch.randn(1000, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    n = R.grad_norm(g)
    assert math.isclose(n, float(g.norm()), rel_tol=1e-14)
    assert math.isclose(R.grad_norm(g, -0.5), 0.5 * n, rel_tol=1e-15)
    for max_norm in (0.25 * n, 4.0 * n, INF):
        clipped, total = R.torch_clip(g, max_norm)
        assert math.isclose(total, n, rel_tol=1e-14)
        c = R.clip_coef(n, max_norm)
        assert (c == 1.0) == (max_norm > n)
        assert torch.allclose(clipped, g * c, rtol=1e-14, atol=0.0)
    R.assert_margin([0.3, 4.1], 1.0)
    with pytest.raises(AssertionError):
        R.assert_margin([0.3, 1.5], 1.0)
