"""EMA of the weights, the parts that need no GPU: the argument checks of a3d_adamw_ema_step / a3d_swap_f32 (they run on the host
before any launch), FlatAdamW's EMA bookkeeping on CPU tensors (nothing is launched), the checkpoint format, and the warm-up table
of the float64 reference (tests/ema_ref.py)."""
import ctypes
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ema_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ C-ABI
def test_symbols_exported_with_signatures(a3d):
    lib = a3d.lib.load()
    for name in ("a3d_adamw_ema_step", "a3d_swap_f32"):
        assert name in a3d.lib.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(HERE), "include", "act3d_hip.h")).read()
    assert "int a3d_adamw_ema_step(" in header and "int a3d_swap_f32(" in header


def _ema_step_args(**over):
    """A valid argument list over host memory that is never dereferenced: every case below must be rejected before a launch."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    a = dict(p=p, g=p, m=p, v=p, ema=p, step=p, seg_off=p, seg_state=p, ema_state=p, nseg=1, n=16, n_nodecay=0, lr=1e-4, beta1=0.9,
             beta2=0.999, eps=1e-8, wd0=0.0, wd1=5e-4, gscale=1.0, ema_decay=0.999, ema_warmup=10.0, stream=None)
    a.update(over)
    return buf, list(a.values())


@pytest.mark.parametrize("over", [dict(ema=None), dict(ema_state=None), dict(p=None), dict(nseg=0), dict(ema_decay=1.0),
                                  dict(ema_decay=-0.1), dict(ema_decay=float("nan")), dict(ema_decay=float("inf")),
                                  dict(ema_warmup=0.5), dict(ema_warmup=-1.0), dict(ema_warmup=float("nan")),
                                  dict(ema_warmup=float("inf"))],
                         ids=lambda o: "%s=%s" % next(iter(o.items())))
def test_adamw_ema_step_rejects_bad_arguments(a3d, over):
    lib = a3d.lib.load()
    keep, args = _ema_step_args(**over)
    assert lib.a3d_adamw_ema_step(*args) == -22
    assert "a3d_adamw_ema_step" in a3d.lib.last_error()
    del keep


def test_swap_rejects_null_and_overlap(a3d):
    lib = a3d.lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for a, b, n in ((None, p, 4), (p, None, 4), (p, p, 4), (p, p + 4, 4), (p + 12, p, 4), (p, p + 15 * 4, 16)):
        assert lib.a3d_swap_f32(a, b, n, None) == -22, (a, b, n)
        assert "a3d_swap_f32" in a3d.lib.last_error()
    assert lib.a3d_swap_f32(None, None, 0, None) == 0                    # n = 0: nothing to do, nothing to check


# ------------------------------------------------------------------------------------------------ optimizer
def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 3))


def _swap_by_hand(opt):
    tmp = opt.flat.flat.clone()
    opt.flat.flat.copy_(opt.ema)
    opt.ema.copy_(tmp)
    opt.ema_swapped = not opt.ema_swapped


def test_ema_off_is_todays_optimizer(a3d):
    E = a3d.engine
    flat, opt = E.get_optimizer(_model())
    assert opt.ema is None and opt.ema_state is None and opt.ema_swapped is False
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and sd["state"] == {}
    flat2, opt2 = E.get_optimizer(_model(), ema_decay=0.999)
    sd2 = opt2.state_dict()
    assert sd2["param_groups"] == sd["param_groups"] and sd2["state"] == {}, "the EMA must not leak into torch's AdamW layout"
    with opt.ema_weights():                                               # no EMA: a no-op, callers need no branch
        pass
    for call in (opt.swap_ema, opt.reset_ema, opt.ema_state_dict):
        with pytest.raises(RuntimeError):
            call()


@pytest.mark.parametrize("kw", [dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=float("nan")),
                                dict(ema_decay=0.9, ema_warmup=0.5), dict(ema_decay=0.9, ema_warmup=-1),
                                dict(ema_decay=0.9, ema_warmup=float("inf"))])
def test_bad_keywords_raise(a3d, kw):
    E = a3d.engine
    with pytest.raises(ValueError):
        E.get_optimizer(_model(), **kw)
    flat = E.FlatParams(_model())
    with pytest.raises(ValueError):
        E.FlatAdamW(flat, **kw)


def test_reset_state_dict_and_swapped_guards(a3d, tmp_path):
    E = a3d.engine
    m = _model()
    flat, opt = E.get_optimizer(m, ema_decay=0.99, ema_warmup=0)
    assert torch.equal(opt.ema, flat.flat) and opt.ema.data_ptr() != flat.flat.data_ptr()
    assert opt.ema_state.shape == (4,) and float(opt.ema_updates) == 0.0
    assert opt.ema_updates.data_ptr() == opt.ema_state.data_ptr() + 4, "ema_updates is a view of ema_state[1]"
    # the average somewhere else, the counter advanced -> reset_ema() brings both back
    opt.ema.add_(1.0)
    opt.ema_state[1] = 7.0
    opt.reset_ema()
    assert torch.equal(opt.ema, flat.flat) and float(opt.ema_state.abs().sum()) == 0.0
    opt.ema.mul_(0.5)
    opt.ema_state[1] = 3.0
    opt.reset_state()
    assert torch.equal(opt.ema, flat.flat) and float(opt.ema_updates) == 0.0, "reset_state() also restarts the EMA"
    # names, shapes, values -- in both swap states
    opt.ema.copy_(flat.flat * 0.5 + 0.25)
    want = {n: (p.detach() * 0.5 + 0.25) for n, p in m.named_parameters()}
    sd = opt.ema_state_dict()
    assert list(sd) == [n for n, _ in flat.order] and set(sd) == set(want)
    for n, v in sd.items():
        assert v.shape == want[n].shape and torch.equal(v, want[n]) and v.data_ptr() != opt.ema.data_ptr()
    raw = flat.flat.clone()
    _swap_by_hand(opt)
    assert opt.ema_swapped and torch.equal(opt.ema, raw)
    sd2 = opt.ema_state_dict()
    assert all(torch.equal(sd2[n], sd[n]) for n in sd), "ema_state_dict() follows the averages into the flat buffer"
    with pytest.raises(RuntimeError, match="swapped"):
        opt.step()
    with pytest.raises(RuntimeError, match="swapped"):
        E.save_checkpoint(str(tmp_path / "no.pth"), m, opt, 0)
    assert not (tmp_path / "no.pth").exists()
    _swap_by_hand(opt)
    assert torch.equal(flat.flat, raw)


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_reseed_and_ema_weights(a3d, tmp_path, capsys):
    E = a3d.engine
    m = _model(1)
    m.register_buffer("calib", torch.arange(3.0))                        # a non-parameter entry of "weight"
    flat, opt = E.get_optimizer(m, ema_decay=0.999, ema_warmup=10)
    opt.ema.copy_(torch.randn(flat.n, generator=torch.Generator().manual_seed(3)))
    opt.ema_state[1] = 5.0
    path = str(tmp_path / "ema.pth")
    E.save_checkpoint(path, m, opt, 4, best_loss=0.5)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"weight", "optimizer", "iter", "best_loss", "ema"}
    assert set(ck["ema"]) == {"weight", "decay", "warmup", "updates"}
    assert ck["ema"]["decay"] == 0.999 and ck["ema"]["warmup"] == 10 and ck["ema"]["updates"] == 5
    assert set(ck["ema"]["weight"]) == {"module." + n for n, _ in flat.order}
    for n, v in opt.ema_state_dict().items():
        assert torch.equal(ck["ema"]["weight"]["module." + n], v)
        assert not torch.equal(ck["weight"]["module." + n], v)
    # resume into an EMA optimizer: average and counter come back
    m2 = _model(2)
    m2.register_buffer("calib", torch.zeros(3))
    flat2, opt2 = E.get_optimizer(m2, ema_decay=0.999, ema_warmup=10)
    assert E.load_checkpoint(path, m2, opt2) == (5, 0.5)
    assert torch.equal(flat2.flat, flat.flat) and torch.equal(opt2.ema, opt.ema) and float(opt2.ema_updates) == 5.0
    # an optimizer without EMA ignores the key
    m3 = _model(2)
    m3.register_buffer("calib", torch.zeros(3))
    flat3, opt3 = E.get_optimizer(m3)
    E.load_checkpoint(path, m3, opt3)
    assert opt3.ema is None and torch.equal(flat3.flat, flat.flat)
    # deployment: weights="ema" -> trained parameters are the averages, everything else is "weight"
    m4 = _model(2)
    m4.register_buffer("calib", torch.zeros(3))
    E.load_checkpoint(path, m4, weights="ema")
    sd4 = m4.state_dict()
    for n, _ in flat.order:
        assert torch.equal(sd4[n], ck["ema"]["weight"]["module." + n])
    assert torch.equal(sd4["calib"], ck["weight"]["module.calib"])
    with pytest.raises(ValueError):
        E.load_checkpoint(path, m4, weights="average")
    with pytest.raises(ValueError):
        E.load_checkpoint(path, m2, opt2, weights="ema")                 # a resumed run starts from the raw weights
    # a size mismatch in the averages raises
    bad = dict(ck)
    bad["ema"] = dict(ck["ema"], weight={k: (v[:1] if k == "module.0.bias" else v) for k, v in ck["ema"]["weight"].items()})
    torch.save(bad, str(tmp_path / "bad.pth"))
    with pytest.raises(RuntimeError):
        E.load_checkpoint(str(tmp_path / "bad.pth"), m4, weights="ema")
    with pytest.raises(RuntimeError):
        E.load_checkpoint(str(tmp_path / "bad.pth"), m2, opt2)

    # a file WITHOUT "ema": exactly today's four keys; an EMA optimizer reseeds from the loaded weights, weights="ema" raises
    plain = str(tmp_path / "plain.pth")
    E.save_checkpoint(plain, m3, opt3, 9)
    assert set(torch.load(plain, map_location="cpu", weights_only=False)) == {"weight", "optimizer", "iter", "best_loss"}
    m5 = _model(7)
    m5.register_buffer("calib", torch.zeros(3))
    flat5, opt5 = E.get_optimizer(m5, ema_decay=0.9)
    opt5.ema_state[1] = 4.0
    capsys.readouterr()
    E.load_checkpoint(plain, m5, opt5)
    assert len(capsys.readouterr().out.strip().splitlines()) == 1
    assert torch.equal(flat5.flat, flat3.flat) and torch.equal(opt5.ema, flat5.flat) and float(opt5.ema_updates) == 0.0
    with pytest.raises(RuntimeError, match="ema"):
        E.load_checkpoint(plain, m4, weights="ema")


# ------------------------------------------------------------------------------------------------ warm-up table
def test_warmup_table():
    assert R.ema_weight(1, 0.999, 10) == 9.0 / 11.0
    # decay form of the same number: min(decay, (1 + t) / (warmup + t))
    for t in (1, 2, 50, 8990, 8991, 8992, 10 ** 6):
        assert math.isclose(1.0 - R.ema_weight(t, 0.999, 10), min(0.999, (1.0 + t) / (10.0 + t)), rel_tol=0, abs_tol=1e-15)
    first = next(t for t in range(1, 20000) if (10 - 1.0) / (10 + t) < 1 - 0.999)
    # 9 / (10 + t) < 1e-3  <=>  t > 8990 in exact arithmetic; the double 1 - 0.999 lies a few ulps above 1e-3, so t = 8990 may tie
    assert first in (8990, 8991)
    assert R.ema_weight(first - 1, 0.999, 10) > 1 - 0.999 and R.ema_weight(first, 0.999, 10) == 1 - 0.999
    assert all(R.ema_weight(t, 0.999, 10) == 1 - 0.999 for t in (first, first + 1, 10 ** 6))
    assert all(R.ema_weight(t, 0.9, 0) == 1 - 0.9 for t in (1, 2, 100, 10 ** 6))
    assert R.ema_weight(1, 0.9, 1) == 1 - 0.9                            # warm-up 1: (1 + t) / (1 + t) = 1 never binds
    e = R.ema_update(torch.zeros(3, dtype=torch.float64), torch.ones(3), 1, 0.999, 10, active=torch.tensor([True, False, True]))
    assert e.tolist() == [9.0 / 11.0, 0.0, 9.0 / 11.0]
