"""Host-side validation of the eight attention-core entries (csrc/attn_launch.h): one order for all of them -- shapes, dropout
arguments, pointers -- with -22 and the name of the entry that was CALLED in a3d_last_error_string().

Every call in this file is one the host refuses, so nothing is launched on a machine that has a GPU either: the shape and dropout
cases pass NULL for every tensor (they are refused before the pointer check, and would be refused by it otherwise), and the
non-NULL pointers of the workspace cases are dummies that are never dereferenced."""
import ctypes

import pytest

from conftest import load_pkg

BASE = dict(B=1, H=4, Lq=10, Lqp=64, S=70, Sp=128, nsplit=1)
PTR = ctypes.c_void_p(256)                           # 256-byte aligned, never dereferenced
MASKW_KEYS = 512 * 32                                # attn_ring.h MASKW * 32: the key bitmask of the fp16 / fp8 kernels


def _shape(s):
    return (s["B"], s["H"], s["Lq"], s["Lqp"], s["S"], s["Sp"], s["nsplit"])


def _drop(state, p):
    return (state, 7, p)


# name -> (args(shape, tensor pointer, ws pointer, dropout state, p), Lqp modulus, Sp limited, takes dropout, takes ws)
ENTRIES = {
    "a3d_attn_fwd": (lambda s, t, ws, st, p: (t, t, t, None, t, t, ws) + _shape(s) + (None,), 16, False, False, True),
    "a3d_attn_fwd_dropout": (lambda s, t, ws, st, p: (t, t, t, None, t, t, ws) + _shape(s) + _drop(st, p) + (None,),
                             16, False, True, True),
    "a3d_attn_bwd_bf16": (lambda s, t, ws, st, p: (t,) * 5 + (None,) + (t,) * 9 + _shape(s) + (None,), 64, False, False, False),
    "a3d_attn_bwd_bf16_dropout": (lambda s, t, ws, st, p: (t,) * 5 + (None,) + (t,) * 9 + _shape(s) + _drop(st, p) + (None,),
                                  64, False, True, False),
    "a3d_attn16_fwd": (lambda s, t, ws, st, p: (t, t, t, None, t, t, ws) + _shape(s) + _drop(st, p) + (None,), 16, True, True, True),
    "a3d_attn16_fwd_rows": (lambda s, t, ws, st, p: (t, t, t, None, t, t, ws) + _shape(s) + _drop(st, p) + (0, None),
                            16, True, True, True),
    "a3d_attn16_bwd": (lambda s, t, ws, st, p: (t,) * 5 + (None,) + (t,) * 10 + _shape(s) + _drop(st, p) + (None,),
                       64, True, True, False),
    "a3d_attn8_fwd": (lambda s, t, ws, st, p: (t, t, t, t, None, t, t, ws) + _shape(s) + (None,), 16, True, False, True),
}
DROPOUT_ONLY = ("a3d_attn_fwd_dropout", "a3d_attn_bwd_bf16_dropout")        # refuse a NULL state
names = pytest.mark.parametrize("name", sorted(ENTRIES))


@pytest.fixture(scope="module")
def lib():
    return load_pkg().lib.load()


def _refused(lib, name, args, *needles):
    assert getattr(lib, name)(*args) == -22, name
    msg = lib.a3d_last_error_string()
    assert msg.startswith(name.encode() + b":"), (name, msg)                # the entry that was called, not a shorter name's
    for n in needles:
        assert n in msg, (name, n, msg)


def _state(name):
    return PTR if name in DROPOUT_ONLY else None


@names
def test_bad_shapes_are_refused_under_the_called_name(lib, name):
    args, qmod, sp_limited, _, _ = ENTRIES[name]
    cases = [dict(B=0), dict(H=0), dict(Lq=0), dict(Lq=80), dict(Lqp=72 if qmod == 16 else 80), dict(S=0), dict(Sp=64), dict(Sp=96),
             dict(nsplit=0), dict(nsplit=65)]
    if sp_limited:
        cases.append(dict(Sp=MASKW_KEYS + 64))                               # 16448
    for c in cases:
        s = dict(BASE, **c)
        if "Lqp" in c:
            assert s["Lqp"] >= s["Lq"] and s["Lqp"] % qmod != 0
        _refused(lib, name, args(s, None, None, _state(name), 0.1), b"bad argument")


@names
def test_null_pointers_are_refused(lib, name):
    args, _, _, _, takes_ws = ENTRIES[name]
    _refused(lib, name, args(BASE, None, None, _state(name), 0.1), b"null pointer")
    if takes_ws:                                                              # split results need the workspace
        _refused(lib, name, args(dict(BASE, nsplit=2), PTR, None, _state(name), 0.1), b"null pointer")


@pytest.mark.parametrize("name", sorted(n for n in ENTRIES if ENTRIES[n][3]))
def test_dropout_probability_is_checked_before_the_pointers(lib, name):
    args = ENTRIES[name][0]
    for p in (-0.1, 1.0, 1.5, float("nan")):
        _refused(lib, name, args(BASE, None, None, PTR, p), b"dropout probability")


@pytest.mark.parametrize("name", DROPOUT_ONLY)
def test_dropout_entries_refuse_a_null_state(lib, name):
    _refused(lib, name, ENTRIES[name][0](BASE, None, None, None, 0.1), b"null dropout state")
