"""The packed in-projection on the host (no GPU): ops.InProj, the one addressing of in_proj_weight [3E][E] / in_proj_bias [3E] and of
their gradient buffers, and what the writers of step-invariant context operands hand to the library -- ops.ctx_kv_cache16 (the fused
sampler's K rows / V planes), the instruction k | v projection of DiffusionHead.build_fused, ops.ctx_kv_operands16.  CPU tensors stand
for device memory; lib.call is replaced by a recorder and lib.stream by a constant.  Every expected pointer and argument tuple is
written out by hand (the tuples of the sampler cache from the launches build_fused used to issue itself), not produced by the code.
"""
import types

import pytest
import torch

from conftest import load_pkg

STREAM = 0x5EED
B, S, SP = 2, 70, 128                                                     # 70 keys: one full and one partial 64-key tile
P16, S16, LIN = "a3d_proj_rope_split16", "a3d_rope_split16", "a3d_linear_fwd"


@pytest.fixture()
def O(monkeypatch):
    ops = load_pkg().ops
    for k, v in dict(ATTN_MODE="f16", ROWS_ONLY=True, FUSED_PROJ=True).items():
        monkeypatch.setattr(ops, k, v)                                  # the defaults, whatever the environment says
    return ops


@pytest.fixture()
def seen(O, monkeypatch):
    """the (entry, *arguments) tuples of every lib.call, in order"""
    out = []
    monkeypatch.setattr(O.L, "call", lambda entry, *args: out.append((entry,) + args))
    monkeypatch.setattr(O.L, "stream", lambda: STREAM)
    return out


def packed(E, seed=0):
    """a module with the packed parameters, as nn.MultiheadAttention keeps them"""
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(in_proj_weight=torch.nn.Parameter(torch.randn(3 * E, E, generator=g)),
                                 in_proj_bias=torch.nn.Parameter(torch.randn(3 * E, generator=g)))


def context(E, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, E, generator=g), torch.rand(B, S, 3, generator=g)


@pytest.mark.parametrize("E", [60, 120, 30])
def test_addressing(O, E):
    m = packed(E)
    w, b = m.in_proj_weight, m.in_proj_bias
    ip = O.InProj(w, b, E)
    wp, bp = w.data_ptr(), b.data_ptr()
    assert (ip.wq, ip.wk, ip.wv) == (wp, wp + E * E * 4, wp + 2 * E * E * 4)
    assert (ip.bq, ip.bk, ip.bv) == (bp, bp + E * 4, bp + 2 * E * 4)
    assert all(type(getattr(ip, n)) is int for n in ("wq", "wk", "wv", "bq", "bk", "bv")) and not hasattr(ip, "__dict__")
    assert w.grad is None and b.grad is None                             # no gradient buffer before a gradient pointer is asked for
    g = ip.grad
    assert w.grad is not None and b.grad is not None and ip.grad is g
    assert w.grad.shape == w.shape and w.grad.is_contiguous() and not w.grad.any() and not b.grad.any()
    gw, gb = w.grad.data_ptr(), b.grad.data_ptr()
    assert (g.wq, g.wk, g.wv) == (gw, gw + E * E * 4, gw + 2 * E * E * 4)
    assert (g.bq, g.bk, g.bv) == (gb, gb + E * 4, gb + 2 * E * 4)
    assert g.weight is w.grad and g.bias is b.grad
    w.grad.fill_(1.0)
    again = O.InProj(w, b, E).grad                                       # an existing buffer is taken as it is
    assert again.wq == gw and again.bq == gb and bool(w.grad.all())
    # a group (first block, roles): group_layout's values, offsets from wq / bq
    assert ip.group(0, ("q",)) == O.group_layout(0, ("q",), E) == (0, 0, (0,), E)
    assert ip.group(1, ("k", "v")) == O.group_layout(1, ("k", "v"), E) == (E * E * 4, E * 4, (0, E * 4), 2 * E)
    assert ip.group(0, ("q", "k")) == O.group_layout(0, ("q", "k"), E) == (0, 0, (0, E * 4), 2 * E)
    assert ip.group(2, ("v",)) == O.group_layout(2, ("v",), E) == (2 * E * E * 4, 2 * E * 4, (0,), E)
    assert ip.wq + ip.group(1, ("k",))[0] == ip.wk and ip.bq + ip.group(2, ("v",))[1] == ip.bv
    # row slices, for the callers that need views
    assert ip.rows(0, ("q",)) == ip.rows(0, "q") == slice(0, E)
    assert ip.rows(1, ("k", "v")) == slice(E, 3 * E)
    assert ip.rows(2, ("v",)) == slice(2 * E, 3 * E)
    assert w[ip.rows(1, ("k", "v"))].data_ptr() == ip.wk and w.grad[ip.rows(2, ("v",))].data_ptr() == g.wv
    assert b[ip.rows(1, ("k", "v"))].data_ptr() == ip.bk and tuple(w[ip.rows(1, ("k", "v"))].shape) == (2 * E, E)


@pytest.mark.parametrize("E,H", [(60, 4), (120, 8)])
@pytest.mark.parametrize("switches", [{}, dict(ROWS_ONLY=False), dict(ATTN_MODE="bf16x3"), dict(ATTN_MODE="fp8")])
def test_context_cache_fused(O, seen, monkeypatch, E, H, switches):
    """One a3d_proj_rope_split16 for k | v: K rows (parts 2, rotated), V planes (parts 2 | 4); the operand-set switches of the training
    side do not enter (dn_cross reads K rows + V planes)."""
    for k, v in switches.items():
        monkeypatch.setattr(O, k, v)
    m, (ctx, xyz) = packed(E), context(E)
    Kf, Vt = O.ctx_kv_cache16(ctx, xyz, m, H)
    assert tuple(Kf.shape) == (B, H, SP, 32) and tuple(Vt.shape) == (B, H, 2, 16, SP)
    assert Kf.dtype == Vt.dtype == torch.float16 and Kf.is_contiguous() and Vt.is_contiguous()
    x, w, b, freq = ctx.data_ptr(), m.in_proj_weight.data_ptr(), m.in_proj_bias.data_ptr(), O.rope_freq(E, ctx.device).data_ptr()
    assert seen == [(P16, x, E, w + E * E * 4, E, b + E * 4, E, xyz.data_ptr(), 1.0, Kf.data_ptr(), None, 2, None, 1.0, None, Vt.data_ptr(),
                     6, freq, B, S, SP, E, H, STREAM)]


@pytest.mark.parametrize("E,H", [(30, 2), (90, 6)])
def test_context_cache_unfused(O, seen, E, H):
    """E % 4 != 0 (the smallest such widths): one linear launch for k | v, then one formatting launch per operand, k before v."""
    m, (ctx, xyz) = packed(E), context(E)
    Kf, Vt = O.ctx_kv_cache16(ctx, xyz, m, H)
    assert tuple(Kf.shape) == (B, H, SP, 32) and tuple(Vt.shape) == (B, H, 2, 16, SP)
    x, w, b, freq = ctx.data_ptr(), m.in_proj_weight.data_ptr(), m.in_proj_bias.data_ptr(), O.rope_freq(E, ctx.device).data_ptr()
    assert len(seen) == 3
    kv = seen[0][6]                                                      # the [B S][2E] fp32 rows the linear launch writes
    assert isinstance(kv, int) and kv != 0
    assert seen[0] == (LIN, x, E, w + E * E * 4, E, b + E * 4, kv, 2 * E, None, 0, B * S, 2 * E, E, 0, 0, STREAM)
    assert seen[1] == (S16, kv, 2 * E, xyz.data_ptr(), freq, 1.0, Kf.data_ptr(), None, 2, B, S, SP, E, H, STREAM)
    assert seen[2] == (S16, kv + E * 4, 2 * E, None, freq, 1.0, None, Vt.data_ptr(), 2 | 4, B, S, SP, E, H, STREAM)


def test_fused_projection_switch_reaches_the_context_cache(O, seen, monkeypatch):
    monkeypatch.setattr(O, "FUSED_PROJ", False)
    O.ctx_kv_cache16(*context(60), packed(60), 4)
    assert [s[0] for s in seen] == [LIN, S16, S16]


def test_build_fused_context_layers_and_instruction_projection(O, seen):
    """DiffusionHead.build_fused on a stand-in head with one cross-attention layer: the layer's operands through ops.ctx_kv_cache16, its
    three AdaLN tables, then the instruction tokens through the k | v rows of traj_lang_attention's projection in ONE linear launch."""
    E, H, S_lang, T, Ln = 60, 4, 7, 4, 5
    D = load_pkg().diffusion
    ada = lambda: types.SimpleNamespace(modulation=[None, torch.nn.Linear(E, 2 * E)])
    lay = types.SimpleNamespace(cross_12=packed(E, 2), adaln_12=ada(), adaln_1=ada(), adaln_ff1=ada())
    lang = packed(E, 3)
    head = types.SimpleNamespace(num_attn_heads=H, use_instruction=True, _cross_layers=lambda: [lay],
                                 _sem=lambda n, e, dev: torch.zeros(n, e),
                                 traj_lang_attention=[types.SimpleNamespace(layers=[types.SimpleNamespace(cross_12=lang)])])
    ctx, xyz = context(E)
    instr = torch.randn(B, S_lang, E)
    st = D.DiffusionHead.build_fused(head, ctx, xyz, instr, None, torch.randn(T, E), Ln)
    assert [s[0] for s in seen] == [P16, LIN, LIN, LIN, LIN]
    rec = st["layers"][0]
    x, w, b, freq = ctx.data_ptr(), lay.cross_12.in_proj_weight.data_ptr(), lay.cross_12.in_proj_bias.data_ptr(), st["freq"].data_ptr()
    assert seen[0] == (P16, x, E, w + E * E * 4, E, b + E * 4, E, xyz.data_ptr(), 1.0, rec["Kf"].data_ptr(), None, 2, None, 1.0, None,
                       rec["Vt"].data_ptr(), 6, freq, B, S, SP, E, H, STREAM)
    w, b, kv = lang.in_proj_weight.data_ptr(), lang.in_proj_bias.data_ptr(), st["lang_kv"]
    assert tuple(kv.shape) == (B * S_lang, 2 * E) and st["S_lang"] == S_lang
    assert seen[4] == (LIN, instr.data_ptr(), E, w + E * E * 4, E, b + E * 4, kv.data_ptr(), 2 * E, None, 0, B * S_lang, 2 * E, E, 0, 0,
                       STREAM)
    assert [t.data_ptr() for t in st["tensors"]] == [t.data_ptr() for t in [rec["Kf"], rec["Vt"]] + rec["mods"] + [kv]]


@pytest.mark.parametrize("layers", [1, 2])
def test_ctx_kv_operands16_pointer_block(O, seen, monkeypatch, layers):
    """a3d_ctx_kv_proj16 takes (Wk, bk, Kr, Vr) of up to two layers: the k | v block of each layer's packed parameters, NULLs beyond."""
    monkeypatch.setattr(O.L, "require_gpu", lambda *tensors: None)       # CPU tensors stand for device memory here
    E, H = 60, 4
    mhas, (ctx, xyz) = [packed(E, 5 + j) for j in range(layers)], context(E)
    pairs = O.ctx_kv_operands16(ctx, xyz, mhas, H)
    assert len(pairs) == layers and all(tuple(t.shape) == (B, H, SP, 32) and t.dtype == torch.float16 for p in pairs for t in p)
    block = []
    for m, (Kr, Vr) in zip(mhas, pairs):
        block += [m.in_proj_weight.data_ptr() + E * E * 4, m.in_proj_bias.data_ptr() + E * 4, Kr.data_ptr(), Vr.data_ptr()]
    block += [None, None, None, None] * (2 - layers)
    assert len(block) == 8
    assert seen == [("a3d_ctx_kv_proj16", ctx.data_ptr(), E, xyz.data_ptr(), *block, E, O.rope_freq(E, ctx.device).data_ptr(), layers,
                     B, S, SP, E, H, 0, STREAM)]
