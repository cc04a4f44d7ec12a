"""Kernel-level parity: every C-ABI entry point of libact3d_hip.so against the CPU oracle / plain torch fp32.

All tests here need the MI355X (`-m gpu`).  They go through the ctypes C-ABI (ops.py -> lib.py -> .so).
Tolerances: indices bit-exact; fp32 kernels 1e-5 class; attention 1e-3 absolute as BASELINE.json's north_star states
(measured errors are ~1e-5, printed by `report`).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg
from oracle import act3d as OA
from oracle import blocks as OB

pytestmark = pytest.mark.gpu


def report(name, got, ref, atol, rtol=0.0):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    worst = (err - tol).max().item()
    print(f"[parity] {name}: max_abs_err={err.max().item():.3e} ref_absmax={ref.abs().max().item():.3e}")
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    if worst > 0:
        idx = torch.nonzero(err > tol)[:5]
        raise AssertionError(f"{name}: max err {err.max().item():.3e} > tol; first bad idx {idx.tolist()} "
                             f"got {[got[tuple(i)].item() for i in idx]} ref {[ref[tuple(i)].item() for i in idx]}")


def report_grad(a3d, name, got, ref, atol, rtol=0.0):
    """Gradient parity of the attention blocks: the same element-wise bound for both kernel families.  (The first cut of the
    split-fp16 family carried single-fp16 dO and weights and needed 1e-3 of the tensor's scale here; with two-part operands
    throughout its errors are at or below the split-bf16 family's on every output, profiles/r03_attn_family_check.txt.)"""
    report(name, got, ref, atol, rtol)


def report_scaled(name, got, ref, tol=1.5e-3):
    """|got - ref| <= tol * max|ref| element-wise: the bound for parameter gradients (sums over all rows of a batch), stated
    relative to the tensor's own scale as north_star does (1e-3 class; 1.5e-3 as for the model-level gradients)."""
    report(name, got, ref, tol * ref.detach().abs().max().item())


def bf16_bits(x):
    return x.to(torch.bfloat16).view(torch.int16)


def test_library_loads(a3d):
    assert a3d.lib.load().a3d_version() >= 100


def test_mfma_layout_probes(a3d, dev):
    """Pins the MFMA operand / result lane mappings every kernel assumes (asymmetric A and B)."""
    L = a3d.lib
    g = torch.Generator().manual_seed(0)
    A = torch.randn(16, 32, generator=g).to(torch.bfloat16)
    Bm = torch.randn(32, 16, generator=g).to(torch.bfloat16)
    D = torch.zeros(16, 16, device=dev)
    Ad, Bd = A.to(dev).contiguous(), Bm.to(dev).contiguous()     # keep alive: raw pointers are passed
    L.call("a3d_dbg_mfma_bf16", Ad.data_ptr(), Bd.data_ptr(), D.data_ptr(), L.stream())
    report("mfma_bf16_16x16x32", D, A.float() @ Bm.float(), 1e-4)
    A4 = torch.randn(16, 4, generator=g)
    B4 = torch.randn(4, 16, generator=g)
    D2 = torch.zeros(16, 16, device=dev)
    A4d, B4d = A4.to(dev), B4.to(dev)
    L.call("a3d_dbg_mfma_f32", A4d.data_ptr(), B4d.data_ptr(), D2.data_ptr(), L.stream())
    report("mfma_f32_16x16x4", D2, A4 @ B4, 1e-6)


def test_linear_large_m_reads_weights_at_4_byte_alignment(a3d, dev):
    """The large-M (bf16x3, linear_split.hip) path with weights and bias that sit at odd float offsets of one buffer, as the
    parameters do inside engine.FlatParams: forward, ReLU and the transposed-weight (dgrad) read."""
    O = a3d.ops
    g = torch.Generator().manual_seed(3)
    M, N, K = 5000, 120, 60
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    flat = torch.zeros(N * K + N + 7, device=dev)
    wd = flat[1:1 + N * K].view(N, K)
    bd = flat[3 + N * K:3 + N * K + N]
    wd.copy_(w)
    bd.copy_(b)
    assert wd.data_ptr() % 16 != 0 and bd.data_ptr() % 16 != 0
    report("linear_fwd, unaligned W", O.linear2d(x.to(dev), wd, bd, act=1), F.relu(F.linear(x, w, b)), 2e-5, 1e-5)
    dy = torch.randn(M, N, generator=g)
    report("linear_dgrad, unaligned W", O.dgrad2d(dy.to(dev), wd), dy @ w, 2e-5, 1e-5)


@pytest.mark.parametrize("M,N,K", [(1, 5, 60), (333, 60, 60), (1000, 120, 60), (70, 480, 120), (257, 120, 480),
                                   (50, 60, 512), (33, 120, 9), (130, 3, 120), (106, 240, 120), (2048, 120, 120),
                                   (4098, 240, 120), (65552, 120, 60), (20011, 60, 60)])
def test_linear_fwd_dgrad_wgrad(a3d, dev, M, N, K):
    O = a3d.ops
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    y = O.linear2d(x.to(dev), w.to(dev), b.to(dev))
    report(f"linear_fwd {M}x{N}x{K}", y, F.linear(x, w, b), 2e-5, 1e-5)
    yr = O.linear2d(x.to(dev), w.to(dev), b.to(dev), act=1)
    report("linear_fwd relu", yr, F.relu(F.linear(x, w, b)), 2e-5, 1e-5)
    dy = torch.randn(M, N, generator=g)
    dx = O.dgrad2d(dy.to(dev), w.to(dev))
    report("linear_dgrad", dx, dy @ w, 2e-5, 1e-5)
    mask = torch.randn(M, K, generator=g)
    dxm = O.dgrad2d(dy.to(dev), w.to(dev), mask=mask.to(dev))
    report("linear_dgrad relu-mask", dxm, (dy @ w) * (mask > 0), 2e-5, 1e-5)
    W = torch.nn.Parameter(w.to(dev))
    Bp = torch.nn.Parameter(b.to(dev))
    O.wgrad2d(dy.to(dev), x.to(dev), W, Bp)
    O.wgrad2d(dy.to(dev), x.to(dev), W, Bp)   # accumulates
    report("linear_wgrad dW", W.grad, 2 * (dy.t() @ x), 1e-4 * max(1.0, math.sqrt(M) / 4), 1e-5)
    report("linear_wgrad db", Bp.grad, 2 * dy.sum(0), 1e-4 * max(1.0, math.sqrt(M) / 4), 1e-5)
    two_stage = a3d.lib.load().a3d_linear_wgrad_ws_bytes(M, N, K, 1) > 0
    assert two_stage == (M >= 1024)         # all but the tiny reductions take the atomics-free, ordered path
    if two_stage:                           # ... which is run-to-run deterministic
        W2 = torch.nn.Parameter(w.to(dev))
        B2 = torch.nn.Parameter(b.to(dev))
        O.wgrad2d(dy.to(dev), x.to(dev), W2, B2)
        O.wgrad2d(dy.to(dev), x.to(dev), W2, B2)
        assert torch.equal(W2.grad, W.grad) and torch.equal(B2.grad, Bp.grad)


@pytest.mark.parametrize("M,E", [(5, 60), (1333, 60), (700, 120), (9, 480)])
def test_add_layernorm(a3d, dev, M, E):
    O = a3d.ops
    g = torch.Generator().manual_seed(E + M)
    a = torch.randn(M, E, generator=g, requires_grad=True)
    r = torch.randn(M, E, generator=g, requires_grad=True)
    gam = (torch.rand(E, generator=g) + 0.5).requires_grad_()
    bet = torch.randn(E, generator=g).requires_grad_()
    ref = F.layer_norm(a + r, (E,), gam, bet, 1e-5)
    dy = torch.randn(M, E, generator=g)
    ref.backward(dy)
    G, Bt = torch.nn.Parameter(gam.detach().to(dev)), torch.nn.Parameter(bet.detach().to(dev))
    y, mean, rstd = O.add_layernorm(a.detach().to(dev), r.detach().to(dev), G, Bt)
    report("add_ln fwd", y, ref, 2e-5)
    ds = O.add_layernorm_bwd(a.detach().to(dev), r.detach().to(dev), G, Bt, mean, rstd, dy.to(dev))
    report("add_ln dS", ds, a.grad, 5e-5)
    report("add_ln dgamma", G.grad, gam.grad, 2e-4 * max(1, math.sqrt(M) / 8), 1e-5)
    report("add_ln dbeta", Bt.grad, bet.grad, 2e-4 * max(1, math.sqrt(M) / 8), 1e-5)


def _mha_params(E, g, scale=1.0):
    in_w = torch.randn(3 * E, E, generator=g) * scale / math.sqrt(E)
    in_b = torch.randn(3 * E, generator=g) * 0.1
    out_w = torch.randn(E, E, generator=g) / math.sqrt(E)
    out_b = torch.randn(E, generator=g) * 0.1
    return in_w, in_b, out_w, out_b


class _Mod:
    pass


def _mk_modules(dev, in_w, in_b, out_w, out_b, ln_g, ln_b):
    mha = _Mod()
    if in_w.shape[1] == 60:
        # as inside engine.FlatParams: a 4-byte-aligned view into a larger buffer (exercises the unaligned-W path of the
        # fused projection kernel); the E = 120 cases keep a 16-byte-aligned weight
        buf = torch.zeros(in_w.numel() + 1, device=dev)
        buf[1:].copy_(in_w.reshape(-1))
        mha.in_proj_weight = torch.nn.Parameter(buf[1:].view(in_w.shape))
        assert mha.in_proj_weight.data_ptr() % 16 == 4
    else:
        mha.in_proj_weight = torch.nn.Parameter(in_w.to(dev))
    mha.in_proj_bias = torch.nn.Parameter(in_b.to(dev))
    mha.out_proj = _Mod()
    mha.out_proj.weight = torch.nn.Parameter(out_w.to(dev))
    mha.out_proj.bias = torch.nn.Parameter(out_b.to(dev))
    norm = _Mod()
    norm.weight = torch.nn.Parameter(ln_g.to(dev))
    norm.bias = torch.nn.Parameter(ln_b.to(dev))
    return mha, norm


@pytest.mark.parametrize("B,Lq,S,E,H,rope,masked,mode", [
    (2, 37, 131, 60, 4, True, False, "kv"),
    (2, 16, 70, 120, 8, True, True, "qk"),
    (3, 1, 200, 60, 4, False, False, "kv"),        # Lq = 1: the single-query kernels (csrc/single_query.hip), no RoPE (level 0)
    (2, 1, 70, 60, 4, True, False, "kv"),           # ... with RoPE, one full + one partial 64-key tile
    (2, 1, 4097, 60, 4, True, False, "kv"),         # ... the query stream at cfg-2's context length (key splits)
    (2, 333, 1025, 60, 4, True, False, "kv"),
    (2, 100, 53, 120, 8, False, False, "none"),
    (1, 130, 4097, 60, 4, True, False, "kv"),
    (2, 1024, 53, 120, 8, False, False, "kv"),      # vision -> language attention of the diffusion head
    (2, 8, 1026, 120, 8, True, False, "kv"),        # trajectory -> context cross-attention of the diffusion head
])
def test_attn_block_fwd_bwd(a3d, dev, B, Lq, S, E, H, rope, masked, mode):
    """AttnBlockFn (projections + RoPE + attention core + out-proj + residual LayerNorm) vs oracle.mha, incl. all grads."""
    O = a3d.ops
    g = torch.Generator().manual_seed(B * 1000 + Lq + S)
    in_w, in_b, out_w, out_b = _mha_params(E, g, scale=2.0)
    ln_g = torch.rand(E, generator=g) + 0.5
    ln_b = torch.randn(E, generator=g) * 0.1
    if mode == "qk":
        S = Lq
    xq = torch.randn(B, Lq, E, generator=g)
    xk = torch.randn(B, S, E, generator=g) if mode != "qk" else xq
    xv = xk if mode == "kv" else torch.randn(B, S, E, generator=g)
    resid = torch.randn(B, Lq, E, generator=g)
    q_xyz = torch.rand(B, Lq, 3, generator=g) * 2 - 0.5 if rope else None
    k_xyz = (torch.rand(B, S, 3, generator=g) * 2 - 0.5 if mode != "qk" else q_xyz) if rope else None
    kmask = None
    if masked:
        kmask = torch.zeros(B, S, dtype=torch.bool)
        kmask[:, -(S // 4):] = True
    # ---- oracle (CPU, autograd)
    leaves = [t.clone().requires_grad_() for t in (xq, xk, xv, resid, in_w, in_b, out_w, out_b, ln_g, ln_b)]
    cq, ck, cv, cr, ciw, cib, cow, cob, cg, cb = leaves
    if mode == "qk":
        ck = cq
    if mode == "kv":
        cv = ck
    o = OB.mha(cq, ck, cv, ciw, cib, cow, cob, H, q_xyz, k_xyz, kmask)
    ref = OB.layer_norm(cr + o, cg, cb)
    dy = torch.randn(B, Lq, E, generator=g)
    ref.backward(dy)
    # ---- device
    mha, norm = _mk_modules(dev, in_w, in_b, out_w, out_b, ln_g, ln_b)
    dq = xq.to(dev).requires_grad_()
    dk = dq if mode == "qk" else xk.to(dev).requires_grad_()
    dv = dk if mode == "kv" else xv.to(dev).requires_grad_()
    dr = resid.to(dev).requires_grad_()
    y = O.attn_block(dq, dk, dv, dr, None if q_xyz is None else q_xyz.to(dev), None if k_xyz is None else k_xyz.to(dev),
                     None if kmask is None else kmask.to(dev), mha, norm, H)
    report(f"attn_block[{mode}] fwd", y, ref, 1e-4)      # observed ~1e-5: fp32-grade logits (three-part q, k operands)
    y.backward(dy.to(dev))
    gtol = 5e-4
    report_grad(a3d, "attn_block d q_in", dq.grad, cq.grad, gtol, 1e-3)
    if mode == "none" or mode == "kv":
        report_grad(a3d, "attn_block d k_in", dk.grad, ck.grad, gtol, 1e-3)
    if mode != "kv":
        report_grad(a3d, "attn_block d v_in", dv.grad, cv.grad, gtol, 1e-3)
    report_grad(a3d, "attn_block d resid", dr.grad, cr.grad, gtol, 1e-3)
    sc = max(1.0, math.sqrt(B * max(Lq, S)) / 8)
    report_grad(a3d, "attn_block d in_w", mha.in_proj_weight.grad, ciw.grad, gtol * sc, 2e-3)
    report_grad(a3d, "attn_block d in_b", mha.in_proj_bias.grad, cib.grad, gtol * sc, 2e-3)
    report_grad(a3d, "attn_block d out_w", mha.out_proj.weight.grad, cow.grad, gtol * sc, 2e-3)
    report_grad(a3d, "attn_block d out_b", mha.out_proj.bias.grad, cob.grad, gtol * sc, 2e-3)
    report_grad(a3d, "attn_block d ln_g", norm.weight.grad, cg.grad, gtol * sc, 2e-3)
    report_grad(a3d, "attn_block d ln_b", norm.bias.grad, cb.grad, gtol * sc, 2e-3)
    # the gradient-free route through the same call site (need_bwd False -> nograd: the adaptive-P forward of attention16.hip,
    # the single-query forward for Lq = 1), same oracle, same tolerance
    with torch.no_grad():
        y_ng = O.attn_block(dq.detach(), dk.detach(), dv.detach(), dr.detach(), None if q_xyz is None else q_xyz.to(dev),
                            None if k_xyz is None else k_xyz.to(dev), None if kmask is None else kmask.to(dev), mha, norm, H)
    assert not y_ng.requires_grad
    report(f"attn_block[{mode}] fwd (no_grad)", y_ng, ref, 1e-4)


@pytest.mark.parametrize("B,S,rope", [(3, 200, False), (70, 130, True), (64, 4097, True)])
def test_query_stream_module_fused_layers_vs_oracle(a3d, dev, B, S, rope):
    """nn.RelativeCrossAttentionModule on ONE query per sample (Act3D's query stream, act3d.py:467-480): the fused per-layer
    launches of csrc/query_stream.hip (ops.QueryLayerFn) against oracle.rel_cross_attn_module -- both layers' outputs, the
    gradients of the query, the context and every parameter -- and against the op-by-op device path it replaces
    (SingleQueryAttnBlockFn + MLPFn; A3D_QS_FUSED=0).  B = 70 crosses the 64-row block of the single workgroup."""
    O = a3d.ops
    E, H, NL = 60, 4, 2
    g = torch.Generator().manual_seed(B + S)
    mod = a3d.nn.RelativeCrossAttentionModule(E, H, NL)
    with torch.no_grad():
        for n, p_ in mod.named_parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * (0.1 if p_.dim() == 1 else 1.4 / math.sqrt(p_.shape[-1])))
            if n.endswith("norm.weight"):
                p_.add_(1.0)
    P = {"m." + n: p_.detach().clone().requires_grad_() for n, p_ in mod.named_parameters()}
    q = torch.randn(B, 1, E, generator=g)
    ctx = torch.randn(B, S, E, generator=g)
    q_xyz = torch.rand(B, 1, 3, generator=g) * 2 - 0.5 if rope else None
    k_xyz = torch.rand(B, S, 3, generator=g) * 2 - 0.5 if rope else None
    cq, cc = q.clone().requires_grad_(), ctx.clone().requires_grad_()
    outs = OB.rel_cross_attn_module(P, "m", NL, cq, cc, H, q_xyz, k_xyz)
    dys = [torch.randn(B, 1, E, generator=g) for _ in range(NL)]
    sum((o * d).sum() for o, d in zip(outs, dys)).backward()

    def run(fused):
        old = O.QUERY_STREAM_FUSED
        O.QUERY_STREAM_FUSED = fused
        try:
            m = a3d.nn.RelativeCrossAttentionModule(E, H, NL).to(dev)
            m.load_state_dict(mod.state_dict())
            dq, dc = q.to(dev).requires_grad_(), ctx.to(dev).requires_grad_()
            got = m(dq, dc, None if q_xyz is None else q_xyz.to(dev), None if k_xyz is None else k_xyz.to(dev))
            sum((o * d.to(dev)).sum() for o, d in zip(got, dys)).backward()
            return m, dq, dc, got
        finally:
            O.QUERY_STREAM_FUSED = old

    m, dq, dc, got = run(True)
    m0, dq0, dc0, got0 = run(False)
    for i in range(NL):
        report(f"query stream layer {i} fwd", got[i], outs[i], 1e-4)
        report(f"query stream layer {i} fwd (fused vs op-by-op)", got[i], got0[i], 2e-5)
    gtol = 5e-4
    report_grad(a3d, "query stream d query", dq.grad, cq.grad, gtol, 1e-3)
    report_grad(a3d, "query stream d context", dc.grad, cc.grad, gtol, 1e-3)
    sc = max(1.0, math.sqrt(B * S) / 8)
    named0 = dict(m0.named_parameters())
    for n, p_ in m.named_parameters():
        report_grad(a3d, f"query stream d {n}", p_.grad, P["m." + n].grad, gtol * sc, 2e-3)
        report_grad(a3d, f"query stream d {n} (fused vs op-by-op)", p_.grad, named0[n].grad, 1e-4 * sc, 5e-4)


@pytest.mark.parametrize("B,Lq,S,E,H,rope,masked,mode", [(2, 37, 131, 60, 4, True, False, "kv"), (2, 16, 70, 120, 8, True, True, "qk"),
                                                          (1, 130, 4097, 60, 4, True, False, "kv")])
def test_attn_block_fwd_bwd_split_bf16_family(a3d, dev, B, Lq, S, E, H, rope, masked, mode):
    """The split-bf16 kernels (attention.hip / attention_bwd.hip, A3D_ATTN_MODE=bf16x3) stay covered: same check, the tight
    element-wise gradient bounds."""
    old = a3d.ops.ATTN_MODE
    a3d.ops.ATTN_MODE = "bf16x3"
    try:
        test_attn_block_fwd_bwd(a3d, dev, B, Lq, S, E, H, rope, masked, mode)
    finally:
        a3d.ops.ATTN_MODE = old


def test_attn_block_query_gradient_with_aliased_residual(a3d, dev):
    """The query / residual gradient fold is decided by OBJECT identity at the call site (`q_in is resid`), not by storage: a
    detached requires-grad leaf that shares the residual's storage is a different autograd tensor and keeps its own gradient
    (round-5 advisor finding: data_ptr equality routed it into the residual's graph and left q_in.grad None)."""
    O = a3d.ops
    B, Lq, S, E, H = 2, 19, 70, 60, 4
    g = torch.Generator().manual_seed(11)
    in_w, in_b, out_w, out_b = _mha_params(E, g, scale=1.0)
    mha, norm = _mk_modules(dev, in_w, in_b, out_w, out_b, torch.ones(E), torch.zeros(E))
    x = torch.randn(B, Lq, E, generator=g).to(dev)
    ctxt = torch.randn(B, S, E, generator=g).to(dev)
    dy = torch.randn(B, Lq, E, generator=g).to(dev)
    # (a) the same object: one gradient, the sum of both roles
    xa = x.clone().requires_grad_()
    O.attn_block(xa, ctxt, ctxt, xa, None, None, None, mha, norm, H).backward(dy)
    # (b) separate tensors: the two roles' gradients
    xq, xr = x.clone().requires_grad_(), x.clone().requires_grad_()
    O.attn_block(xq, ctxt, ctxt, xr, None, None, None, mha, norm, H).backward(dy)
    # (c) an alias: same storage, distinct autograd leaves
    base = x.clone()
    aq, ar = base.detach().requires_grad_(), base.detach().requires_grad_()
    assert aq.data_ptr() == ar.data_ptr() and aq is not ar
    O.attn_block(aq, ctxt, ctxt, ar, None, None, None, mha, norm, H).backward(dy)
    assert aq.grad is not None and ar.grad is not None
    report("aliased query gradient", aq.grad, xq.grad.cpu(), 1e-4, 1e-5)
    report("aliased residual gradient", ar.grad, xr.grad.cpu(), 1e-4, 1e-5)
    report("folded gradient = sum of the roles", xa.grad, (xq.grad + xr.grad).cpu(), 1e-4, 1e-5)


@pytest.mark.parametrize("B,Lq,S,E,H,masked,mode", [(2, 37, 131, 60, 4, False, "kv"), (1, 333, 4097, 60, 4, False, "kv"),
                                                      (2, 16, 70, 120, 8, True, "qk"), (2, 50, 1026, 120, 8, True, "kv")])
def test_rows_only_operand_set_equals_rows_plus_planes_bit_for_bit(a3d, dev, B, Lq, S, E, H, masked, mode):
    """Round 6: the projection kernels write ONE layout of q, k, v (rows16; value rows with the ones channel) and the kernels form
    V^T (forward) and K^T (dQ) with transposed LDS reads of the rows tiles.  Same fragments, same MFMA order: the block's output and
    every gradient must equal the rows + planes operand set (A3D_ATTN_ROWS_ONLY=0, the round-5 data flow) BIT FOR BIT."""
    O = a3d.ops
    g = torch.Generator().manual_seed(S + Lq)
    in_w, in_b, out_w, out_b = _mha_params(E, g, scale=2.0)
    if mode == "qk":
        S = Lq
    x = torch.randn(B, Lq, E, generator=g)
    c = x if mode == "qk" else torch.randn(B, S, E, generator=g)
    v = c if mode == "kv" else torch.randn(B, S, E, generator=g)
    q_xyz = torch.rand(B, Lq, 3, generator=g) * 2 - 0.5
    k_xyz = q_xyz if mode == "qk" else torch.rand(B, S, 3, generator=g) * 2 - 0.5
    kmask = None
    if masked:
        kmask = torch.zeros(B, S, dtype=torch.bool)
        kmask[:, -(S // 4):] = True
        kmask = kmask.to(dev)
    dy = torch.randn(B, Lq, E, generator=g).to(dev)

    def run(rows_only):
        keep = O.ROWS_ONLY
        O.ROWS_ONLY = rows_only
        try:
            mha, norm = _mk_modules(dev, in_w, in_b, out_w, out_b, torch.ones(E), torch.zeros(E))
            xq = x.to(dev).requires_grad_()
            xk = xq if mode == "qk" else c.to(dev).requires_grad_()
            xv = xk if mode == "kv" else v.to(dev).requires_grad_()
            r = torch.zeros(B, Lq, E, device=dev, requires_grad=True)
            y = O.attn_block(xq, xk, xv, r, q_xyz.to(dev), k_xyz.to(dev), kmask, mha, norm, H)
            y.backward(dy)
            return [y.detach(), xq.grad, xk.grad, xv.grad, mha.in_proj_weight.grad, mha.in_proj_bias.grad]
        finally:
            O.ROWS_ONLY = keep

    a, b = run(True), run(False)
    names = ["y", "d q_in", "d k_in", "d v_in", "d in_proj_weight", "d in_proj_bias"]
    for n, ta, tb in zip(names, a, b):
        same = torch.equal(ta, tb)
        print(f"[parity] rows-only vs rows + planes, {n}: {'bit-identical' if same else 'max diff %.3e' % (ta - tb).abs().max().item()}")
        if n in ("y", "d q_in", "d k_in", "d v_in"):
            assert same, n
        else:                                   # float-atomic weight gradients: accumulation order varies from run to run
            assert (ta - tb).abs().max().item() <= 1e-5 * max(1.0, tb.abs().max().item()), n


def test_attn_softmax_rescale_spike(a3d, dev):
    """Online-softmax rescale path: one key with a huge score in a late chunk (cdna guide rule 26)."""
    O = a3d.ops
    B, Lq, S, E, H = 1, 20, 300, 60, 4
    g = torch.Generator().manual_seed(5)
    in_w = torch.zeros(3 * E, E)
    in_w[:E] = torch.eye(E)
    in_w[E:2 * E] = torch.eye(E)
    in_w[2 * E:] = torch.eye(E)
    in_b = torch.zeros(3 * E)
    out_w, out_b = torch.eye(E), torch.zeros(E)
    xq = torch.randn(B, Lq, E, generator=g)
    xk = torch.randn(B, S, E, generator=g)
    xk[0, 250] = xq[0, 3] * 6.0       # spike for query 3 in the 4th key chunk
    xk[0, 10] = xq[0, 7] * 5.0
    ref = OB.layer_norm(xq + OB.mha(xq, xk, xk, in_w, in_b, out_w, out_b, H), torch.ones(E), torch.zeros(E))
    mha, norm = _mk_modules(dev, in_w, in_b, out_w, out_b, torch.ones(E), torch.zeros(E))
    kd = xk.to(dev)
    y = O.attn_block(xq.to(dev), kd, kd, xq.to(dev), None, None, None, mha, norm, H)
    report("attn spike", y, ref, 1e-3)


@pytest.mark.parametrize("shape,hidden,out,ln", [((4, 33, 60), 60, 60, True), ((2, 16, 120), 480, 120, True),
                                                 ((7, 60), 60, 5, False), ((3, 16, 9), 120, 120, False)])
def test_mlp_block(a3d, dev, shape, hidden, out, ln):
    O = a3d.ops
    g = torch.Generator().manual_seed(hidden + out)
    K = shape[-1]
    x = torch.randn(*shape, generator=g)
    ws = [torch.randn(hidden, K, generator=g) / math.sqrt(K), torch.randn(hidden, generator=g) * 0.1,
          torch.randn(out, hidden, generator=g) / math.sqrt(hidden), torch.randn(out, generator=g) * 0.1]
    lg, lb = torch.rand(out, generator=g) + 0.5, torch.randn(out, generator=g) * 0.1
    cl = [t.clone().requires_grad_() for t in [x] + ws + [lg, lb]]
    o = F.linear(F.relu(F.linear(cl[0], cl[1], cl[2])), cl[3], cl[4])
    ref = F.layer_norm(cl[0] + o, (out,), cl[5], cl[6], 1e-5) if ln else o
    dy = torch.randn(*ref.shape, generator=g)
    ref.backward(dy)
    P = [torch.nn.Parameter(t.to(dev)) for t in ws + [lg, lb]]
    xd = x.to(dev).requires_grad_()
    y = O.MLPFn.apply(xd, P[0], P[1], P[2], P[3], P[4] if ln else None, P[5] if ln else None)
    report("mlp fwd", y, ref, 5e-5, 1e-5)
    y.backward(dy.to(dev))
    report("mlp dx", xd.grad, cl[0].grad, 2e-4, 1e-4)
    for i, nm in enumerate(["w1", "b1", "w2", "b2"]):
        report("mlp d" + nm, P[i].grad, cl[1 + i].grad, 5e-4, 1e-4)
    if ln:
        report("mlp dln_g", P[4].grad, cl[5].grad, 5e-4, 1e-4)


@pytest.mark.parametrize("f,H", [(2, 256), (8, 256), (4, 128), (2, 128)])
def test_pcd_downsample_bit_exact(a3d, dev, f, H):
    g = torch.Generator().manual_seed(f)
    pcd = torch.rand(2, 3, 3, H, H, generator=g) * 2 - 1
    ref = F.interpolate(pcd.view(6, 3, H, H), scale_factor=1.0 / f, mode="bilinear")
    h = H // f
    ref = ref.view(2, 3, 3, h, h).permute(0, 1, 3, 4, 2).reshape(2, 3 * h * h, 3)
    got = a3d.ops.pcd_downsample(pcd.to(dev), f).cpu()
    assert torch.equal(got, ref), f"pcd_downsample f={f}: max diff {(got - ref).abs().max().item():.3e}"


@pytest.mark.parametrize("B,N,k", [(3, 16384, 1024), (2, 65536, 4096), (2, 49152, 3072), (1, 500, 500), (2, 1000, 7), (1, 40000, 9000),
                                   (1, 40000, 16384)])
def test_knn_topk_indices_exact(a3d, dev, B, N, k):
    """Bit-exact against the oracle (IEEE fp32 distances, (distance, index) order).  Against torch.topk on CPU the
    index sequence must agree wherever neighbouring distances are not within 2 ulp: torch's CPU sqrt (MKL VML) is not
    correctly rounded, so exact ties / near-ties may legitimately come out in a different order."""
    from oracle import sampling as OS
    g = torch.Generator().manual_seed(N + k)
    xyz = torch.rand(B, N, 3, generator=g)
    pos = torch.rand(B, 3, generator=g)
    idx, dist = a3d.ops.knn_topk(pos.to(dev), xyz.to(dev), k, return_dist=True)
    idx, dist = idx.cpu(), dist.cpu()
    o_idx, o_dist = OS.knn_topk(pos.numpy(), xyz.numpy(), k)
    assert np.array_equal(dist.numpy(), o_dist), "top-k distances differ from the oracle"
    assert np.array_equal(idx.numpy(), o_idx), "top-k indices differ from the oracle"
    d = ((pos[:, None] - xyz) ** 2).sum(-1).sqrt()
    tv = d.topk(k, dim=-1, largest=False)
    assert (dist - tv.values).abs().max().item() <= 2e-7, "top-k distances differ from torch.topk by more than 2 ulp"
    gap = 3e-7
    strict = torch.ones_like(dist, dtype=torch.bool)
    strict[:, 1:] &= (tv.values[:, 1:] - tv.values[:, :-1]) > gap
    strict[:, :-1] &= (tv.values[:, 1:] - tv.values[:, :-1]) > gap
    assert torch.equal(idx[strict], tv.indices[strict]), "indices differ from torch.topk where distances are separated"
    assert strict.float().mean().item() > 0.9
    for b in range(B):
        assert set(idx[b, :-2].tolist()) <= set(tv.indices[b].tolist()) | set(idx[b, -4:].tolist())


def test_knn_topk_dense_shell_overflows_the_candidate_list(a3d, dev):
    """30 000 points within 1e-4 of distance 1 share ONE bin of the coarse histogram (bin width 2^-3 there): the k-th bin's
    candidate list cannot hold them in LDS and the selection runs its radix passes over the stored distances instead; k = 5000
    also takes the sort through two 4096-key register groups + the LDS merge.  Bit-exact against the oracle, as everywhere."""
    from oracle import sampling as OS
    g = torch.Generator().manual_seed(11)
    N, k = 30000, 5000
    d = torch.randn(2, N, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True) * (1.0 + 1e-4 * torch.rand(2, N, 1, generator=g))
    d[:, :100] *= 0.5                                   # a few points in lower bins ("definitely in")
    d[1, 5000:5200] = d[1, 4999]                        # exact ties around the threshold region
    pos = torch.zeros(2, 3)
    idx, dist = a3d.ops.knn_topk(pos.to(dev), d.to(dev), k, return_dist=True)
    o_idx, o_dist = OS.knn_topk(pos.numpy(), d.numpy(), k)
    assert np.array_equal(dist.cpu().numpy(), o_dist) and np.array_equal(idx.cpu().numpy(), o_idx)


def test_knn_topk_ties(a3d, dev):
    xyz = torch.zeros(1, 300, 3)
    xyz[0, 100:] = 1.0
    idx = a3d.ops.knn_topk(torch.zeros(1, 3).to(dev), xyz.to(dev), 150).cpu()
    assert idx[0].tolist() == list(range(100)) + list(range(100, 150))


def test_build_context_and_grad(a3d, dev):
    O = a3d.ops
    g = torch.Generator().manual_seed(3)
    B, Npts, E, k, X = 2, 500, 60, 64, 1
    feat = torch.randn(B, Npts, E, generator=g)
    extra = torch.randn(B, X, E, generator=g)
    idx = torch.stack([torch.randperm(Npts, generator=g)[:k] for _ in range(B)])
    fd, ed = feat.to(dev).requires_grad_(), extra.to(dev).requires_grad_()
    ctx = O.BuildContextFn.apply(fd, idx.to(dev), ed)
    ref = torch.cat([torch.stack([f[i] for f, i in zip(feat, idx)]), extra], 1)
    assert torch.equal(ctx.cpu(), ref)
    dy = torch.randn(B, k + X, E, generator=g)
    ctx.backward(dy.to(dev))
    rf = torch.zeros_like(feat)
    for b in range(B):
        rf[b, idx[b]] = dy[b, :k]
    assert torch.equal(fd.grad.cpu(), rf) and torch.equal(ed.grad.cpu(), dy[:, k:])
    ctx0 = O.BuildContextFn.apply(fd, None, ed)
    assert torch.equal(ctx0.cpu(), torch.cat([feat, extra], 1))
    x3 = O.gather_rows(torch.arange(B * Npts * 3, dtype=torch.float32).view(B, Npts, 3).to(dev), idx.to(dev),
                       torch.ones(B, 1, 3).to(dev)).cpu()
    assert x3.shape == (B, k + 1, 3) and x3[1, 5, 0].item() == (Npts + idx[1, 5].item()) * 3


def test_heads_and_losses(a3d, dev):
    O = a3d.ops
    g = torch.Generator().manual_seed(11)
    B, Ng, E = 5, 333, 60
    q = torch.randn(B, E, generator=g, requires_grad=True)
    Fm = torch.randn(B, Ng, E, generator=g, requires_grad=True)
    ref = torch.einsum("bc,bnc->bn", q, Fm)
    dl = torch.randn(B, Ng, generator=g)
    ref.backward(dl)
    qd, fd = q.detach().to(dev).requires_grad_(), Fm.detach().to(dev).requires_grad_()
    lg = O.MaskLogitsFn.apply(qd, fd)
    report("mask_logits", lg, ref, 2e-5, 1e-5)
    lg.backward(dl.to(dev))
    report("mask_logits dq", qd.grad, q.grad, 2e-4, 1e-5)
    report("mask_logits dF", fd.grad, Fm.grad, 1e-5, 1e-5)
    ghost = torch.rand(B, Ng, 3, generator=g)
    logits = ref.detach().clone()
    logits[2, 50] = logits[2].max() + 1
    logits[2, 20] = logits[2, 50]          # tie -> first index wins
    top, pos = O.argmax_gather(logits.to(dev), ghost.to(dev))
    assert torch.equal(top.cpu(), logits.max(-1).indices) and top[2].item() == 20
    assert torch.equal(pos.cpu(), ghost[torch.arange(B), top.cpu()])
    # soft CE (main_keypose.py:382-405)
    gt = torch.rand(B, 3, generator=g)
    z = (ref.detach() * 0.3).requires_grad_()
    l2 = ((ghost.permute(0, 2, 1) - gt.unsqueeze(-1)) ** 2).sum(1).sqrt()
    label = torch.softmax(-l2 / 0.01, dim=-1)
    rl = F.cross_entropy(z, label).mean() * 1.0 / 3
    rl.backward()
    zd = z.detach().to(dev).requires_grad_()
    ls = O.SoftCEFn.apply(zd, ghost.to(dev), gt.to(dev), 0.01, 0.0, 1.0 / 3)
    report("soft_ce loss", ls, rl, 1e-5, 1e-5)
    (ls * 2.0).backward()
    report("soft_ce dlogits", zd.grad, 2 * z.grad, 1e-6, 1e-4)
    # mse / l1
    p = torch.randn(B, 4, generator=g, requires_grad=True)
    t = torch.randn(B, 4, generator=g)
    for kind, fn in ((0, F.mse_loss), (1, F.l1_loss)):
        p.grad = None
        r = fn(p, t) * 10
        r.backward()
        pd = p.detach().to(dev).requires_grad_()
        l = O.ElemLossFn.apply(pd, t.to(dev), kind, 10.0)
        report(f"elem_loss{kind}", l, r, 1e-5, 1e-5)
        l.backward()
        report(f"elem_loss{kind} grad", pd.grad, p.grad, 1e-6, 1e-5)
    # quat + sigmoid
    pr = torch.randn(B, 5, generator=g, requires_grad=True)
    rot = pr[:, :4] / torch.clamp(pr[:, :4].square().sum(-1).sqrt().unsqueeze(-1), min=1e-10)
    gr = torch.sigmoid(pr[:, 4:])
    dr, dg = torch.randn(B, 4, generator=g), torch.randn(B, 1, generator=g)
    (rot * dr).sum().backward(retain_graph=True)
    (gr * dg).sum().backward()
    prd = pr.detach().to(dev).requires_grad_()
    rd, gd = O.QuatSigmoidFn.apply(prd)
    report("quat", rd, rot, 1e-6)
    report("sigmoid", gd, gr, 1e-6)
    ((rd * dr.to(dev)).sum() + (gd * dg.to(dev)).sum()).backward()
    report("quat_sigmoid grad", prd.grad, pr.grad, 1e-5, 1e-5)


def test_adamw_matches_torch(a3d, dev):
    """a3d_adamw_step against torch.optim.AdamW with the reference's two groups (engine.py:89-102), PER-PARAMETER skipping:
    a matrix with an all-zero gradient row from step 1 on (a dead ReLU unit) is decayed like torch decays it; a tensor whose
    .grad stays None is left alone; a tensor that joins at step 3 gets the bias correction of its own step count."""
    L = a3d.lib
    g = torch.Generator().manual_seed(2)
    shapes = [(37,), (40, 25), (64,), (48,)]            # bias (no decay) | weight with a dead row | never used | joins late
    ps = [torch.nn.Parameter(torch.randn(sh, generator=g)) for sh in shapes]
    opt = torch.optim.AdamW([{"params": ps[:1], "weight_decay": 0.0}, {"params": ps[1:], "weight_decay": 5e-4}], lr=1e-4)
    sizes = [p.numel() for p in ps]
    off = [0]
    for k in sizes:
        off.append(off[-1] + k)
    n = off[-1]
    pd = torch.cat([p.detach().reshape(-1) for p in ps]).to(dev)
    p0 = pd.clone()
    m, v = torch.zeros_like(pd), torch.zeros_like(pd)
    step = torch.zeros(1, device=dev)
    seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
    seg_state = torch.zeros((len(ps), 4), device=dev)
    for it in range(5):
        gr = [torch.randn(sh, generator=g) for sh in shapes]
        gr[1][7] = 0.0                                   # dead row: exactly zero gradient at every step
        ps[0].grad, ps[1].grad = gr[0].clone(), gr[1].clone()
        ps[2].grad = None
        ps[3].grad = gr[3].clone() if it >= 2 else None
        opt.step()
        gd = torch.cat([gr[0].reshape(-1), gr[1].reshape(-1), torch.zeros(sizes[2]),
                        gr[3].reshape(-1) if it >= 2 else torch.zeros(sizes[3])]).to(dev)
        L.call("a3d_adamw_step", pd.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), seg_off.data_ptr(),
               seg_state.data_ptr(), len(ps), n, sizes[0], 1e-4, 0.9, 0.999, 1e-8, 0.0, 5e-4, 1.0, L.stream())
    ref = torch.cat([p.detach().reshape(-1) for p in ps])
    report("adamw", pd, ref, 1e-6, 1e-6)
    assert step.item() == 5.0
    assert seg_state[:, 0].cpu().tolist() == [5.0, 5.0, 0.0, 3.0], "per-parameter step counts (torch's state[p]['step'])"
    assert [float(opt.state[p]["step"]) if p in opt.state else 0.0 for p in ps] == [5.0, 5.0, 0.0, 3.0]
    assert torch.equal(pd[off[2]:off[3]], p0[off[2]:off[3]]), "unused parameters must not decay"
    dead = slice(off[1] + 7 * 25, off[1] + 8 * 25)
    assert not torch.equal(pd[dead], p0[dead]), "a zero-gradient row of a trained matrix is decayed, as torch does"
    report("adamw dead row", pd[dead], ref[dead], 1e-7, 1e-6)


def test_sampler_matches_cpu_twin(a3d, dev):
    from oracle import sampling as OS
    O = a3d.ops
    bounds = torch.tensor([[-0.11, -0.55, 0.71], [0.64, 0.51, 1.51]])
    state = torch.tensor([1234567, 3], dtype=torch.int64, device=dev)
    got = O.sample_ghost_points(state, bounds.to(dev), None, 0.0, 4, 333, 0).cpu().numpy()
    ref = OS.philox_ghost_points(1234567, 3, bounds.numpy(), None, 0.0, 4, 333, 0)
    assert np.array_equal(got, ref), "device Philox cube sampler differs from its CPU twin"
    anchor = torch.tensor([[0.3, 0.1, 0.9], [0.63, 0.5, 1.5], [-0.1, -0.5, 0.72], [0.2, 0.0, 1.0]])
    got = O.sample_ghost_points(state, bounds.to(dev), anchor.to(dev), 0.08, 4, 333, 1).cpu().numpy()
    ref = OS.philox_ghost_points(1234567, 3, bounds.numpy(), anchor.numpy(), 0.08, 4, 333, 1)
    assert np.array_equal(got, ref), "device Philox ball sampler differs from its CPU twin"
    d = np.linalg.norm(got - anchor.numpy()[:, None], axis=-1)
    assert (d < 0.08 + 1e-6).all()
    assert (got >= bounds.numpy()[0] - 1e-6).all() and (got <= bounds.numpy()[1] + 1e-6).all()
    # anchor far outside the workspace: the reference loops forever; we terminate with the clipped anchor
    far = O.sample_ghost_points(state, bounds.to(dev), torch.tensor([[5.0, 5.0, 5.0]]).to(dev), 0.02, 1, 8, 2).cpu()
    assert torch.allclose(far, bounds[1].expand(1, 8, 3))


def test_diffusion_elementwise(a3d, dev):
    O, L = a3d.ops, a3d.lib
    from oracle import diffusion as OD
    g = torch.Generator().manual_seed(4)
    B, Ln, E = 3, 16, 120
    x = torch.randn(B, Ln, E, generator=g, requires_grad=True)
    mod = torch.randn(B, 2 * E, generator=g, requires_grad=True)
    sc, sh = mod.chunk(2, -1)
    ref = x * (1 + sc.unsqueeze(1)) + sh.unsqueeze(1)
    dy = torch.randn(B, Ln, E, generator=g)
    ref.backward(dy)
    xd, md = x.detach().to(dev).requires_grad_(), mod.detach().to(dev).requires_grad_()
    y = O.AdaLNFn.apply(xd, md)
    report("adaln", y, ref, 1e-6)
    y.backward(dy.to(dev))
    report("adaln dx", xd.grad, x.grad, 1e-6)
    report("adaln dmod", md.grad, mod.grad, 2e-5)
    t = torch.tensor([0.0, 3.0, 57.0, 99.0])
    report("sinusoidal", O.sinusoidal_emb(t.to(dev), E), OB.sinusoidal(t, E), 2e-5)
    s = torch.randn(50, generator=g, requires_grad=True)
    r = F.silu(s)
    r.backward(torch.ones(50))
    sd = s.detach().to(dev).requires_grad_()
    ys = O.SiLUFn.apply(sd)
    ys.backward(torch.ones(50, device=dev))
    report("silu", ys, r, 1e-6)
    report("silu grad", sd.grad, s.grad, 1e-6)
    # DDPM tables / add_noise / step against the oracle restatement
    sched = OD.DDPMSchedules(100)
    x0 = torch.randn(B, Ln, 9, generator=g)
    eps = torch.randn(B, Ln, 9, generator=g)
    tt = torch.tensor([0, 57, 99])
    ref_noisy = sched.add_noise(x0, eps, tt)
    out = torch.empty(B, Ln, 9, device=dev)
    x0d, epsd, ttd, apd, ard = x0.to(dev), eps.to(dev), tt.to(dev), sched.acp_pos.to(dev), sched.acp_rot.to(dev)
    L.call("a3d_ddpm_add_noise", x0d.data_ptr(), epsd.data_ptr(), ttd.data_ptr(), apd.data_ptr(), ard.data_ptr(),
           out.data_ptr(), B, Ln, 9, 3, L.stream())
    report("ddpm add_noise", out, ref_noisy, 1e-6)
    cond = torch.randn(B, Ln, 9, generator=g)
    cmask = torch.zeros(B, Ln, 9, dtype=torch.bool)
    cmask[:, 0] = True
    cmask[1, -3:] = True
    mo = torch.randn(B, Ln, 9, generator=g) * 1.5
    cp, cr = sched.coef_pos.to(dev), sched.coef_rot.to(dev)
    mod_, condd, cmd = mo.to(dev), cond.to(dev), cmask.to(dev).to(torch.uint8).contiguous()
    for tstep in (99, 40, 1, 0):
        ref_prev = sched.step_with_inpaint(mo, x0, eps, cond, cmask, tstep)
        L.call("a3d_ddpm_step", mod_.data_ptr(), x0d.data_ptr(), epsd.data_ptr(), condd.data_ptr(), cmd.data_ptr(),
               cp.data_ptr(), cr.data_ptr(), out.data_ptr(), B * Ln, 9, 3, tstep, L.stream())
        report(f"ddpm step t={tstep}", out, ref_prev, 2e-6, 1e-6)


@pytest.mark.parametrize("N,C,H", [(4, 32, 16), (3, 64, 24), (2, 256, 8), (2, 2048, 4), (7, 64, 40), (3, 512, 12), (5, 1024, 6)])
def test_fused_batchnorm_train_relu_residual(a3d, dev, N, C, H):
    """vision.hip BN (batch statistics + running-stat update) + residual + ReLU vs torch's fp32 batch_norm."""
    g = torch.Generator().manual_seed(C + N)
    x = (torch.randn(N, C, H, H, generator=g) * 1.7 + 0.3).to(torch.bfloat16)
    res = torch.randn(N, C, H, H, generator=g).to(torch.bfloat16)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.2)
    ref_bn = torch.nn.BatchNorm2d(C)
    ref_bn.load_state_dict(bn.state_dict())
    ref = torch.relu(ref_bn(x.float()) + res.float())
    bnd = bn.to(dev).train()
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    rd = res.to(dev).contiguous(memory_format=torch.channels_last)
    y = a3d.nn.bn_act(xd, bnd, relu=True, residual=rd)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    report("bn_act train", y.float(), ref, 2e-2, 8e-3)          # bf16 output rounding
    report("bn running_mean", bnd.running_mean, ref_bn.running_mean, 1e-5, 1e-4)
    report("bn running_var", bnd.running_var, ref_bn.running_var, 1e-5, 1e-4)
    bnd.eval(); ref_bn.eval()
    y2 = a3d.nn.bn_act(xd, bnd, relu=False)
    report("bn_act eval", y2.float(), ref_bn(x.float()), 2e-2, 8e-3)
    # fused AvgPool2d(2): the pooled output is the mean of the bf16 activations the un-pooled kernel writes
    yf, yp = a3d.nn.bn_act(xd, bnd, relu=True, residual=rd, pool=True)
    assert torch.equal(yf, a3d.nn.bn_act(xd, bnd, relu=True, residual=rd))
    assert yp.is_contiguous(memory_format=torch.channels_last)
    report("bn_act pooled", yp.float(), F.avg_pool2d(yf.float(), 2), 1e-6, 8e-3)     # one bf16 rounding
    _, yp2 = a3d.nn.bn_act(xd, bnd, relu=True, residual=rd, pool=True, keep_full=False)
    assert torch.equal(yp2, yp)
    report("plain pool2", a3d.nn.bn_act(xd, None, relu=False, pool=True, keep_full=False)[1].float(),
           F.avg_pool2d(x.float(), 2), 1e-6, 8e-3)
    # the residual as a raw convolution output with its own BatchNorm (the downsample branch folded into the final apply):
    # relu(bn(x) + bn_r(res)) without materialising bn_r(res)
    bn_r = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn_r.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn_r.bias.copy_(torch.randn(C, generator=g) * 0.2)
    ref_r = torch.nn.BatchNorm2d(C)
    ref_r.load_state_dict(bn_r.state_dict())
    bnd.train(); ref_bn.train()
    ref2 = torch.relu(ref_bn(x.float()) + ref_r(res.float()))
    bn_rd = bn_r.to(dev).train()
    y3 = a3d.nn.bn_act(xd, bnd, relu=True, residual=rd, residual_scale=a3d.nn.bn_scale_shift(rd, bn_rd))
    report("bn_act with a normalised residual", y3.float(), ref2, 2e-2, 8e-3)
    report("residual bn running_var", bn_rd.running_var, ref_r.running_var, 1e-5, 1e-4)


def test_fused_frozen_backbone_matches_module(a3d, dev):
    """Whole frozen backbone (train-mode BN): the fused-BN bf16 runner must be as close to the fp32 module as the plain
    torch bf16 path (bf16 convs + torch BatchNorm) is -- both are bf16 activations through ~50 layers."""
    import copy
    torch.manual_seed(0)
    bb32 = a3d.nn.SyntheticCLIPResNet50().to(dev).train()
    bb, bb2 = copy.deepcopy(bb32), copy.deepcopy(bb32)
    x = torch.rand(4, 3, 128, 128, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = bb32(x)
        a3d.nn.FUSED_BN = False
        plain = a3d.nn.run_frozen_backbone(bb2, x, torch.bfloat16)
        a3d.nn.FUSED_BN = True
        got = a3d.nn.run_frozen_backbone(bb, x, torch.bfloat16)
    rms = lambda t: t.float().pow(2).mean().sqrt().item()
    for k in ref:
        e_f, e_p, sc = rms(got[k] - ref[k]), rms(plain[k] - ref[k]), rms(ref[k])
        print(f"[parity] backbone {k}: rms_err fused={e_f:.3e} torch_bf16={e_p:.3e} ref_rms={sc:.3e}")
        assert got[k].shape == ref[k].shape and e_f <= 1.25 * e_p + 1e-3 * sc, k
    report("backbone bn1.running_mean", bb.bn1.running_mean, bb32.bn1.running_mean, 1e-4, 1e-2)
    report("backbone layer4 running_var", bb.layer4[2].bn3.running_var, bb32.layer4[2].bn3.running_var, 1e-3, 5e-2)
    assert int(bb.layer3[0].bn2.num_batches_tracked) == 1


def test_fpn_top_down_fused(a3d, dev):
    """lat + nearest_up2(top), bf16 NHWC, C = 60: forward bit-exact vs torch, backward = 2x2 block sums (one bf16 rounding)."""
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(3, 60, 16, 24, generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
    top = torch.randn(3, 60, 8, 12, generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
    l1, t1 = lat.clone().requires_grad_(), top.clone().requires_grad_()
    l2, t2 = lat.clone().requires_grad_(), top.clone().requires_grad_()
    y = a3d.nn.fpn_top_down(l1, t1)
    ref = l2 + F.interpolate(t2, size=l2.shape[-2:], mode="nearest")
    assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y, ref)
    dy = torch.randn(3, 60, 16, 24, generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
    y.backward(dy)
    ref.backward(dy)
    assert torch.equal(l1.grad, l2.grad)
    report("fpn top-down dtop", t1.grad.float(), t2.grad.float(), 1e-6, 8e-3)
    # shapes the fused kernel does not cover fall back to torch
    odd = torch.randn(1, 60, 5, 7, generator=g).to(torch.bfloat16).to(dev)
    assert a3d.nn.fpn_top_down(odd, top[:1, :, :3, :4].contiguous()).shape == odd.shape


@pytest.mark.parametrize("images,H,W,K,N,nbias,with_top", [(3, 16, 32, 64, 64, 60, True), (2, 8, 8, 256, 64, 64, True),
                                                          (1, 6, 10, 128, 128, 120, True), (5, 7, 9, 64, 64, 0, False),
                                                          (2, 64, 64, 256, 128, 128, True)])
def test_fpn_lateral_convolution_with_top_down_epilogue(a3d, dev, images, H, W, K, N, nbias, with_top):
    """a3d_conv1x1_topdown_fwd: y = bf16(x w^T + bias + up2(top)) with ONE rounding of the fp32 sum, against torch in fp32 on the same
    bf16 operands (tile tails: rows not a multiple of the 64 / 128 / 256-row tile; pad channels without bias; the pyramid's top level
    without a top map), and nn._LateralTopDownFn's backward against the unfused path's autograd (library convolution + top-down kernel)."""
    g = torch.Generator().manual_seed(images * 1000 + K + N)
    cl = torch.channels_last
    x = torch.randn(images, K, H, W, generator=g).to(dev).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(N, K, 1, 1, generator=g) * K ** -0.5).to(dev)
    bias = (torch.randn(nbias, generator=g).to(dev) if nbias else None)
    top = torch.randn(images, N, H // 2, W // 2, generator=g).to(dev).to(torch.bfloat16).contiguous(memory_format=cl) if with_top else None
    w16 = w.to(torch.bfloat16)
    ref = F.conv2d(x.float(), w16.float())
    if bias is not None:
        ref = ref + F.pad(bias, (0, N - nbias)).view(1, N, 1, 1)
    if top is not None:
        ref = ref + F.interpolate(top.float(), size=(H, W), mode="nearest")
    y = torch.full((images, N, H, W), float("nan"), device=dev, dtype=torch.bfloat16).contiguous(memory_format=cl)
    L = a3d.lib
    assert L.load().a3d_conv1x1_topdown_serves(K, N) == 1
    L.call("a3d_conv1x1_topdown_fwd", x.data_ptr(), w16.reshape(N, K).contiguous().data_ptr(), None if bias is None else bias.data_ptr(),
           nbias, None if top is None else top.data_ptr(), y.data_ptr(), images, H, W, K, N, L.stream())
    torch.cuda.synchronize()
    # one bf16 rounding of an fp32 sum whose accumulation order differs from torch's: half an ulp (2^-9 relative) plus summation noise
    report(f"fpn lateral + top-down K={K} N={N}", y, ref, 1e-3, 2.0 ** -8)
    if not with_top or (H % 2) or (W % 2):
        return
    # autograd: fused Function vs library convolution + top-down kernel
    res = {}
    for tag in ("fused", "unfused"):
        wp = w.clone().requires_grad_()
        bp = bias.clone().requires_grad_() if bias is not None else None
        tp = top.clone().requires_grad_()
        if tag == "fused":
            out = a3d.nn._LateralTopDownFn.apply(x, wp, bp, tp)
        else:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = a3d.nn.fpn_top_down(F.conv2d(x, wp), tp, bp)
        dy = torch.randn(images, N, H, W, generator=torch.Generator().manual_seed(7)).to(dev).to(torch.bfloat16).contiguous(memory_format=cl)
        out.backward(dy)
        res[tag] = (out.detach(), wp.grad, None if bp is None else bp.grad, tp.grad)
    # one rounding against two: the unfused path rounds the lateral map before the add, an ulp of the LARGER of |lateral|, |sum|
    report(f"fused vs unfused lateral map K={K} N={N}", res["fused"][0], res["unfused"][0], 2.0 ** -7 * res["unfused"][0].abs().max().item())
    report_scaled(f"fused lateral weight gradient K={K} N={N}", res["fused"][1], res["unfused"][1], 1e-2)        # the same library kernel on the same dy (its bf16 result: an ulp where its atomics reorder)
    if bias is not None:
        report_scaled(f"fused lateral bias gradient K={K} N={N}", res["fused"][2], res["unfused"][2], 1e-5)
    assert torch.equal(res["fused"][3], res["unfused"][3])


def test_fpn_with_folded_biases_matches_plain_convolutions(a3d, dev):
    """nn.FeaturePyramidNetwork on bf16 channels-last maps: the lateral convolutions run bias-free with their bias added by the
    top-down kernel (forward) and reduced by it (backward), and the output convolutions' bias is deferred to the token
    gather (ops.BuildContextFn bias, a3d_colsum_rows).  Against the same module evaluated the plain way (F.conv2d with bias,
    torch add + nearest interpolate, torch gather): outputs within bf16 rounding, every weight / bias gradient within
    bf16-accumulation noise of its scale."""
    import copy
    torch.manual_seed(3)
    E, Cin, N = 60, [64, 256, 512, 1024, 2048], 3
    fpn = a3d.nn.FeaturePyramidNetwork(Cin, E).to(dev)
    with torch.no_grad():
        for m in fpn.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.bias.copy_(torch.randn_like(m.bias) * 0.3)
    ref = copy.deepcopy(fpn)
    g = torch.Generator().manual_seed(4)
    sizes = [32, 16, 8, 4, 2]
    feats = {f"res{i + 1}": (torch.randn(N, c, s_, s_, generator=g) * 0.5).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
             for i, (c, s_) in enumerate(zip(Cin, sizes))}
    needed = ["res1", "res3"]
    k = 37
    idx = torch.stack([torch.randperm(32 * 32, generator=g)[:k] for _ in range(N)]).to(dev)
    extra = torch.randn(N, 1, E, generator=g).to(dev)
    wts = {n: torch.randn(N, (k if n == "res1" else 64) + 1, E, generator=g).to(dev) for n in needed}

    def tokens(fm):
        n_, C_, h, w = fm.shape
        return fm.permute(0, 2, 3, 1).reshape(N, h * w, C_)

    # product path
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pyr, ob = fpn(feats, needed=needed, pad_to=64, defer_output_bias=True)
    assert set(ob) == set(needed) and all(v.dtype == torch.bfloat16 for v in pyr.values())
    loss = 0
    outs = {}
    for n in needed:
        ctx = a3d.ops.BuildContextFn.apply(tokens(pyr[n]), idx if n == "res1" else None, extra, None, ob[n])
        outs[n] = ctx
        loss = loss + (ctx * wts[n]).sum()
    loss.backward()
    # plain path: convolutions with bias, torch top-down, torch gather
    with torch.autocast("cuda", dtype=torch.bfloat16):
        xs = list(feats.values())
        last = ref.inner_blocks[4][0](xs[4])
        maps = {}
        for i in range(3, -1, -1):
            last = ref.inner_blocks[i][0](xs[i]) + torch.nn.functional.interpolate(last, size=xs[i].shape[-2:], mode="nearest")
            if f"res{i + 1}" in needed:
                maps[f"res{i + 1}"] = ref.layer_blocks[i][0](last)
    rloss = 0
    for n in needed:
        t = tokens(maps[n]).float()
        rows = t if n != "res1" else torch.gather(t, 1, idx[..., None].expand(N, k, E))
        rctx = torch.cat([rows, extra], dim=1)
        report(f"fpn folded-bias tokens {n}", outs[n], rctx, 2e-2, 1.6e-2)          # bf16 maps: one rounding apart
        rloss = rloss + (rctx * wts[n]).sum()
    rloss.backward()
    used = [f"inner_blocks.{i}.0" for i in range(5)] + ["layer_blocks.0.0", "layer_blocks.2.0"]
    gp, gr = dict(fpn.named_parameters()), dict(ref.named_parameters())
    for pre in used:
        for leaf in ("weight", "bias"):
            a, b = gp[f"{pre}.{leaf}"].grad, gr[f"{pre}.{leaf}"].grad
            assert a is not None and b is not None, pre
            err = (a.float() - b.float()).abs().max().item()
            sc = b.float().abs().max().item()
            print(f"[parity] fpn folded-bias grad {pre}.{leaf}: max abs err {err:.3e} (scale {sc:.3e})")
            assert err <= 3e-2 * sc + 1e-6, (pre, leaf, err, sc)
    assert gp["layer_blocks.1.0.bias"].grad is None                                    # maps nobody reads stay untouched


@pytest.mark.parametrize("B,ncam,hw,k", [(2, 2, 32, 128), (3, 1, 16, 100), (2, 4, 32, 64)])
def test_fpn_output_convolution_token_sparse_weight_gradient(a3d, dev, B, ncam, hw, k):
    """The FPN's 3x3 output convolution with its weight gradient computed from the gathers (csrc/fpn_sparse.hip through
    ops.SparseConvCtx / nn._LayerConv3x3Fn) against the library's dense backward of the same bf16 convolution: TWO gather
    levels on the same map (overlapping index sets: duplicates add up), tokens indexed over (camera, h, w), border pixels
    included (zero padding), k not a multiple of 64 (masked tail), plus the deferred bias and the input gradient, which stay on
    the library / column-sum path.  Also: a dense reader (idx None) switches the map back to the dense weight gradient."""
    import copy
    torch.manual_seed(5)
    E, Cin = 60, [64, 256, 512, 1024, 2048]
    N = B * ncam
    fpn = a3d.nn.FeaturePyramidNetwork(Cin, E).to(dev)
    ref = copy.deepcopy(fpn)
    g = torch.Generator().manual_seed(6)
    sizes = [hw, hw // 2, hw // 4, hw // 8, hw // 16]
    feats = {f"res{i + 1}": (torch.randn(N, c, s_, s_, generator=g) * 0.5).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
             for i, (c, s_) in enumerate(zip(Cin, sizes))}
    npts = ncam * hw * hw
    # two levels' index sets: unique within a level (as k-NN indices are; the map's scatter relies on it), half of level 2 shared
    # with level 1 (the same pixel in both levels: the contributions add up), the image corners included (zero padding)
    rows1, rows2 = [], []
    for _ in range(B):
        perm = torch.randperm(npts - 2, generator=g) + 1                       # 1 .. npts - 2: the corners are placed by hand
        r1 = torch.cat([torch.tensor([0]), perm[:k - 1]])
        r2 = torch.cat([torch.tensor([npts - 1]), r1[k // 2:], perm[k - 1:k - 1 + (k - 1 - (k - k // 2))]])
        assert r1.unique().numel() == k and r2.unique().numel() == k
        rows1.append(r1)
        rows2.append(r2)
    idx1, idx2 = torch.stack(rows1).to(dev), torch.stack(rows2).to(dev)
    extra = torch.randn(B, 1, E, generator=g).to(dev)
    wts = [torch.randn(B, k + 1, E, generator=g).to(dev) for _ in range(2)]

    def run(model, sparse, dense_reader=False):
        for p in model.parameters():
            p.grad = None
        keep = a3d.ops.SPARSE_FPN_WGRAD
        a3d.ops.SPARSE_FPN_WGRAD = sparse
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                res = model(feats, needed=["res1"], pad_to=64, defer_output_bias=True, sparse_ncam=ncam)
            pyr, ob = res[0], res[1]
            cc = res[2].get("res1") if len(res) > 2 else None
            assert (cc is not None) == sparse
            fm = pyr["res1"]
            tok = fm.permute(0, 2, 3, 1).reshape(B, npts, fm.shape[1])
            accum = a3d.ops.GradAccum()
            loss = 0
            for idx, w in ((idx1, wts[0]), (idx2, wts[1])):
                loss = loss + (a3d.ops.BuildContextFn.apply(tok, idx, extra, accum, ob["res1"], cc) * w).sum()
            if dense_reader:
                loss = loss + a3d.ops.BuildContextFn.apply(tok, None, extra, accum, ob["res1"], cc).sum() * 0.01
            loss.backward()
            return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        finally:
            a3d.ops.SPARSE_FPN_WGRAD = keep

    gs, gd = run(fpn, True), run(ref, False)
    assert set(gs) == set(gd)
    bad = []
    for n in sorted(gd):
        err = (gs[n] - gd[n]).abs().max().item()
        sc = gd[n].abs().max().item()
        print(f"[parity] fpn token-sparse backward, grad {n}: max abs err {err:.3e} (scale {sc:.3e})")
        # bf16 operands on both sides (the dense path rounds the SUMMED gradient map to bf16, the sparse one each gradient row)
        if err > 2e-2 * sc + 1e-6:
            bad.append((n, err, sc))
    assert not bad, bad
    w_err = (gs["layer_blocks.0.0.weight"] - gd["layer_blocks.0.0.weight"]).norm() / gd["layer_blocks.0.0.weight"].norm()
    print(f"[parity] fpn token-sparse weight gradient of the output convolution: relative L2 {w_err.item():.3e}")
    assert w_err.item() <= 5e-3
    # a dense reader of the same map: the sparse context is marked and the library's dense weight gradient takes over
    gs2, gd2 = run(fpn, True, dense_reader=True), run(ref, False, dense_reader=True)
    w2 = (gs2["layer_blocks.0.0.weight"] - gd2["layer_blocks.0.0.weight"]).abs().max().item()
    assert w2 <= 1e-2 * max(1.0, gd2["layer_blocks.0.0.weight"].abs().max().item()), w2      # the same library kernel on both sides (its bf16 result: one ulp)


@pytest.mark.parametrize("B,ncam,H,W,k", [(2, 2, 32, 64, 90), (1, 3, 16, 32, 40), (3, 1, 64, 128, 300)])
def test_conv3x3_token_sparse_input_gradient_vs_library(a3d, dev, B, ncam, H, W, k):
    """a3d_conv3x3_mark_tiles + a3d_conv3x3_dgrad_tiles (the LIST variant of the 3x3 stream kernel over the 8 x 32-pixel tiles the
    gathered tokens' neighbourhoods touch, zeros elsewhere) against the library's dense input gradient of the same bf16 convolution
    (torch.ops.aten.convolution_backward) on a gradient map that is non-zero only on the gathered pixels: clustered tokens (whole
    tiles stay unmarked), the image corners and borders included, one sample without any token in one camera."""
    g = torch.Generator().manual_seed(B * 100 + k)
    N = B * ncam
    w = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(dev).to(torch.bfloat16)
    # clustered pixel sets: k tokens per sample around a few centres (plus the two extreme corners), over (camera, h, w)
    npts = ncam * H * W
    rows = []
    for b in range(B):
        cams = torch.randint(0, ncam if b else max(1, ncam - 1), (4,), generator=g)           # sample 0 leaves the last camera empty
        cy, cx = torch.randint(0, H, (4,), generator=g), torch.randint(0, W, (4,), generator=g)
        pts = {0, (int(cams[0]) * H + H - 1) * W + W - 1}
        while len(pts) < k:
            c = int(torch.randint(0, 4, (1,), generator=g))
            y = int((cy[c] + torch.randint(-5, 6, (1,), generator=g)).clamp(0, H - 1))
            x_ = int((cx[c] + torch.randint(-9, 10, (1,), generator=g)).clamp(0, W - 1))
            pts.add((int(cams[c]) * H + y) * W + x_)
        rows.append(torch.tensor(sorted(pts))[torch.randperm(k, generator=g)])
    idx = torch.stack(rows).to(dev)
    dy = torch.zeros(B, npts, 64, device=dev, dtype=torch.bfloat16)
    dy.scatter_(1, idx[..., None].expand(B, k, 64), torch.randn(B, k, 64, generator=g).to(dev).to(torch.bfloat16))
    dy4 = dy.view(B, ncam, H, W, 64).reshape(N, H, W, 64).permute(0, 3, 1, 2)                # NCHW view of NHWC storage
    assert dy4.is_contiguous(memory_format=torch.channels_last)
    x = torch.zeros(N, 64, H, W, device=dev, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ref, _, _ = torch.ops.aten.convolution_backward(dy4, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (True, False, False))
    L = a3d.lib
    lib = L.load()
    nt = lib.a3d_conv3x3_tile_count(N, H, W)
    assert nt == N * (H // 8) * (W // 32)
    mask = torch.zeros(nt, device=dev, dtype=torch.uint8)
    L.call("a3d_conv3x3_mark_tiles", idx.data_ptr(), B, k, ncam, H, W, mask.data_ptr(), L.stream())
    ws = torch.empty(lib.a3d_conv3x3_dgrad_tiles_ws_ints(N, H, W), device=dev, dtype=torch.int32)
    wt = w.flip(2, 3).permute(1, 2, 3, 0).contiguous()
    dx = torch.full((N, H, W, 64), float("nan"), device=dev, dtype=torch.bfloat16)            # every pixel must be written
    L.call("a3d_conv3x3_dgrad_tiles", dy4.data_ptr(), wt.data_ptr(), mask.data_ptr(), ws.data_ptr(), dx.data_ptr(), N, H, W, L.stream())
    torch.cuda.synchronize()
    n_on, n_off = int(ws[0]), int(ws[1])
    assert n_on + n_off == nt and n_on == int(mask.sum()) and 0 < n_on < nt
    got = dx.permute(0, 3, 1, 2).float()
    assert torch.isfinite(got).all()
    report(f"conv3x3 token-sparse input gradient ({n_on} of {nt} tiles)", got, ref.float(), 1e-3, 1.6e-2)     # fp32 accumulation in different orders on the two sides, one bf16 rounding each: <= 2 ulp
    # unmarked tiles hold exact zeros, and the reference is zero there too (nothing outside the marked tiles was skipped wrongly)
    tile_on = mask.view(N, H // 8, W // 32).bool()
    pix_on = tile_on.repeat_interleave(8, 1).repeat_interleave(32, 2)
    assert (got.abs().amax(1)[~pix_on] == 0).all() and (ref.float().abs().amax(1)[~pix_on] == 0).all()


@pytest.mark.parametrize("mode,B,Lq,S,E,H", [("kv", 2, 37, 131, 60, 4), ("qk", 2, 70, 70, 120, 8), ("none", 1, 5, 64, 60, 4),
                                             ("kv", 1, 1, 1, 60, 4)])
def test_fused_projection_equals_unfused_operands(a3d, dev, mode, B, Lq, S, E, H):
    """a3d_proj_rope_split (projection + RoPE + operand formats in one kernel) writes exactly the operand tensors of the
    unfused path (a3d_linear_fwd + a3d_rope_split): same fp32 MFMA order, same rotation, same bf16 splits."""
    O = a3d.ops
    g = torch.Generator().manual_seed(E + Lq)
    in_w, in_b, _, _ = _mha_params(E, g, scale=2.0)
    in_w, in_b = in_w.to(dev), in_b.to(dev)
    xq = torch.randn(B, Lq, E, generator=g).to(dev)
    xk = xq if mode == "qk" else torch.randn(B, S, E, generator=g).to(dev)
    xv = xk if mode == "kv" else torch.randn(B, S, E, generator=g).to(dev)
    q_xyz = (torch.rand(B, Lq, 3, generator=g) * 2 - 0.5).to(dev)
    k_xyz = q_xyz if mode == "qk" else (torch.rand(B, S, 3, generator=g) * 2 - 0.5).to(dev)
    fused = O.attn_operands_fused(mode, xq, xk, xv, in_w.data_ptr(), in_b.data_ptr(), q_xyz, k_xyz, B, Lq, S, E, H, dev,
                                  need_bwd=True)
    y = O.linear2d(torch.cat([xq.reshape(-1, E)]), in_w[:E], in_b[:E])
    yk = O.linear2d(xk.reshape(-1, E), in_w[E:2 * E], in_b[E:2 * E])
    yv = O.linear2d(xv.reshape(-1, E), in_w[2 * E:], in_b[2 * E:])
    ref = O.attn_operands(y.data_ptr(), E, yk.data_ptr(), E, yv.data_ptr(), E, q_xyz, k_xyz, B, Lq, S, E, H, dev, need_bwd=True)
    def value(t, rows):
        """fp32 value carried by an operand tensor: sum of its bf16 parts (rows: 16-wide column groups; planes: dim 2)."""
        t = t.float()
        return t.view(*t.shape[:-1], t.shape[-1] // 16, 16).sum(-2) if rows else t.sum(2)

    # same fp32 MFMA order, same angles; the two kernels may contract the rotation's multiply-adds differently, so the
    # carried values agree to an fp32 ulp of the tensor scale (the hi / lo parts then agree exactly almost everywhere)
    # three-part rows carry 24 bits (tolerance: an fp32 ulp of the scale); two-part tensors 16 bits (their last part
    # may round the other way when the fp32 input moves by an ulp: 2^-16 of the scale)
    for n, a, b, rows, tol in [("Qs", fused[0], ref[0], True, 4e-7), ("Ks", fused[1], ref[1], True, 4e-7),
                               ("Vt", fused[2], ref[2], False, 2e-5), ("Qt", fused[7][0], ref[7][0], False, 2e-5),
                               ("Kt", fused[7][1], ref[7][1], False, 2e-5), ("Vs", fused[7][2], ref[7][2], True, 2e-5)]:
        assert a.shape == b.shape, f"{mode}: {n} shape"
        va, vb = value(a, rows), value(b, rows)
        err = (va - vb).abs().max().item()
        assert err <= tol * max(vb.abs().max().item(), 1e-30), f"{mode}: {n} differs by {err:.3e}"
        if rows:
            same_hi = (a[..., :16].view(torch.int16) == b[..., :16].view(torch.int16)).float().mean().item()
            assert same_hi > 0.999, f"{mode}: {n} hi parts agree only {same_hi:.4f}"
    assert fused[3:6] == ref[3:6]


def test_attention_edge_shapes(a3d, dev):
    """One query / one key, a key count that is an exact multiple of the 64-key chunk, and a sample whose keys are all
    padding except one (the softmax collapses onto it) -- against the oracle."""
    O = a3d.ops
    g = torch.Generator().manual_seed(11)
    E, H = 60, 4
    in_w, in_b, out_w, out_b = _mha_params(E, g, scale=1.5)
    ln_g, ln_b = torch.ones(E), torch.zeros(E)
    for B, Lq, S, keep in [(1, 1, 1, None), (2, 3, 64, None), (2, 17, 128, 1), (1, 64, 65, 3)]:
        xq = torch.randn(B, Lq, E, generator=g)
        xk = torch.randn(B, S, E, generator=g)
        kmask = None
        if keep is not None:
            kmask = torch.ones(B, S, dtype=torch.bool)
            kmask[:, :keep] = False
        ref = OB.layer_norm(xq + OB.mha(xq, xk, xk, in_w, in_b, out_w, out_b, H, None, None, kmask), ln_g, ln_b)
        mha, norm = _mk_modules(dev, in_w, in_b, out_w, out_b, ln_g, ln_b)
        kd = xk.to(dev)
        y = O.attn_block(xq.to(dev), kd, kd, xq.to(dev), None, None, None if kmask is None else kmask.to(dev), mha, norm, H)
        report(f"attn edge B={B} Lq={Lq} S={S} keep={keep}", y, ref, 1e-4)


def test_metric_tables_and_optional_losses_vs_reference_golden(a3d, dev):
    """LossAndMetrics.compute_metrics (per-task table), TrajectoryCriterion.compute_metrics, symmetric_rotation_loss and
    position_loss="mse" against values recorded from the reference (tests/golden/metrics.pt)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import common as C
    g = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.pt"), weights_only=False)
    pred, gt, action, kp, tasks = C.metrics_inputs()
    summ, per = a3d.TrajectoryCriterion.compute_metrics(pred.to(dev), gt.to(dev), None)
    assert set(summ) == set(g["traj"]["summary"]) and set(per) == set(g["traj"]["per_traj"])
    for k, v in g["traj"]["summary"].items():
        report("traj metric " + k, summ[k], v, 1e-6)
    for k, v in g["traj"]["per_traj"].items():
        report("traj per-trajectory " + k, per[k], v, 1e-6)
    for sym in (False, True):
        r = g[f"keypose_sym{int(sym)}"]
        crit = a3d.LossAndMetrics(position_loss="mse", rotation_parametrization="quat_from_query",
                                  ground_truth_gaussian_spread=0.01, symmetric_rotation_loss=sym)
        p = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in kp.items()}
        p["rotation"] = p["rotation"].clone().requires_grad_()
        sample = {"action": action.to(dev), "task": tasks}
        losses = crit.compute_loss(p, sample)
        assert set(losses) == set(r["losses"])
        for k, v in r["losses"].items():
            report(f"sym={sym} loss {k}", losses[k], v, 1e-5)
        sum(losses.values()).backward()
        report(f"sym={sym} d rotation", p["rotation"].grad, r["d_rotation"], 1e-6)
        m = crit.compute_metrics({k: (v.detach() if torch.is_tensor(v) else v) for k, v in p.items()}, sample)
        assert set(m) == set(r["metrics"]), sorted(set(m) ^ set(r["metrics"]))
        for k, v in r["metrics"].items():
            report(f"sym={sym} metric {k}", m[k], v, 1e-6)


def test_pose_signal_kernels_vs_oracle_and_golden(a3d, dev):
    """a3d_pose_to_signal / a3d_signal_to_pose (normalisation + quaternion <-> 6D) vs the oracle's restatement of
    diffusion_model.py:187-230 and the reference's recorded conversions (tests/golden/diffusion.pt "rot")."""
    from oracle import diffusion as OD
    D = a3d.diffusion
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import common as C
    g = torch.Generator().manual_seed(4)
    bounds = torch.from_numpy(C.DIFFUSION_BOUNDS).float()
    for extra in (0, 1):
        pose = torch.cat([torch.rand(3, 37, 3, generator=g) * 2 - 1, torch.randn(3, 37, 4, generator=g),
                          torch.rand(3, 37, extra, generator=g)], dim=-1)
        ref = pose.clone()
        ref[..., :3] = OD.normalize_pos(ref[..., :3], bounds)
        ref = OD.convert_rot(ref)
        got = D.pose_to_signal(pose.to(dev), bounds.to(dev))
        report("pose -> signal", got, ref, 2e-6)
        report("pose -> signal (no bounds)", D.pose_to_signal(pose.to(dev)), OD.convert_rot(pose), 2e-6)
        sig = torch.cat([torch.rand(3, 37, 3, generator=g) * 2 - 1, torch.randn(3, 37, 6, generator=g),
                         torch.rand(3, 37, extra, generator=g)], dim=-1)
        back = OD.unconvert_rot(sig)
        back = torch.cat([OD.unnormalize_pos(back[..., :3], bounds), back[..., 3:]], dim=-1)
        report("signal -> pose", D.signal_to_pose(sig.to(dev), bounds.to(dev)), back, 5e-6)
    r = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diffusion.pt"), weights_only=False)["rot"]
    pose = torch.cat([torch.zeros(6, 3), r["q"]], dim=-1)
    report("reference 6D", D.pose_to_signal(pose.to(dev))[:, 3:], r["o6"], 2e-6)
    sig = torch.cat([torch.zeros(6, 3), r["o6"]], dim=-1)
    report("reference quaternion", D.signal_to_pose(sig.to(dev))[:, 3:], r["q_back"], 2e-6)


def test_rgb_normalize_kernel_matches_torch(a3d, dev):
    """a3d_rgb_normalize_nhwc_bf16 == ClipNormalize -> channels_last -> bf16 cast, bit for bit"""
    g = torch.Generator().manual_seed(9)
    x = torch.rand(3, 3, 128, 128, generator=g).to(dev)
    norm = a3d.nn.ClipNormalize().to(dev)
    ref = norm(x).contiguous(memory_format=torch.channels_last).to(torch.bfloat16)
    got = a3d.nn.normalize_to_nhwc_bf16(x, norm)
    assert got.is_contiguous(memory_format=torch.channels_last) and got.shape == ref.shape
    assert torch.equal(got, ref)


def test_option_head_kernels(a3d, dev):
    """Kernels of Act3D's non-default options: 6D -> rotation matrix + sigmoid with its analytic backward
    (act3d.py:529-533, utils.py:93-130), the top-ghost row selection (act3d.py:513-522) and the batch-sum backward of the
    instruction position embedding (act3d.py:201-209), each against torch autograd of the oracle's restatement."""
    O = a3d.ops
    g = torch.Generator().manual_seed(7)
    # ---- ortho6d + sigmoid
    pred = torch.randn(9, 7, generator=g)
    pred[3, :3] *= 1e-3                                        # a short first axis (normalisation well away from 1)
    w_rot, w_grip = torch.randn(9, 3, 3, generator=g), torch.randn(9, 1, generator=g)
    pc = pred.clone().requires_grad_()
    rot_ref, grip_ref = OA.ortho6d_to_matrix(pc[:, :6]), torch.sigmoid(pc[:, 6:])
    ((rot_ref * w_rot).sum() + (grip_ref * w_grip).sum()).backward()
    pd = pred.to(dev).requires_grad_()
    rot, grip = O.Ortho6dSigmoidFn.apply(pd)
    ((rot * w_rot.to(dev)).sum() + (grip * w_grip.to(dev)).sum()).backward()
    report("6D rotation", rot, rot_ref, 2e-6, 1e-6)
    report("6D gripper", grip, grip_ref, 1e-6)
    report("6D d pred", pd.grad, pc.grad, 2e-5, 1e-5)
    eye = torch.eye(3).expand(9, 3, 3)
    report("R^T R", rot.transpose(1, 2) @ rot, eye, 1e-5)
    # ---- select row (W = 3 offsets, W = 60 features)
    for W in (3, 60):
        x = torch.randn(4, 37, W, generator=g)
        idx = torch.tensor([0, 36, 5, 5])
        dy = torch.randn(4, W, generator=g)
        xd = x.to(dev).requires_grad_()
        y = O.SelectRowFn.apply(xd, idx.to(dev))
        y.backward(dy.to(dev))
        assert torch.equal(y.cpu(), x[torch.arange(4), idx])
        ref = torch.zeros_like(x)
        ref[torch.arange(4), idx] = dy
        assert torch.equal(xd.grad.cpu(), ref)
    # ---- broadcast add of shared rows: gradient of the rows = sum over the batch
    x, r = torch.randn(5, 53, 60, generator=g), torch.randn(53, 60, generator=g)
    dy = torch.randn(5, 53, 60, generator=g)
    xd, rd = x.to(dev).requires_grad_(), r.to(dev).requires_grad_()
    y = O.AddRowsFn.apply(xd, rd)
    y.backward(dy.to(dev))
    assert torch.equal(y.cpu(), x + r[None])
    assert torch.equal(xd.grad.cpu(), dy)
    report("d rows", rd.grad, dy.sum(0), 1e-5, 1e-6)


@pytest.mark.parametrize("M,K,N,pro", [(1000, 256, 64, True), (4096, 64, 256, False), (16, 128, 256, True),
                                       # every (waves along N, K steps) instance, workgroups with fewer steps than the prefetch depth
                                       # and with many tiles, ragged last tiles
                                       (5000, 64, 64, True), (3000, 256, 128, True), (70001, 128, 512, False), (100000, 64, 256, True),
                                       (400003, 64, 256, False), (150000, 128, 128, True), (9000, 64, 128, False), (33000, 128, 64, True),
                                       # the deep-layer GEMM (conv1x1_deep.hip): every backbone shape class, ragged M, one / many tiles per workgroup
                                       (16384, 512, 2048, False), (16384, 2048, 512, False), (65536, 1024, 256, False), (65536, 256, 1024, True),
                                       (70001, 512, 128, True), (300, 1024, 2048, False), (40000, 512, 1024, True), (130, 128, 128, True)])
def test_conv1x1_gemm_with_folded_batchnorm(a3d, dev, M, K, N, pro):
    """a3d_conv1x1_bn_fwd: y = bf16(f(x) w^T) with f = the producer's BatchNorm-apply + ReLU (rounded to bf16 as the unfused
    path materialises it), fp32 accumulation, and the per-slab (sum, sum of squares) of the rounded outputs."""
    _check_conv1x1(a3d, dev, M, K, N, pro)


def _check_conv1x1(a3d, dev, M, K, N, pro):
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    sc = (1.0 + 0.3 * torch.randn(K, generator=g)) if pro else None
    sh = (0.2 * torch.randn(K, generator=g)) if pro else None
    xd, wd = x.to(dev), w.to(dev)
    y = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
    nslab = a3d.lib.load().a3d_conv1x1_nslab(M, K, N)
    part = torch.zeros((nslab, 2, N), device=dev, dtype=torch.float32)
    scd = None if sc is None else sc.to(dev).contiguous()
    shd = None if sh is None else sh.to(dev).contiguous()
    a3d.lib.call("a3d_conv1x1_bn_fwd", xd.data_ptr(), wd.data_ptr(), None if scd is None else scd.data_ptr(),
                 None if shd is None else shd.data_ptr(), 1 if pro else 0, y.data_ptr(), part.data_ptr(), M, K, N, a3d.lib.stream())
    torch.cuda.synchronize()
    xf = x.float()
    if pro:
        # x * scale + shift as ONE rounding (the kernel's fma, the same expression a3d_bn_apply evaluates on the unfused path)
        xf = torch.relu((xf.double() * sc.double() + sh.double()).float()).to(torch.bfloat16).float()
    ref = xf.double() @ w.double().t()
    got = y.float().cpu()
    # one bf16 rounding of an fp32-accumulated sum: half an ulp (2^-9 relative) plus accumulation noise
    err = (got.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-3
    assert torch.isfinite(got).all()
    assert (err <= tol).all(), f"max err {err.max().item():.3e} at {torch.nonzero(err > tol)[:3].tolist()}"
    s = part.sum(0).cpu()
    report("sum", s[0], got.sum(0), 1e-2, 1e-4)
    report("sum of squares", s[1], (got * got).sum(0), 1e-2, 1e-4)


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 16, 32, 32, 32), (3, 24, 64, 32, 64), (2, 16, 32, 64, 64), (5, 8, 96, 64, 64),
                                            (1, 64, 64, 32, 32)])
@pytest.mark.parametrize("pro", [False, True])
def test_conv3x3_gemm_with_folded_batchnorm(a3d, dev, N, H, W, Cin, Cout, pro):
    """a3d_conv3x3_bn_fwd: y = bf16(conv3x3(f(x), w)) with f = the producer's BatchNorm-apply + ReLU (rounded to bf16 as the
    unfused path materialises it), zero padding of the NORMALISED map, fp32 accumulation, and the per-slab (sum, sum of squares)
    of the rounded outputs; the reference is F.conv2d in float64 on the same bf16 operands (clip.py:22-43: padding=1, no bias)."""
    g = torch.Generator().manual_seed(N * 1000 + H + W + Cin + Cout)
    x = torch.randn(N, Cin, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(torch.bfloat16)
    sc = (1.0 + 0.3 * torch.randn(Cin, generator=g)) if pro else None
    sh = (0.2 * torch.randn(Cin, generator=g)) if pro else None      # non-zero shift: a wrongly padded border would show relu(shift)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1, bias=False).to(dev).to(torch.bfloat16)
    conv.weight.data = w.to(dev).contiguous(memory_format=torch.channels_last)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    scale = None if not pro else torch.stack([sc, sh]).to(dev).contiguous()
    assert a3d.nn.conv3x3_serves(xd, conv)
    y, part = a3d.nn.conv3x3_bn(xd, conv, in_scale=scale, in_relu=pro, want_stats=True)
    torch.cuda.synchronize()
    assert y.shape == (N, Cout, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    assert part.shape == (a3d.lib.load().a3d_conv3x3_nslab(N, H, W, Cin, Cout), 2, Cout)
    xf = x.float()
    if pro:
        # x * scale + shift as ONE rounding (the kernel's fma, the same expression a3d_bn_apply evaluates on the unfused path)
        xf = torch.relu((xf.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float()).to(torch.bfloat16).float()
    ref = F.conv2d(xf.double(), w.double(), padding=1)
    got = y.float().cpu()
    err = (got.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-3          # one bf16 rounding of an fp32-accumulated sum
    assert torch.isfinite(got).all()
    assert (err <= tol).all(), f"max err {err.max().item():.3e} at {torch.nonzero(err > tol)[:3].tolist()}"
    print(f"[parity] conv3x3 {Cin}->{Cout} {N}x{H}x{W} pro={pro}: max_abs_err={err.max().item():.3e} ref_absmax={ref.abs().max().item():.3e}")
    s = part.sum(0).cpu()
    report("conv3x3 sum", s[0], got.sum((0, 2, 3)), 1e-2, 1e-4)
    report("conv3x3 sum of squares", s[1], (got * got).sum((0, 2, 3)), 1e-2, 1e-4)
    # without the statistics epilogue: same map
    y2, p2 = a3d.nn.conv3x3_bn(xd, conv, in_scale=scale, in_relu=pro, want_stats=False)
    assert p2 is None and torch.equal(y2, y)


@pytest.mark.parametrize("N,H,W", [(2, 64, 64), (3, 32, 128), (1, 256, 256), (5, 16, 64)])
@pytest.mark.parametrize("stats", [True, False])
def test_stem_convolution_with_folded_normalisation_and_statistics(a3d, dev, N, H, W, stats):
    """a3d_stem_conv_bn_fwd: y = bf16(conv_{3x3, stride 2, pad 1}(bf16((rgb - mean) / std), w)) on the raw fp32 images (clip.py:22-43
    conv1 behind act3d.py:365's normalisation), zero padding of the NORMALISED map, fp32 accumulation, and the per-slab (sum, sum of
    squares) of the rounded outputs; the reference is F.conv2d in float64 on the bf16-rounded normalised image and the bf16 weight."""
    g = torch.Generator().manual_seed(N * 1000 + H + W)
    x = torch.rand(N, 3, H, W, generator=g)
    norm = a3d.nn.ClipNormalize()
    conv = torch.nn.Conv2d(3, 32, 3, stride=2, padding=1, bias=False)
    conv.weight.data = torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5
    conv = conv.to(dev).to(torch.bfloat16)
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)      # as run_frozen_backbone stores the frozen weights
    xd, normd = x.to(dev), a3d.nn.ClipNormalize().to(dev)
    assert a3d.nn.stem_serves(xd, conv, normd)
    y, part = a3d.nn.stem_conv_bn(xd, conv, normd, want_stats=stats)
    torch.cuda.synchronize()
    assert y.shape == (N, 32, H // 2, W // 2) and y.is_contiguous(memory_format=torch.channels_last)
    xn = ((x - norm.mean) / norm.std).to(torch.bfloat16).double()
    ref = F.conv2d(xn, conv.weight.detach().cpu().double(), stride=2, padding=1)
    got = y.float().cpu()
    err = (got.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-3          # one bf16 rounding of an fp32-accumulated sum
    assert torch.isfinite(got).all()
    assert (err <= tol).all(), f"max err {err.max().item():.3e} at {torch.nonzero(err > tol)[:3].tolist()}"
    print(f"[parity] stem conv {N}x{H}x{W}: max_abs_err={err.max().item():.3e} ref_absmax={ref.abs().max().item():.3e}")
    if stats:
        assert part.shape == (a3d.lib.load().a3d_stem_conv_nslab(N, H, W), 2, 32)
        s_ = part.sum(0).cpu()
        report("stem conv sum", s_[0], got.sum((0, 2, 3)), 1e-2, 1e-4)
        report("stem conv sum of squares", s_[1], (got * got).sum((0, 2, 3)), 1e-2, 1e-4)
    else:
        assert part is None
    # shapes it refuses fall back to the library path
    assert not a3d.nn.stem_serves(torch.zeros(1, 3, 24, 64, device=dev), conv, normd)


def test_backbone_with_fused_1x1_convolutions_matches_miopen_path(a3d, dev):
    """The backbone path with the layer-1 / layer-2 1x1 convolutions through a3d_conv1x1_bn_fwd (bn2-apply folded into conv3's
    operand load, output statistics from the GEMM epilogue; default) must be as close to the fp32 module as the all-MIOpen bf16
    path (A3D_FUSED_CONV1X1=0: MIOpen convolutions + separate BatchNorm kernels) is -- two bf16 evaluations of ~50 layers differ from each other by a few
    percent in the deep maps, so each is measured against fp32."""
    import copy
    torch.manual_seed(0)
    bb32 = a3d.nn.SyntheticCLIPResNet50().to(dev).train()
    nets = {False: copy.deepcopy(bb32), True: copy.deepcopy(bb32), "1x1": copy.deepcopy(bb32)}
    x = torch.rand(4, 3, 128, 128, device=dev).contiguous(memory_format=torch.channels_last)
    outs = {}
    keep = a3d.nn.FUSED_CONV1X1, a3d.nn.FUSED_CONV3X3
    with torch.no_grad():
        ref = bb32(x)
        for flag, net in nets.items():
            # False: MIOpen everywhere; True (default): the streaming 1x1 GEMM and the 3x3 implicit GEMM on the shapes they serve;
            # "1x1": only the 1x1 GEMM (the round-4 path before conv3x3.hip)
            a3d.nn.FUSED_CONV1X1, a3d.nn.FUSED_CONV3X3 = bool(flag), flag is True
            try:
                outs[flag] = a3d.nn.run_frozen_backbone(net, x.clone(), torch.bfloat16)
            finally:
                a3d.nn.FUSED_CONV1X1, a3d.nn.FUSED_CONV3X3 = keep
    rms = lambda t: t.float().pow(2).mean().sqrt().item()
    for k in ref:
        e_f, e_1, e_d, sc = rms(outs[True][k] - ref[k]), rms(outs["1x1"][k] - ref[k]), rms(outs[False][k] - ref[k]), rms(ref[k])
        print(f"[parity] backbone {k}: rms_err fused-1x1+3x3={e_f:.3e} fused-1x1={e_1:.3e} all-MIOpen={e_d:.3e} ref_rms={sc:.3e}")
        assert torch.isfinite(outs[True][k]).all() and e_f <= 1.25 * e_d + 1e-3 * sc, k
        assert e_1 <= 1.25 * e_d + 1e-3 * sc, k
    for (n, p), (_, q) in zip(bb32.named_buffers(), nets[True].named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert torch.equal(p, q), n
    report("layer1 running_mean", nets[True].layer1[0].bn1.running_mean, bb32.layer1[0].bn1.running_mean, 1e-3, 1e-2)
    report("layer4 running_var", nets[True].layer4[2].bn3.running_var, bb32.layer4[2].bn3.running_var, 1e-3, 5e-2)
