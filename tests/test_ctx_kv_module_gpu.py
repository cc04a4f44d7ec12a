"""RelativeCrossAttentionModule with the batched context projection (ops.CTX_KV_BATCH: one a3d_ctx_kv_proj16 launch for the k | v rows
of both layers) against the same module with per-layer a3d_proj_rope_split16 launches, from identical parameters: forward and backward
with a GradSink attached to the context as act3d.py does.

Bars: the project's own parity bars -- outputs within 1e-3 of the tensor scale, parameter and context gradients within
1.5e-3 of the gradient scale.  A larger on / off difference would let one path fail the oracle tests the other passes; the observed
differences are printed and are expected to be orders of magnitude below the bars (the two kernels sum the 60-term contraction in a
different order, nothing else differs).
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
E, H, NL, B, LQ, S = 60, 4, 2, 2, 40, 150


class _Counter:
    """Counting wrapper round lib.call: name -> list of argument tuples."""
    def __init__(self, L):
        self.L, self.orig, self.calls = L, L.call, {}

    def __enter__(self):
        def call(name, *args):
            self.calls.setdefault(name, []).append(args)
            return self.orig(name, *args)
        self.L.call = call
        return self

    def __exit__(self, *exc):
        self.L.call = self.orig


def _inputs(dev):
    g = torch.Generator().manual_seed(777)
    q = torch.randn(B, LQ, E, generator=g).to(dev)
    ctx = torch.randn(B, S, E, generator=g).to(dev)
    qx = (torch.rand(B, LQ, 3, generator=g) * 2 - 0.5).to(dev)
    cx = (torch.rand(B, S, 3, generator=g) * 2 - 0.5).to(dev)
    dys = [torch.randn(B, LQ, E, generator=g).to(dev) for _ in range(NL)]
    return q, ctx, qx, cx, dys


def _run(a3d, mod, q, ctx, qx, cx, dys, batch):
    O_ = a3d.ops
    old = O_.CTX_KV_BATCH
    O_.CTX_KV_BATCH = batch
    try:
        for p in mod.parameters():
            p.grad = None
        q = q.clone().requires_grad_(True)
        leaf = ctx.clone().requires_grad_(True)
        registry = []
        with _Counter(a3d.lib) as cnt:
            c = O_.attach_grad_sink(leaf * 1.0, registry)          # a non-leaf context, as the model's (the gate node owns the sink)
            assert getattr(c, "_a3d_sink", None) is not None
            outs = mod(q, c, qx, cx)
            loss = sum((o * dy).sum() for o, dy in zip(outs, dys))
            loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in mod.named_parameters()}
        return [o.detach().clone() for o in outs], grads, leaf.grad.detach().clone(), q.grad.detach().clone(), cnt.calls
    finally:
        O_.CTX_KV_BATCH = old


def _big_kv_calls(calls):
    """a3d_proj_rope_split16 launches over the S context rows (two output blocks: k | v)."""
    return [a for a in calls.get("a3d_proj_rope_split16", []) if a[18] == S and a[13] is not None]


def test_module_batched_context_projection_matches_per_layer_launches(a3d, dev):
    torch.manual_seed(5)
    mod = a3d.nn.RelativeCrossAttentionModule(E, H, NL).to(dev)
    for n, p in mod.named_parameters():                             # biases and norms away from their trivial initial values
        if p.dim() == 1:
            torch.nn.init.normal_(p, mean=1.0 if ("norm" in n and n.endswith("weight")) else 0.0, std=0.5)
    ref = copy.deepcopy(mod)
    q, ctx, qx, cx, dys = _inputs(dev)
    on = _run(a3d, mod, q, ctx, qx, cx, dys, True)
    off = _run(a3d, ref, q, ctx, qx, cx, dys, False)

    assert len(on[4].get("a3d_ctx_kv_proj16", [])) == 1, "the batched path makes exactly one context launch"
    assert _big_kv_calls(on[4]) == [], "the per-layer k | v launch over the context is still made with the switch on"
    assert len(on[4].get("a3d_proj_rope_split16", [])) == NL, "the q projections stay, one per layer"
    assert "a3d_ctx_kv_proj16" not in off[4] and len(_big_kv_calls(off[4])) == NL

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()

    for l in range(NL):
        r = rel(on[0][l], off[0][l])
        print(f"[parity] ctx kv module: layer {l} output on/off max_abs_diff / scale = {r:.3e} (bar 1e-3)")
        assert torch.isfinite(on[0][l]).all() and r <= 1e-3, (l, r)
    worst = 0.0
    for n in on[1]:
        r = rel(on[1][n], off[1][n])
        worst = max(worst, r)
        print(f"[parity] ctx kv module: grad {n} on/off = {r:.3e}")
        assert torch.isfinite(on[1][n]).all() and r <= 1.5e-3, (n, r)
    rc, rq = rel(on[2], off[2]), rel(on[3], off[3])
    print(f"[parity] ctx kv module: context grad on/off = {rc:.3e}, query grad = {rq:.3e}, worst parameter grad = {worst:.3e} (bar 1.5e-3)")
    assert torch.isfinite(on[2]).all() and rc <= 1.5e-3 and rq <= 1.5e-3, (rc, rq)

    # the same forward without a gradient takes the batched path too
    O_ = a3d.ops
    old = O_.CTX_KV_BATCH
    O_.CTX_KV_BATCH = True
    try:
        with torch.no_grad(), _Counter(a3d.lib) as cnt:
            outs = mod(q, ctx, qx, cx)
        torch.cuda.synchronize()
    finally:
        O_.CTX_KV_BATCH = old
    assert len(cnt.calls.get("a3d_ctx_kv_proj16", [])) == 1 and _big_kv_calls(cnt.calls) == []
    for l in range(NL):
        r = rel(outs[l], off[0][l])
        print(f"[parity] ctx kv module: no_grad layer {l} output vs per-layer launches = {r:.3e}")
        assert r <= 1e-3, (l, r)
