"""Deferred gradient reductions (ops.ReduceQueue, a3d_grad_reduce_table) and the LayerNorm backward without same-address atomics.

Bounds (u = 2^-24, the unit roundoff of fp32; nothing here is tuned to what the kernels give):
  * a sum of n fp32 terms formed in ANY order differs from the exact sum by at most (n - 1) u sum|terms| (to first order).  The
    reductions here are trees: a chain of `rows per chain` adds inside a lane, 64 LDS slots, then the partial records, then one
    add into the destination -- the depth of that tree replaces n - 1.
  * LayerNorm dS per element: dS = rstd (gy - s1 - xh s2), gy = dy gamma, s1 = mean(gy), s2 = mean(gy xh).  xh is formed in fp32
    from x = fl(A + R): |d xh| <= u (|x| rstd + 2 |xh|).  The two E-term means are off by at most (E - 1) u of their absolute
    sums, the four remaining operations by u each:
        |d dS| <= rstd [ (E + 8) u (|gy| + mean|gy| + |xh| mean|gy xh|) + |d xh| |s2| + |xh| mean(|gy| |d xh|) ].
    This is the bound any fp32 evaluation of the formula meets, the row-per-wave kernel included.
  * dgamma / dbeta per channel: (rows per chain + 64 + partial count + 2) u sum|terms| (+ sum|dy| |d xh| for dgamma: the
    terms themselves carry xh's rounding), + u |prefill| for the add into a pre-filled buffer.
  * reduce table: (nsplit + records) u sum|partials| per output, as the sum of nsplit * records terms in a tree of that depth.
"""
import ctypes
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_case(dev, M, E, with_r, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, E, generator=g).to(dev)
    r = (torch.randn(M, E, generator=g) * 0.7).to(dev) if with_r else None
    dy = torch.randn(M, E, generator=g).to(dev)
    gam = (torch.rand(E, generator=g) + 0.5).to(dev)
    bet = torch.randn(E, generator=g).to(dev)
    return a, r, dy, gam, bet


def _ln_reference(a, r, dy, gam, mean, rstd):
    """float64 evaluation on the fp32 inputs (mean / rstd as the forward kernel saved them) and the bounds of the docstring"""
    E = a.shape[1]
    x = a.double() + (0 if r is None else r.double())
    rs, mu = rstd.double()[:, None], mean.double()[:, None]
    xh = (x - mu) * rs
    gy = dy.double() * gam.double()
    s1, s2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    ds = rs * (gy - s1 - xh * s2)
    dxh = U * (x.abs() * rs + 2 * xh.abs())
    ds_bound = rs * ((E + 8) * U * (gy.abs() + gy.abs().mean(1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(1, keepdim=True))
                     + dxh * s2.abs() + xh.abs() * (gy.abs() * dxh).mean(1, keepdim=True))
    tg, tb = dy.double() * xh, dy.double()
    return ds, ds_bound, tg.sum(0), tb.sum(0), tg.abs().sum(0), tb.abs().sum(0), (dy.double().abs() * dxh).sum(0)


def _ln_depth(a3d, M, E):
    cnt = a3d.lib.load().a3d_add_layernorm_bwd_partials_count(M, E)
    assert 0 < cnt <= 256
    rows_per_wg = -(-(-(-M // 256)) // 64) * 64                 # whole 64-row passes (16 waves x 4 rows), at most 256 workgroups
    assert cnt == -(-M // rows_per_wg)
    return rows_per_wg // 64 + 64 + cnt + 2                      # a lane's chain, the 64 LDS slots, the records, the two final adds


@pytest.mark.parametrize("with_r", [True, False])
@pytest.mark.parametrize("E", [12, 60, 64])
def test_layernorm_backward_small_e_against_float64(a3d, dev, E, with_r):
    O, L = a3d.ops, a3d.lib
    for M in (1, 3, 4, 63, 64, 65, 257, 1332):
        a, r, dy, gam, bet = _ln_case(dev, M, E, with_r, 1000 * E + M)
        G, Bt = torch.nn.Parameter(gam), torch.nn.Parameter(bet)
        _, mean, rstd = O.add_layernorm(a, r, G, Bt)
        ds_ref, ds_bound, dg_ref, db_ref, ag, ab, xg = _ln_reference(a, r, dy, gam, mean, rstd)
        depth = _ln_depth(a3d, M, E)
        pre_g = torch.linspace(-3.0, 5.0, E, device=dev)
        pre_b = torch.linspace(2.0, -1.0, E, device=dev)
        bound_g = depth * U * ag + xg + U * pre_g.double().abs()
        bound_b = depth * U * ab + U * pre_b.double().abs()
        for entry in ("ops", "direct"):
            G.grad, Bt.grad = pre_g.clone(), pre_b.clone()             # pre-filled: the result is added, not stored
            if entry == "ops":                                         # partial records + the fixed-order finish
                ds = O.add_layernorm_bwd(a, r, G, Bt, mean, rstd, dy)
            else:                                                      # the C entry existing callers use
                ds = torch.empty_like(a)
                L.call("a3d_add_layernorm_bwd", a.data_ptr(), None if r is None else r.data_ptr(), G.data_ptr(), mean.data_ptr(),
                       rstd.data_ptr(), dy.data_ptr(), ds.data_ptr(), G.grad.data_ptr(), Bt.grad.data_ptr(), M, E, L.stream())
            torch.cuda.synchronize()
            e_ds = ((ds.double() - ds_ref).abs() / ds_bound).max().item()
            e_g = ((G.grad.double() - pre_g.double() - dg_ref).abs() / bound_g).max().item()
            e_b = ((Bt.grad.double() - pre_b.double() - db_ref).abs() / bound_b).max().item()
            print(f"[ln_bwd] {entry:6s} M={M:5d} E={E} R={with_r}: err / bound  dS {e_ds:.3f}  dgamma {e_g:.3f}  dbeta {e_b:.3f}")
            assert torch.isfinite(ds).all() and e_ds <= 1.0, (entry, M, e_ds)
            assert e_g <= 1.0 and e_b <= 1.0, (entry, M, e_g, e_b)


def test_layernorm_backward_partials_entry_is_deterministic_and_leaves_records(a3d, dev):
    """the first stage alone: records [count][2][E] whose float64 column sums are the gradients; same bits on a second launch"""
    O, L = a3d.ops, a3d.lib
    M, E = 1332, 60
    a, r, dy, gam, bet = _ln_case(dev, M, E, True, 77)
    _, mean, rstd = O.add_layernorm(a, r, gam, bet)
    _, _, dg_ref, db_ref, ag, ab, xg = _ln_reference(a, r, dy, gam, mean, rstd)
    cnt = L.load().a3d_add_layernorm_bwd_partials_count(M, E)
    outs = []
    for _ in range(2):
        part = torch.full((cnt + 1, 2, E), 777.0, device=dev)
        ds = torch.empty_like(a)
        L.call("a3d_add_layernorm_bwd_partials", a.data_ptr(), r.data_ptr(), gam.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
               dy.data_ptr(), ds.data_ptr(), part.data_ptr(), M, E, L.stream())
        torch.cuda.synchronize()
        outs.append((ds, part))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    part = outs[0][1]
    assert (part[cnt] == 777.0).all(), "a record past the reported count was written"
    depth = _ln_depth(a3d, M, E)
    assert ((part[:cnt, 0].double().sum(0) - dg_ref).abs() <= depth * U * ag + xg).all()
    assert ((part[:cnt, 1].double().sum(0) - db_ref).abs() <= depth * U * ab).all()


def test_layernorm_backward_e120_keeps_its_bits(a3d, dev):
    """64 < E <= 128 is served by the kernel it was served by before: dS bit for bit as recorded from the tree this change started
    from (tests/golden/ln_bwd_e120.pt holds the inputs and that result); dgamma / dbeta end in float atomics there, so they are
    compared to the recorded values within the order bound 2 (M + 1) u sum|terms| <= 2 (M + 1) u M max|term| of two such runs."""
    O = a3d.ops
    rec = torch.load(os.path.join(GOLDEN, "ln_bwd_e120.pt"))
    a, r, dy, gam, bet = (rec[k].to(dev) for k in ("a", "r", "dy", "gamma", "beta"))
    G, Bt = torch.nn.Parameter(gam), torch.nn.Parameter(bet)
    _, mean, rstd = O.add_layernorm(a, r, G, Bt)
    ds = O.add_layernorm_bwd(a, r, G, Bt, mean, rstd, dy)
    torch.cuda.synchronize()
    assert torch.equal(mean.cpu(), rec["mean"]) and torch.equal(rstd.cpu(), rec["rstd"])
    assert torch.equal(ds.cpu(), rec["ds"]), "the E = 120 LayerNorm backward changed its dS bits"
    M = a.shape[0]
    xh = ((a.double() + r.double()) - mean.double()[:, None]) * rstd.double()[:, None]
    bg = 2 * (M + 1) * U * (dy.double() * xh).abs().sum(0)
    bb = 2 * (M + 1) * U * dy.double().abs().sum(0)
    assert ((G.grad.double().cpu() - rec["dgamma"].double()).abs() <= bg.cpu()).all()
    assert ((Bt.grad.double().cpu() - rec["dbeta"].double()).abs() <= bb.cpu()).all()


# ------------------------------------------------------------------------------------------------ the reduce table
POISON = 31337.0
GUARD = 96


class _Dst:
    """a destination [N][stride] (+ bias [N]) inside a poisoned buffer"""
    def __init__(self, dev, N, K, stride, bias):
        self.N, self.K, self.stride, self.has_bias = N, K, stride, bias
        self.buf = torch.full((2 * GUARD + N * stride,), POISON, device=dev)
        self.view = self.buf[GUARD:GUARD + N * stride].view(N, stride)
        self.bbuf = torch.full((2 * GUARD + N,), POISON, device=dev) if bias else None
        self.zero()

    def zero(self):
        self.view[:, :self.K] = 0.0
        if self.has_bias:
            self.bbuf[GUARD:GUARD + self.N] = 0.0

    def result(self):
        w = self.view[:, :self.K]
        return torch.cat([w, self.bbuf[GUARD:GUARD + self.N, None]], dim=1) if self.has_bias else w.clone()

    def guards_intact(self):
        ok = (self.buf[:GUARD] == POISON).all() and (self.buf[GUARD + self.N * self.stride:] == POISON).all()
        ok = ok and (self.view[:, self.K:] == POISON).all()                       # the columns between row length and row stride
        if self.has_bias:
            ok = ok and (self.bbuf[:GUARD] == POISON).all() and (self.bbuf[GUARD + self.N:] == POISON).all()
        return bool(ok)


def _run_table(a3d, dev, dsts, recs, launches=1):
    """recs: [(dst index, nsplit, extra slab stride)] in append order -> per destination (result, float64 sum, sum|partials|, terms)"""
    O = a3d.ops
    g = torch.Generator().manual_seed(len(recs) * 131 + len(dsts))
    records, partials = [], []
    for di, nsplit, pad in recs:
        d = dsts[di]
        KE = d.K + (1 if d.has_bias else 0)
        count = d.N * KE
        p = (torch.randn(nsplit, count + pad, generator=g) * (1.0 + di)).to(dev)
        partials.append((di, p[:, :count]))
        records.append((p.data_ptr(), nsplit, count + pad, count, KE, d.view.data_ptr(), d.stride,
                        d.bbuf[GUARD:].data_ptr() if d.has_bias else None))
    results = []
    for _ in range(launches):
        for d in dsts:
            d.zero()
        O.reduce_table_launch(records, dev)
        torch.cuda.synchronize()
        results.append([d.result() for d in dsts])
    out = []
    for di, d in enumerate(dsts):
        KE = d.K + (1 if d.has_bias else 0)
        mine = [p for i, p in partials if i == di]
        ref = sum(p.double().sum(0) for p in mine).view(d.N, KE)
        mag = sum(p.double().abs().sum(0) for p in mine).view(d.N, KE)
        depth = max(p.shape[0] for p in mine) + len(mine)
        out.append((results[0][di], ref, depth * U * mag))
        assert d.guards_intact(), "destination %d: the guard band or the row padding was written" % di
    for k in range(1, launches):
        for x, y in zip(results[0], results[k]):
            assert torch.equal(x, y), "a second launch on re-zeroed destinations gave other bits"
    return out


def _check(out, what):
    worst = 0.0
    for di, (got, ref, bound) in enumerate(out):
        e = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
        worst = max(worst, e)
        assert torch.isfinite(got).all() and e <= 1.0, (what, di, e)
    print(f"[reduce_table] {what}: {len(out)} destinations, worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("nsplit", [1, 15, 16, 17, 333])
def test_reduce_table_one_record(a3d, dev, nsplit):
    _check(_run_table(a3d, dev, [_Dst(dev, 60, 60, 60, True)], [(0, nsplit, 0)], launches=2), "one record, nsplit %d" % nsplit)


def test_reduce_table_tied_destinations_strides_and_bias(a3d, dev):
    dsts = [_Dst(dev, 60, 60, 60, True),        # a square weight with its bias column, three records (tied over three levels)
            _Dst(dev, 7, 33, 40, False),        # a row stride wider than the row, two records
            _Dst(dev, 1, 60, 60, False),        # a vector (LayerNorm dgamma), one record with a slab stride wider than its count
            _Dst(dev, 120, 60, 180, True)]      # k | v rows of a packed in-projection: stride 180 > 60, bias, two records
    recs = [(0, 17, 0), (1, 5, 3), (2, 222, 60), (0, 16, 0), (3, 21, 0), (1, 1, 0), (0, 333, 5), (3, 4, 0)]
    _check(_run_table(a3d, dev, dsts, recs, launches=2), "tied destinations")


def test_reduce_table_many_records(a3d, dev):
    """more records than one writer launch carries (64), every third destination shared by two records"""
    dsts = [_Dst(dev, 5 + (i % 7), 9 + (i % 11), 24, i % 2 == 0) for i in range(60)]
    recs = [(i, 1 + (7 * i) % 23, i % 3) for i in range(60)] + [(i, 2 + i % 5, 0) for i in range(0, 60, 3)]
    assert len(recs) > 64
    _check(_run_table(a3d, dev, dsts, recs, launches=2), "many records")


def test_reduce_table_adds_to_what_the_destination_holds(a3d, dev):
    O = a3d.ops
    d = _Dst(dev, 12, 20, 20, False)
    p = torch.randn(9, 240, generator=torch.Generator().manual_seed(3)).to(dev)
    d.view[:, :] = 2.5
    O.reduce_table_launch([(p.data_ptr(), 9, 240, 240, 20, d.view.data_ptr(), 20, None)], dev)
    torch.cuda.synchronize()
    ref = p.double().sum(0).view(12, 20) + 2.5
    bound = (9 + 1 + 1) * U * (p.double().abs().sum(0).view(12, 20) + 2.5)
    assert ((d.result().double() - ref).abs() <= bound).all() and d.guards_intact()


# ------------------------------------------------------------------------------------------------ end to end at a small shape
E, H, NL, LEVELS, B = 60, 4, 2, 2, 2
SHAPES = {"small": (48, 129),          # the ghost-stream shape of the issue: only the LayerNorm records are two-stage
          "two-stage": (520, 515)}     # B * Lq and B * S above the 1024-row threshold: every linear's reduction is deferred too


def _module(a3d, dev):
    torch.manual_seed(11)
    mod = a3d.nn.RelativeCrossAttentionModule(E, H, NL).to(dev)      # ONE module for both levels: tied weights
    for n, p in mod.named_parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, mean=1.0 if ("norm" in n and n.endswith("weight")) else 0.0, std=0.5)
    return mod


def _inputs(dev, Lq, S):
    g = torch.Generator().manual_seed(4242)
    lv = []
    for _ in range(LEVELS):
        lv.append(dict(q=torch.randn(B, Lq, E, generator=g).to(dev), ctx=torch.randn(B, S, E, generator=g).to(dev),
                       qx=(torch.rand(B, Lq, 3, generator=g) * 2 - 0.5).to(dev), cx=(torch.rand(B, S, 3, generator=g) * 2 - 0.5).to(dev),
                       dys=[torch.randn(B, Lq, E, generator=g).to(dev) for _ in range(NL)]))
    return lv


def _forward_loss(a3d, mod, lv, ctxs):
    O = a3d.ops
    O.begin_grad_sinks()                                               # as Act3D.forward: this is where the queue is created
    loss = 0.0
    for l, c in zip(lv, ctxs):
        c = O.attach_grad_sink(c * 1.0)
        outs = mod(l["q"], c, l["qx"], l["cx"])
        loss = loss + sum((o * dy).sum() for o, dy in zip(outs, l["dys"]))
    return loss


def _step(a3d, mod, lv, defer, watch=None):
    """one forward + backward -> ({name: grad}, [context grads]); grads start from zero"""
    O = a3d.ops
    old, O.DEFER_REDUCE = O.DEFER_REDUCE, defer
    orig_add = O.ReduceQueue.add
    if watch is not None:
        def add(self, owner, partial_ptr, nsplit, slab_stride, count, row_len, dst_ptr, dst_stride, bias_ptr=None):
            flat = owner.reshape(-1)
            off = (partial_ptr - owner.data_ptr()) // 4
            idx = off + torch.arange(nsplit, device=flat.device)[:, None] * slab_stride + torch.arange(count, device=flat.device)[None]
            watch.append((dst_ptr, dst_stride, bias_ptr, row_len, nsplit, flat[idx].double().abs().sum(0)))
            return orig_add(self, owner, partial_ptr, nsplit, slab_stride, count, row_len, dst_ptr, dst_stride, bias_ptr)
        O.ReduceQueue.add = add
    try:
        for p in mod.parameters():
            p.grad = torch.zeros_like(p)
        leaves = [l["ctx"].clone().requires_grad_(True) for l in lv]
        n0 = O.ReduceQueue.flushes
        _forward_loss(a3d, mod, lv, leaves).backward()
        flushed = O.ReduceQueue.flushes - n0
        grads = {n: p.grad.detach().clone() for n, p in mod.named_parameters()}       # no synchronise, no flush call in between:
        torch.cuda.synchronize()                                                      # stream order alone must make them complete
        return grads, [x.grad.detach().clone() for x in leaves], flushed
    finally:
        O.DEFER_REDUCE = old
        O.ReduceQueue.add = orig_add


def _bounds(mod, watch):
    """{name: per-element bound tensor} from the watched records: (nsplit + records) u sum|partials| for each side, twice that for
    the difference of two orders"""
    out = {}
    for n, p in mod.named_parameters():
        g = p.grad
        lo, hi = g.data_ptr(), g.data_ptr() + 4 * g.numel()
        mag, depth, nrec = torch.zeros(g.numel(), dtype=torch.float64, device=g.device), 0, 0
        for dst, stride, bias, row_len, nsplit, s in watch:
            K = row_len - 1 if bias else row_len
            rows = s.numel() // row_len
            s = s.view(rows, row_len)
            hit = False
            if lo <= dst < hi:
                assert stride == K or rows == 1
                o = (dst - lo) // 4
                mag[o:o + rows * K] += s[:, :K].reshape(-1)
                hit = True
            if bias and lo <= bias < hi:
                o = (bias - lo) // 4
                mag[o:o + rows] += s[:, K]
                hit = True
            if hit:
                depth, nrec = max(depth, nsplit), nrec + 1
        if nrec:
            out[n] = (2 * (depth + nrec) * U * mag).view_as(g)
    return out


@pytest.fixture(scope="module")
def e2e(a3d, dev):
    """per shape: the module, its inputs, the step with the queue off (once) and on (with the watched records)"""
    res = {}
    for name, (Lq, S) in SHAPES.items():
        mod, lv = _module(a3d, dev), _inputs(dev, Lq, S)
        off = _step(a3d, mod, lv, False)
        watch = []
        on = _step(a3d, mod, lv, True, watch)
        res[name] = dict(mod=mod, lv=lv, off=off, on=on, bounds=_bounds(mod, watch), nrec=len(watch))
    return res


@pytest.mark.parametrize("shape", list(SHAPES))
def test_end_to_end_queue_on_equals_queue_off(e2e, shape):
    r = e2e[shape]
    (g_on, c_on, flushed), (g_off, c_off, flushed_off) = r["on"], r["off"]
    assert flushed == 1 and flushed_off == 0, "one table launch per backward with the queue on, none with it off"
    owned = r["bounds"]
    print(f"[e2e {shape}] {r['nrec']} deferred records, parameters with deferred reductions: {sorted(owned)}")
    assert any("norm" in n for n in owned), "the LayerNorm gradients were not deferred"
    if shape == "two-stage":
        assert set(owned) == set(g_on), "at two-stage row counts every ghost-stream parameter's reduction is deferred"
    for x, y in zip(c_on, c_off):                                    # activations' gradients: no reduction order is involved
        assert torch.equal(x, y)
    for n in g_on:
        assert torch.isfinite(g_on[n]).all()
        if n in owned:
            e = ((g_on[n].double() - g_off[n].double()).abs() / owned[n].clamp_min(1e-300)).max().item()
            print(f"[e2e {shape}] {n}: on / off err / bound = {e:.3f}")
            assert e <= 1.0, (n, e)
        else:
            # one-stage kernels, the same launches either way; at these row counts each address has one adder per launch, or two
            # onto a zeroed buffer (commutative): the same bits
            assert torch.equal(g_on[n], g_off[n]), n


@pytest.mark.parametrize("shape", list(SHAPES))
def test_end_to_end_two_passes_give_identical_bits(a3d, e2e, shape):
    r = e2e[shape]
    again = _step(a3d, r["mod"], r["lv"], True)
    for n in r["bounds"]:
        assert torch.equal(again[0][n], r["on"][0][n]), n


def test_split_backward_flushes_before_the_hot_path_callback(a3d, dev, e2e):
    O, r = a3d.ops, e2e["two-stage"]
    mod, lv = r["mod"], r["lv"]
    w = torch.nn.Parameter(torch.ones(E, device=dev))                  # stands for the FPN: the tokens depend on it
    for p in mod.parameters():
        p.grad = torch.zeros_like(p)
    seen = {}

    def on_hot_done():
        seen["flushes"] = O.ReduceQueue.flushes
        seen["grads"] = {n: p.grad.detach().clone() for n, p in mod.named_parameters()}

    n0 = O.ReduceQueue.flushes
    a3d.engine._split_backward([l["ctx"] * w for l in lv], lambda leaves: _forward_loss(a3d, mod, lv, leaves), on_hot_done)
    torch.cuda.synchronize()
    assert seen["flushes"] == n0 + 1 and O.ReduceQueue.flushes == n0 + 1
    assert w.grad is not None and torch.isfinite(w.grad).all()
    for n, p in mod.named_parameters():
        assert torch.equal(seen["grads"][n], p.grad), n                # complete at the boundary, untouched by the late stage
        if n in r["bounds"]:
            assert torch.equal(p.grad, r["on"][0][n]), n               # and the bits of the plain backward()


def test_graph_replay_equals_eager(a3d, dev, e2e):
    r = e2e["small"]
    mod, lv = r["mod"], r["lv"]
    leaves = [l["ctx"].clone().requires_grad_(True) for l in lv]

    def step():
        for p in mod.parameters():
            p.grad.zero_()
        for x in leaves:
            if x.grad is not None:
                x.grad.zero_()
        _forward_loss(a3d, mod, lv, leaves).backward()

    for p in mod.parameters():
        p.grad = torch.zeros_like(p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for p in mod.parameters():
        p.grad.fill_(float("nan"))                                     # whatever the capture left: the replay must rebuild it
    graph.replay()
    torch.cuda.synchronize()
    for n, p in mod.named_parameters():
        assert torch.equal(p.grad, r["on"][0][n]), n
