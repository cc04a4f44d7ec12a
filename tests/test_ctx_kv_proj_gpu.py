"""a3d_ctx_kv_proj16 (csrc/ctx_proj.hip: the k | v operand rows of one or two attention layers from ONE pass over the context) against
the float64 reference and the DERIVED per-element bounds of tests/rope_ref.py -- the bounds tests/test_rope_operands_gpu.py holds
a3d_proj_rope_split16 to -- called through lib.py's ctypes binding.  No tolerance is chosen here: the criterion is
max(err / bound) <= 1 on every output of every layer plus zero format violations (rope_ref.format_violations: |lo| <= ulp(hi) / 2, pad
rows zero in channels 0-14, channel 15 of the K hi part 0 and of the V hi part 1.0 on every row below Npad, lo pads zero, all finite).

Cases (E = 60, H = 4): N = 1, 15, 16, 17, 63, 64, 65, 200, 4097 with B = 2, each with Npad = ceil64(N) and ceil64(N) + 128; B = 3 with
N = 130; more workgroup splits than 16-key groups (workgroups without a key); xyz NULL; |theta| >= 200 on half of the keys (the
double-precision reduction of fast_sincos on the device); W / bias 4-byte aligned only; ldx = 2 E; bias NULL; X spanning 2^-30 .. 2^15
with an identity W_v (bit-exact against the format conversion restated in torch; fp16-subnormal hi and lo parts asserted to occur).
Every case runs nl = 2 with different weights per layer and checks: a poisoned guard band on both sides of every output buffer is
untouched; a second launch is bit-identical; layer 0 equals an nl = 1 call with the same weights bit for bit; X carries NaN in rows
beyond the last sample (and, with ldx > E, in the columns outside E) and no NaN reaches an output.  The number of elements whose bits
differ from a3d_proj_rope_split16's on the same inputs is printed as a [parity] line (the k-steps of the contraction are summed in
another order, so bit equality is not asserted).
"""
import pytest
import torch

import rope_ref as R
from test_rope_operands_gpu import _Guarded, _same_bits

pytestmark = pytest.mark.gpu
F64, F32, F16 = torch.float64, torch.float32, torch.float16
E, H = 60, 4
NAN_ROWS = 64


def _case(name, B=2, N=200, pad=0, nsplit=0, xyz="unit", walign=True, ld=1, bias=True, vals="randn"):
    return R.SimpleNamespace(name=name, B=B, N=N, pad=pad, nsplit=nsplit, xyz=xyz, walign=walign, ld=ld, bias=bias, vals=vals)


CASES = [_case(f"n{n}_pad{pad}", N=n, pad=pad) for n in (1, 15, 16, 17, 63, 64, 65, 200, 4097) for pad in (0, 128)] + [
    _case("b3_n130", B=3, N=130),
    _case("more_splits_than_groups", N=65, nsplit=64),            # Npad / 16 = 8 groups
    _case("no_xyz", N=130, xyz=None),
    _case("big_theta", N=130, xyz="big"),
    _case("unaligned_w", N=130, walign=False),
    _case("ldx_2e", N=130, ld=2),
    _case("no_bias", N=130, bias=False),
    _case("sweep_identity_wv", N=130, vals="sweep", pad=128),
]


def _build(c):
    g = torch.Generator().manual_seed(9100 + 13 * [k.name for k in CASES].index(c.name))
    B, N = c.B, c.N
    x = R.SimpleNamespace(case=c, B=B, N=N, Npad=R.pad_to(N, 64) + c.pad, freq=R.freq32(E))
    x.ldx = E * c.ld
    x.xoff = x.ldx - E
    x.Xbuf = torch.full((B * N + NAN_ROWS, x.ldx), float("nan"), dtype=F32)
    x.X = R._values(g, (B, N, E), c.vals)
    x.Xbuf[:B * N, x.xoff:] = x.X.view(B * N, E)
    x.xyz = R._xyz(g, c.xyz, B, N)
    # parameter buffer: per layer W_k | W_v [2E][E] then bias [2E]; 4-byte aligned only when asked
    x.wshift = 0 if c.walign else 1
    per = 2 * E * E + 2 * E
    x.Pbuf = torch.zeros(x.wshift + 2 * per + 3)
    x.W, x.bias, x.woff, x.boff = [], [], [], []
    for l in range(2):
        wo = x.wshift + l * per
        bo = wo + 2 * E * E
        W = x.Pbuf[wo:wo + 2 * E * E].view(2 * E, E)
        W.copy_(torch.randn(2 * E, E, generator=g) * E ** -0.5)
        b = x.Pbuf[bo:bo + 2 * E]
        b.copy_(torch.randn(2 * E, generator=g))
        if c.vals == "sweep":
            W.mul_(0.25)                                   # |y| stays inside fp16's range for |x| up to 2^15
            if l == 0:
                W[E:].copy_(torch.eye(E))                  # layer 0's value block: a pure format conversion
        has_b = c.bias and not (c.vals == "sweep" and l == 0)
        x.W.append(W)
        x.bias.append(b if has_b else None)
        x.woff.append(wo)
        x.boff.append(bo)
    return x


def _launch(a3d, dev, x, d, nl, old=False):
    """One a3d_ctx_kv_proj16 launch (or, old=True, one a3d_proj_rope_split16 k | v launch per layer) into fresh poisoned buffers ->
    [(K rows, V rows)] CPU tensors per layer."""
    L = a3d.lib
    c = x.case
    B, N, Npad = x.B, x.N, x.Npad
    bufs = [(_Guarded((B, H, Npad, 32), F16, dev), _Guarded((B, H, Npad, 32), F16, dev)) for _ in range(nl)]
    X = d.Xbuf.data_ptr() + 4 * x.xoff
    xp = None if d.xyz is None else d.xyz.data_ptr()
    wp = lambda l: d.Pbuf.data_ptr() + 4 * x.woff[l]
    bp = lambda l: None if x.bias[l] is None else d.Pbuf.data_ptr() + 4 * x.boff[l]
    st = L.stream()
    if old:
        for l in range(nl):
            L.call("a3d_proj_rope_split16", X, x.ldx, wp(l), E, bp(l), E, xp, 1.0, bufs[l][0].ptr(), None, 2, None, 1.0, bufs[l][1].ptr(),
                   None, 2 | 8, d.freq.data_ptr(), B, N, Npad, E, H, st)
    else:
        args = []
        for l in range(2):
            args += [wp(l), bp(l), bufs[l][0].ptr(), bufs[l][1].ptr()] if l < nl else [None, None, None, None]
        L.call("a3d_ctx_kv_proj16", X, x.ldx, xp, *args, E, d.freq.data_ptr(), nl, B, N, Npad, E, H, c.nsplit, st)
    torch.cuda.synchronize()
    for kb, vb in bufs:
        assert kb.guards_intact() and vb.guards_intact(), f"{c.name}: bytes outside an output tensor were written"
    return [(kb.t.cpu(), vb.t.cpu()) for kb, vb in bufs]


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_ctx_kv_rows_within_the_derived_bounds(a3d, dev, name):
    c = next(k for k in CASES if k.name == name)
    x = _build(c)
    d = R.SimpleNamespace(Xbuf=x.Xbuf.to(dev), Pbuf=x.Pbuf.to(dev), freq=x.freq.to(dev), xyz=None if x.xyz is None else x.xyz.to(dev))
    assert d.Xbuf.data_ptr() % 16 == 0 and d.Pbuf.data_ptr() % 16 == 0
    outs = _launch(a3d, dev, x, d, 2)
    again = _launch(a3d, dev, x, d, 2)
    one = _launch(a3d, dev, x, d, 1)
    prev = _launch(a3d, dev, x, d, 2, old=True)
    differ = total = 0
    for l in range(2):
        for what, j, xyz, parts in (("K", 0, x.xyz, 2), ("V", 1, None, 2 | 8)):
            tag = f"{name} layer {l} {what}"
            rows = outs[l][j]
            ref = R.forward(X=x.X, W=x.W[l][j * E:(j + 1) * E], b=None if x.bias[l] is None else x.bias[l][j * E:(j + 1) * E],
                            xyz=xyz, freq=x.freq, scale=1.0)
            xs = R.SimpleNamespace(case=R.SimpleNamespace(entry="split16", blocks=[R.blk(parts=parts)]), N=x.N, H=H)
            r, bad = R.evaluate(xs, 0, dict(rows=rows, planes=None), ref)
            big = 0 if ref.theta is None else int((ref.theta.abs() >= 200).sum())
            print(f"[parity] ctx kv rows {tag}: max(err/bound)={r:.3f}" + (f" ({big} angles >= 200)" if big else ""))
            assert bad == [], (tag, bad)
            assert r <= 1.0, (tag, r)
            assert _same_bits(rows, again[l][j]), f"{tag}: rows differ between two launches"
            a, b = rows.view(torch.int16), prev[l][j].view(torch.int16)
            differ += int((a != b).sum())
            total += a.numel()
    for j, what in ((0, "K"), (1, "V")):
        assert _same_bits(outs[0][j], one[0][j]), f"{name}: layer 0 {what} rows of the nl = 2 call differ from the nl = 1 call"
    print(f"[parity] ctx kv rows {name}: {differ} of {total} elements differ in bits from a3d_proj_rope_split16")
    if c.vals == "sweep":
        # layer 0's value block is X itself: the format conversion restated in torch, bit for bit
        assert torch.equal(x.X.to(F64).to(F32), x.X)
        want = R.encode16(x.X, H, x.Npad, True)
        assert _same_bits(outs[0][1], want), f"{name}: identity value rows differ from the format conversion restated in torch"
        v = outs[0][1][:, :, :x.N].float()
        hi, lo = v[..., :15].abs(), v[..., 16:31].abs()
        assert ((hi > 0) & (hi < 2.0 ** -14)).any() and ((lo > 0) & (lo < 2.0 ** -14)).any(), "no fp16-subnormal parts in the sweep"
