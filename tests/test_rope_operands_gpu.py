"""The RoPE / projection operand writers and the gradient merge (csrc/rope.hip; a3d_rope_rows_f32 of csrc/denoise.hip) against the
float64 reference and the DERIVED bounds of tests/rope_ref.py (fair and with teeth: tests/test_rope_operands_cpu.py), called through
lib.py's ctypes binding.  No tolerance is chosen here.

Case table (tests/rope_ref.py CASES; prefix = entry point).  proj_rope_split_kernel<NT, EC, KEQ> instances are named in the case:
  s16_*  a3d_rope_split16 (rope_split_kernel, fmt16)        E = 60 / 120 / 30 / 90; N = 1, 63, 64, 65, 130, 1025, 4097; B = 70;
         Npad = ceil64(N) + 128; ldy = E, 2E, 3E; rows only / planes only / both; parts 1, 2, 2|4, 2|8, 2|4|8; xyz NULL, [-0.5, 1.5],
         signed zeros, |theta| >= 200 (s16_big_theta_e60: the double-precision reduction of fast_sincos ON THE DEVICE); the 2^-30 .. 2^15
         sweep unrotated (bit-exact, fp16 subnormal hi and lo parts) and rotated
  p16_*  a3d_proj_rope_split16: p16_4_60_keq_* <4,60,true>; p16_4_60_k12 / k256 <4,60,false>; p16_8_120_keq_* <8,120,true>;
         p16_8_120_k64 / k256 <8,120,false>; p16_4_0_e30_* <4,0,false>; p16_8_0_e90_* <8,0,false>.  Two output blocks with different
         xyz / scale / parts (the qk and kv packings of ops.attn_operands_fused16), W / bias 4-byte aligned only (*_unaligned_w and
         others), ldx = 2K, no bias, B = 70, K = 12 / 64 / 256, identity W on the sweep (bit-exact through the MFMA chain), |theta| >= 200
  sb_* / pb_*  the bf16 family: a3d_rope_split (rows 48 / 32 + planes), a3d_rope_split_qk, a3d_split_vt, a3d_proj_rope_split
         (<4,60,true>, <8,120,false>, <4,0,false>, <8,0,false>)
  rf_*   a3d_rope_rows_f32 (N = Npad = 1 as the single-query block calls it, Npad = N + 7, fp32 copy, |theta| >= 200)
  m_*    a3d_rope_merge_bwd: nsplit 1 / 3 / 16, ldy = E, 2E, 3E, no rotation, B = 70, N = 4097, |theta| >= 200: rope_merge_bwd_kernel
         in-process; the E = 60 / 120 cases again under A3D_ROPE_MERGE_ROWS=1 (rope_merge_bwd_rows_kernel<60 / 120>) and
         A3D_ROPE_MERGE_PAIRS=1 (rope_merge_bwd_pairs_kernel<60 / 120>), each in ONE fresh child process (the switch is a static)

Every case: (1) the exact cases (no rotation, power-of-two scale, no or an identity projection) equal the format conversion restated
in torch bit for bit; (2) every case is within the derived bound ([parity] lines); (3) the format invariants of
rope_ref.format_violations -- |lo| <= ulp(hi) / 2, pad rows zero in channels 0-14, channel 15 of the hi part exactly 1.0 on EVERY row
below Npad where the flag asks for it and 0 otherwise (the convention of write_operand_formats16, stated in include/act3d_hip.h),
rows and planes of one call carry the same bits -- and a poisoned guard band round every output buffer is untouched; (4) the merge
is handed dR with NaN in rows >= N and in channel 15 and dY with poison in columns outside its E; (6) a second launch gives the
same bits.  (5) the seam: device-written operands through ops.attn_core_fwd / attn_core_bwd against attn16_core_ref's bounds on the
values they carry, then a3d_rope_merge_bwd on the core's dQ partials / dK against the merge reference.  (7) the argument checks
need no device: tests/test_host_cpu.py.
"""
import os
import subprocess
import sys

import pytest
import torch

import attn16_core_ref as C
import rope_ref as R

pytestmark = pytest.mark.gpu
F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
GUARD = 64                 # elements of poison on either side of every output buffer (a multiple of 16 bytes for every dtype used)
POISON = 0xA5


class _Guarded:
    """A device buffer of `shape` inside a poisoned allocation."""
    def __init__(self, shape, dtype, dev):
        n = 1
        for s in shape:
            n *= s
        self.full = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.full.view(torch.uint8).fill_(POISON)
        self.t = self.full[GUARD:GUARD + n].view(*shape)
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        b = self.full.view(torch.uint8)
        w = self.full.element_size()
        return bool((b[:GUARD * w] == POISON).all() and (b[(GUARD + self.n) * w:] == POISON).all())


def _poisoned(t):
    return (t.contiguous().view(torch.uint8) == POISON).all().item()


def _dev_inputs(x, dev):
    d = R.SimpleNamespace(freq=x.freq.to(dev), xyz=[None if t is None else t.contiguous().to(dev) for t in x.xyz])
    c = x.case
    if c.entry == "merge":
        d.dR = x.dR.to(dev)
    elif c.K is not None:
        d.Xbuf, d.Pbuf = x.Xbuf.to(dev), x.Pbuf.to(dev)
        assert d.Xbuf.data_ptr() % 16 == 0 and d.Pbuf.data_ptr() % 16 == 0
    else:
        d.Ybuf = x.Ybuf.to(dev)
    return d


def _launch(a3d, dev, x, d):
    """One launch of the case's entry point into fresh poisoned buffers -> per block {"rows", "planes"} CPU tensors (merge: the dY buffer)."""
    L = a3d.lib
    c = x.case
    B, N, Npad, E, H = x.B, x.N, x.Npad, x.E, x.H
    st = L.stream()
    fp = d.freq.data_ptr()
    xp = [None if t is None else t.data_ptr() for t in d.xyz]
    if c.entry == "merge":
        dY = _Guarded((B, N, x.ldy), F32, dev)
        L.call("a3d_rope_merge_bwd", d.dR.data_ptr(), c.ns, xp[0], fp, c.blocks[0].scale, dY.ptr() + 4 * x.off, x.ldy, B, N, Npad, E, H, st)
        torch.cuda.synchronize()
        assert dY.guards_intact(), c.name
        return dY.t.cpu()
    fp16 = c.entry in R.FP16_ENTRIES
    dt = F16 if fp16 else BF16
    bufs = []
    for b_ in c.blocks:
        if c.entry == "rows_f32":
            bufs.append((_Guarded((B, H, Npad, 16), F32, dev), None))
            continue
        rows = _Guarded((B, H, Npad, 32 if fp16 else b_.width), dt, dev) if b_.rows else None
        planes = _Guarded((B, H, (b_.parts & 3) if fp16 else 2, 16, Npad), dt, dev) if b_.planes else None
        bufs.append((rows, planes))
    p = lambda g: None if g is None else g.ptr()
    b0 = c.blocks[0]
    if c.entry in ("split16", "split", "split_qk", "split_vt", "rows_f32"):
        Y = d.Ybuf.data_ptr() + 4 * x.off
        r0, p0 = bufs[0]
        if c.entry == "split16":
            L.call("a3d_rope_split16", Y, x.ldy, xp[0], fp, b0.scale, p(r0), p(p0), b0.parts, B, N, Npad, E, H, st)
        elif c.entry == "split":
            L.call("a3d_rope_split", Y, x.ldy, xp[0], fp, b0.scale, p(r0), b0.width, p(p0), B, N, Npad, E, H, st)
        elif c.entry == "split_qk":
            assert b0.width == 48 and p0 is None
            L.call("a3d_rope_split_qk", Y, x.ldy, xp[0], fp, b0.scale, p(r0), B, N, Npad, E, H, st)
        elif c.entry == "split_vt":
            assert r0 is None and b0.xyz is None and b0.scale == 1.0
            L.call("a3d_split_vt", Y, x.ldy, p(p0), B, N, Npad, E, H, st)
        else:
            L.call("a3d_rope_rows_f32", Y, x.ldy, xp[0], fp, b0.scale, p(r0), B, N, Npad, E, H, st)
    else:
        X = d.Xbuf.data_ptr() + 4 * x.xoff
        W = d.Pbuf.data_ptr() + 4 * x.wshift
        bias = None if x.bias is None else d.Pbuf.data_ptr() + 4 * x.boff
        blocks = []
        for j in range(2):
            if j < x.nb:
                b_, (r_, p_) = c.blocks[j], bufs[j]
                blocks.append((xp[j], b_.scale, p(r_), p(p_), b_.parts) if fp16 else (xp[j], b_.scale, p(r_), b_.width, p(p_)))
            else:
                blocks.append((None, 1.0, None, None, 1) if fp16 else (None, 1.0, None, 32, None))
        L.call("a3d_proj_rope_split16" if fp16 else "a3d_proj_rope_split", X, x.ldx, W, x.K, bias, x.K, *blocks[0], *blocks[1], fp,
               B, N, Npad, E, H, st)
    torch.cuda.synchronize()
    outs = []
    for r_, p_ in bufs:
        for g in (r_, p_):
            assert g is None or g.guards_intact(), f"{c.name}: bytes outside an output tensor were written"
        outs.append(dict(rows=None if r_ is None else r_.t.cpu(), planes=None if p_ is None else p_.t.cpu()))
    return outs


def _same_bits(a, b):
    if a is None:
        return b is None
    return torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                       b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def _check_merge(x, dYbuf, tag):
    c = x.case
    ref = R.merge(x.dR, x.N, x.xyz[0], x.freq, c.blocks[0].scale)
    got = dYbuf[..., x.off:x.off + x.E]
    assert x.off == 0 or _poisoned(dYbuf[..., :x.off]), f"{tag}: columns of dY outside [0, E) were written"
    assert torch.isfinite(got).all(), f"{tag}: dR rows >= N or channel 15 (NaN) reached dY"
    r = R.ratio(got.to(F64) - ref.val, ref.bound)
    print(f"[parity] rope merge {tag} nsplit={c.ns} ldy={x.ldy}: max(err/bound)={r:.3f} (max_abs_err {(got.to(F64) - ref.val).abs().max():.2e} "
          f"of {ref.val.abs().max():.2e})")
    return r


FWD_CASES = [c.name for c in R.CASES if c.entry != "merge"]
MERGE_CASES = [c.name for c in R.CASES if c.entry == "merge"]


@pytest.mark.parametrize("name", FWD_CASES)
def test_writers_within_the_derived_bounds(a3d, dev, name):
    x = R.build(name)
    c = x.case
    d = _dev_inputs(x, dev)
    outs = _launch(a3d, dev, x, d)
    again = _launch(a3d, dev, x, d)
    for j, b_ in enumerate(c.blocks):
        tag = f"{name} block {j}" + (" <%d,%d,%s>" % R.proj_instance(c) if c.K else "")
        ref = R.forward(**R.block_inputs(x, j))
        r, bad = R.evaluate(x, j, outs[j], ref)
        big = 0 if ref.theta is None else int((ref.theta.abs() >= 200).sum())
        print(f"[parity] rope writer {tag}: max(err/bound)={r:.3f}" + (f" ({big} angles >= 200)" if big else ""))
        assert bad == [], (tag, bad)
        assert r <= 1.0, (tag, r)
        if R.is_exact(x, j):
            T = ref.val.to(F32)
            assert torch.equal(T.to(F64), ref.val)
            want = R.expected_outputs(x, j, T)
            for k in ("rows", "planes"):
                assert _same_bits(outs[j][k], want[k]), f"{tag}: {k} differ from the format conversion restated in torch"
        for k in ("rows", "planes"):
            assert _same_bits(outs[j][k], again[j][k]), f"{tag}: {k} differ between two launches"


@pytest.mark.parametrize("name", MERGE_CASES)
def test_merge_within_the_derived_bound(a3d, dev, name):
    x = R.build(name)
    d = _dev_inputs(x, dev)
    dY = _launch(a3d, dev, x, d)
    r = _check_merge(x, dY, f"{name} default kernel")
    assert r <= 1.0, (name, r)
    assert _same_bits(dY, _launch(a3d, dev, x, d)), f"{name}: dY differs between two launches"
    # large finite values where the NaNs were: still ignored
    d.dR = torch.nan_to_num(d.dR, nan=3e38)
    assert _same_bits(dY, _launch(a3d, dev, x, d)), f"{name}: dR rows >= N or channel 15 change dY"


def _merge_child():
    """Body of the child process: the E = 60 / 120 merge cases under whatever A3D_ROPE_MERGE_* switch the environment holds."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import importlib
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    worst = 0.0
    for name in R.MERGE_OPT_IN_CASES:
        x = R.build(name)
        d = _dev_inputs(x, dev)
        dY = _launch(a3d, dev, x, d)
        r = _check_merge(x, dY, f"{name} {sys.argv[2]}")
        assert _same_bits(dY, _launch(a3d, dev, x, d)), f"{name}: dY differs between two launches"
        worst = max(worst, r)
    assert worst <= 1.0, worst
    print(f"merge-child ok {len(R.MERGE_OPT_IN_CASES)} cases worst {worst:.3f}")


@pytest.mark.parametrize("switch", ["A3D_ROPE_MERGE_ROWS", "A3D_ROPE_MERGE_PAIRS"])
def test_opt_in_merge_kernels_in_a_fresh_process(dev, switch):
    """rope_merge_bwd_rows_kernel<60 / 120> and rope_merge_bwd_pairs_kernel<60 / 120>: the switch is read once into a static, so each
    runs in a process of its own (started fresh, one at a time)."""
    env = dict(os.environ)
    env.pop("A3D_ROPE_MERGE_ROWS", None)
    env.pop("A3D_ROPE_MERGE_PAIRS", None)
    env[switch] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "merge-child", switch], env=env, capture_output=True, text=True,
                       timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"merge-child ok {len(R.MERGE_OPT_IN_CASES)} cases" in p.stdout


# ------------------------------------------------------------------------------------------------ the seam
SEAM = [  # name, B, H, Lq, S, nsplit, masked, value planes in the forward
    ("seam_q37_s131", 2, 4, 37, 131, 1, False, False),
    ("seam_q70_s300_ns3_masked", 2, 4, 70, 300, 3, True, False),
    ("seam_q65_s1025_ns2_planes", 1, 8, 65, 1025, 2, False, True),
    ("seam_q130_s131_ns2_masked_planes", 2, 4, 130, 131, 2, True, True),
]


@pytest.mark.parametrize("name,B,H,Lq,S,ns,masked,planes", SEAM, ids=[s[0] for s in SEAM])
def test_seam_device_written_operands_through_the_core_and_back(a3d, dev, name, B, H, Lq, S, ns, masked, planes):
    """Y -> a3d_rope_split16 -> ops.attn_core_fwd / attn_core_bwd -> a3d_rope_merge_bwd -> dY, every link against float64: the operands
    against the writer bound, the core against attn16_core_ref.bounds on the values the DEVICE-WRITTEN operands carry (the product's
    pad / ones convention: 1.0 in channel 15 of every value row below Sp), the merge against the merge reference on the core's own
    gradients."""
    O_, L = a3d.ops, a3d.lib
    E = 15 * H
    g = torch.Generator().manual_seed(len(name) * 7 + S)
    Lqp, Sp = C.pad_to(Lq, 64), C.pad_to(S, 64)
    Yq, Yk, Yv = torch.randn(B, Lq, E, generator=g), torch.randn(B, S, E, generator=g), torch.randn(B, S, E, generator=g)
    qx, kx = torch.rand(B, Lq, 3, generator=g) * 2 - 0.5, torch.rand(B, S, 3, generator=g) * 2 - 0.5
    dO = torch.randn(B, H, Lq, 15, generator=g, dtype=F64).to(F32).to(F64)
    kmask = None
    if masked:
        kmask = torch.rand(B, S, generator=g) < 0.3
        kmask[:, 0] = False
        kmask[B - 1, S - S // 3:] = True                                   # a ragged tail
    freq = O_.rope_freq(E, dev)
    fr = freq.cpu()
    st = L.stream()
    dY = [t.to(dev) for t in (Yq, Yk, Yv)]
    dqx, dkx = qx.to(dev), kx.to(dev)
    Qr, Kr, Vr = (_Guarded((B, H, n, 32), F16, dev) for n in (Lqp, Sp, Sp))
    Vp = _Guarded((B, H, 2, 16, Sp), F16, dev) if planes else None
    L.call("a3d_rope_split16", dY[0].data_ptr(), E, dqx.data_ptr(), freq.data_ptr(), R.SC, Qr.ptr(), None, 2, B, Lq, Lqp, E, H, st)
    L.call("a3d_rope_split16", dY[1].data_ptr(), E, dkx.data_ptr(), freq.data_ptr(), 1.0, Kr.ptr(), None, 2, B, S, Sp, E, H, st)
    L.call("a3d_rope_split16", dY[2].data_ptr(), E, None, freq.data_ptr(), 1.0, Vr.ptr(), None if Vp is None else Vp.ptr(),
           2 | 8 | (4 if planes else 0), B, S, Sp, E, H, st)
    torch.cuda.synchronize()
    assert all(t is None or t.guards_intact() for t in (Qr, Kr, Vr, Vp))
    # link 1: the operands
    for what, buf, n, Y, xyz, sc, parts in (("q", Qr, Lq, Yq, qx, R.SC, 2), ("k", Kr, S, Yk, kx, 1.0, 2),
                                           ("v", Vr, S, Yv, None, 1.0, 2 | 8 | (4 if planes else 0))):
        ref = R.forward(Y=Y, xyz=xyz, freq=fr, scale=sc)
        xs = R.SimpleNamespace(case=R.SimpleNamespace(entry="split16", blocks=[R.blk(parts=parts)]), N=n, H=H)
        r, bad = R.evaluate(xs, 0, dict(rows=buf.t.cpu(), planes=Vp.t.cpu() if (what == "v" and planes) else None), ref)
        print(f"[parity] seam {name}: {what} operands max(err/bound)={r:.3f}")
        assert bad == [] and r <= 1.0, (name, what, r, bad)
    # link 2: the core on what the operands carry
    q, k, v = C.carried(Qr.t.cpu(), Lq), C.carried(Kr.t.cpu(), S), C.carried(Vr.t.cpu(), S)
    ref = C.reference(q, k, v, kmask, dO)
    b = C.bounds(ref, q, k, v, kmask, dO)
    km = None if kmask is None else kmask.to(torch.uint8).to(dev)
    old = O_.ATTN_MODE
    O_.ATTN_MODE = "f16"
    try:
        O, LSE = O_.attn_core_fwd(Qr.t, Kr.t, Vp.t if planes else Vr.t, km, B, H, Lq, Lqp, S, Sp, ns, nograd=False)
    finally:
        O_.ATTN_MODE = old
    dQp, dK, dV = O_.attn_core_bwd(Qr.t, Kr.t, Vr.t, km, O, C.to_kernel_layout(dO).float().to(dev), LSE, B, H, Lq, Lqp, S, Sp, ns,
                                   extra=(None, None, Vr.t))
    torch.cuda.synchronize()
    Og = C.from_kernel_layout(O.double().cpu(), H)
    Lg = LSE[:, :, :Lq].double().cpu()
    assert torch.isfinite(Og).all() and torch.isfinite(Lg).all()
    ro, rl = C.ratio(Og - ref.O, b.O), C.ratio(Lg - ref.LSE2, b.LSE2)
    dQ = dQp.double().cpu().sum(0)[:, :, :Lq, :15]
    dKc, dVc = dK.double().cpu(), dV.double().cpu()
    assert (dKc[:, :, S:] == 0).all() and (dVc[:, :, S:] == 0).all() and (dKc[..., 15] == 0).all() and (dVc[..., 15] == 0).all()
    rq = C.ratio(dQ - ref.dQ, b.dQ)
    rk = C.ratio(dKc[:, :, :S, :15] - ref.dK, b.dK + b.dK_dropped)
    rv = C.ratio(dVc[:, :, :S, :15] - ref.dV, b.dV + b.dV_dropped)
    print(f"[parity] seam {name} VR={0 if planes else 1} nsplit={ns}{' masked' if masked else ''}: core on device-written operands "
          f"max(err/bound) O={ro:.3f} LSE2={rl:.3f} dQ={rq:.3f} dK={rk:.3f} dV={rv:.3f}")
    assert max(ro, rl, rq, rk, rv) <= 1.0, (name, ro, rl, rq, rk, rv)
    # link 3: the merge on the core's own gradients (rows of dQp beyond the last 16-query tile are never written: not read either)
    for what, dR, nsp, n, npad, xyz, dxyz, sc in (("dYq", dQp, ns, Lq, Lqp, qx, dqx, R.SC), ("dYk", dK.unsqueeze(0), 1, S, Sp, kx, dkx, 1.0),
                                                ("dYv", dV.unsqueeze(0), 1, S, Sp, None, None, 1.0)):
        out = _Guarded((B, n, E), F32, dev)
        L.call("a3d_rope_merge_bwd", dR.data_ptr(), nsp, None if dxyz is None else dxyz.data_ptr(), freq.data_ptr(), sc, out.ptr(), E,
               B, n, npad, E, H, st)
        torch.cuda.synchronize()
        assert out.guards_intact()
        mref = R.merge(dR.cpu(), n, xyz, fr, sc)
        rm = R.ratio(out.t.cpu().to(F64) - mref.val, mref.bound)
        print(f"[parity] seam {name}: merge {what} max(err/bound)={rm:.3f}")
        assert rm <= 1.0, (name, what, rm)


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "merge-child":
    _merge_child()
