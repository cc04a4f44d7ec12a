"""The float64 reference and the derived bounds of tests/rope_ref.py are right, fair and have teeth -- no GPU.

 * CONVENTION: the reference's rotation equals the oracle's rotary code (oracle/blocks.py rope3d_code + rotary_apply, which restates
   the reference project's and is what its golden files rotate) and a hand-derived known answer (axis order, rotation sense);
   forward and merge are each other's transpose (adjoint identity in float64).
 * FAIR: for every case of tests/test_rope_operands_gpu.py (same table, same seeds) an fp32 CPU emulation of the writers -- sin / cos
   from the library's host mirror a3d_sincos_host, the rotation evaluated uncontracted and with either product fused -- passes every
   bound and every format invariant, and reproduces the format conversion of the exact cases bit for bit.
 * TEETH: emulated defects each fail the check they target.
 * the case table hits what its names claim.
"""
import math

import numpy as np
import pytest
import torch

import rope_ref as R
from conftest import load_pkg

F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def sincos():
    """sin / cos of an fp32 tensor through the host mirror of the device's fast_sincos."""
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()

    def f(th):
        x = np.ascontiguousarray(th.detach().numpy().astype(np.float32))
        sn, cs = np.empty_like(x), np.empty_like(x)
        lib.a3d_sincos_host(x.ctypes.data, sn.ctypes.data, cs.ctypes.data, x.size)
        return torch.from_numpy(sn), torch.from_numpy(cs)
    return f


# ------------------------------------------------------------------------------------------------ conventions
@pytest.mark.parametrize("E", [30, 60, 120])
def test_reference_rotation_equals_the_oracle_rotary_code(E):
    from oracle import blocks as OB
    g = torch.Generator().manual_seed(E)
    y = torch.randn(2, 7, E, generator=g)
    xyz = torch.rand(2, 7, 3, generator=g) * 2 - 0.5
    cos, sin = OB.rope3d_code(xyz, E)
    want = OB.rotary_apply(y, cos.to(y.dtype), sin.to(y.dtype)).to(F64)
    got = R.forward(Y=y, xyz=xyz, freq=R.freq32(E)).val
    assert (got - want).abs().max().item() <= 4e-6 * want.abs().max().item()          # the oracle evaluates in fp32
    assert torch.equal(R.freq32(E), torch.exp(torch.arange(0, E // 3, 2, dtype=F32) * (-math.log(10000.0) / (E // 3))))


def test_reference_known_answer_pins_axis_order_and_rotation_sense():
    """One row, E = 30 (third = 10, five pairs per axis, freq[k] = 1e4^(-2k / 10)), one non-zero pair per axis, each with angle pi / 2:
    x-third pair k = 0 (channels 0, 1; freq 1):           xyz.x = pi / 2,         y = (1, 0) -> (0, 1)
    y-third pair k = 1 (channels 12, 13; freq f1):        xyz.y = pi / 2 / f1,    y = (0, 2) -> (-2, 0)
    z-third pair k = 4 (channels 28, 29; freq f4):        xyz.z = -pi / 2 / f4,   y = (3, 0) -> (0, -3)   (rotation by -pi / 2)
    and the merge takes each back.  Heads: channel c = h * 15 + d, so channel 28 is (h, d) = (1, 13)."""
    E = 30
    f = R.freq32(E).to(F64)
    xyz = torch.tensor([[[math.pi / 2, math.pi / 2 / f[1].item(), -math.pi / 2 / f[4].item()]]], dtype=F64)
    y = torch.zeros(1, 1, E, dtype=F64)
    y[0, 0, 0], y[0, 0, 13], y[0, 0, 28] = 1.0, 2.0, 3.0
    # float64 xyz is not an fp32 value: evaluate the pieces directly (forward() itself takes fp32 inputs to float64 unchanged)
    th = R.angles(xyz, f, E)
    o = R.rotate(y, torch.cos(th), torch.sin(th))
    want = torch.zeros(E, dtype=F64)
    want[1], want[12], want[29] = 1.0, -2.0, -3.0
    assert (o[0, 0] - want).abs().max().item() < 1e-15
    h = R.heads(o, 2)
    assert abs(h[0, 1, 0, 14].item() + 3.0) < 1e-15 and abs(h[0, 0, 0, 12].item() + 2.0) < 1e-15
    back = R.rotate(o, torch.cos(th), -torch.sin(th))
    assert (back - y).abs().max().item() < 1e-15


@pytest.mark.parametrize("E,ns", [(60, 1), (120, 3), (30, 16)])
def test_forward_and_merge_are_adjoint(E, ns):
    """<R(y) s, g> == <y, s R^T g> with g = sum_s dR[s]: a sign or an axis error in one of the two references fails here."""
    g_ = torch.Generator().manual_seed(ns)
    B, N, H = 2, 9, E // 15
    y = torch.randn(B, N, E, generator=g_)
    xyz = torch.rand(B, N, 3, generator=g_) * 4 - 2
    dR = torch.randn(ns, B, H, 64, 16, generator=g_)
    fr = R.freq32(E)
    o = R.forward(Y=y, xyz=xyz, freq=fr, scale=R.SC).val
    dY = R.merge(dR, N, xyz, fr, R.SC).val
    gsum = R.unheads(dR[:, :, :, :N, :15].to(F64).sum(0))
    lhs, rhs = (o * gsum).sum().item(), (y.to(F64) * dY).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    o2 = R.forward(Y=y, xyz=None, scale=R.SC).val
    dY2 = R.merge(dR, N, None, None, R.SC).val
    assert abs((o2 * gsum).sum().item() - (y.to(F64) * dY2).sum().item()) <= 1e-12 * max(1.0, abs(lhs))


def test_decoders_invert_the_encoders():
    g = torch.Generator().manual_seed(2)
    T = torch.randn(2, 37, 60, generator=g) * 3
    rows = R.encode16(T, 4, 64, True)
    assert torch.equal(R.carried_rows(rows), R.C.carried(rows))
    assert ((R.carried_rows(rows)[:, :, :37] - R.heads(T, 4).to(F64)).abs() <= R.format_bound(R.heads(T, 4).to(F64), "f16x2")).all()
    pl = R.planes16_of(rows, 2 | 4)
    assert torch.equal(R.planes_to_rows(R.C.rows_to_planes(rows)), rows) and (pl[:, :, 0, 15] == 1).all() and (pl[:, :, 1, 15] == 0).all()
    assert R.format_violations(rows, pl, 37, "f16", True, True) == []
    b3 = R.encode_bf16(T, 4, 64, 48)
    assert torch.equal(R.carried_rows(b3)[:, :, :37].float(), R.heads(T, 4))            # three parts carry fp32 exactly
    b2 = R.encode_bf16(T, 4, 64, 32)
    assert ((R.carried_rows(b2)[:, :, :37] - R.heads(T, 4).to(F64)).abs() <= R.format_bound(R.heads(T, 4).to(F64), "bf16x2")).all()
    assert R.format_violations(b3, R.C.rows_to_planes(b3[..., :32].contiguous()), 37, "bf16") == []


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_hits_what_its_names_claim():
    cs = R.CASES
    assert len({c.name for c in cs}) == len(cs)
    inst = {R.proj_instance(c) for c in cs if c.entry in ("proj16", "proj")}
    assert inst == {(4, 60, True), (4, 60, False), (8, 120, True), (8, 120, False), (4, 0, False), (8, 0, False)}
    inst16 = {R.proj_instance(c) for c in cs if c.entry == "proj16"}
    assert inst16 == inst                                                                # all six in the fp16 family alone
    for c in cs:
        if c.entry in ("proj16", "proj"):
            tag = "_%d_%d_" % R.proj_instance(c)[:2]
            assert tag in c.name and (("keq" in c.name or "identity" in c.name) == R.proj_instance(c)[2]), c.name
            assert c.K % 4 == 0
    assert {c.entry for c in cs} == {"split16", "proj16", "split", "split_qk", "split_vt", "proj", "rows_f32", "merge"}
    for entry in ("split16", "proj16", "merge"):
        assert {(c.E, c.H) for c in cs if c.entry == entry} == {(60, 4), (120, 8), (30, 2), (90, 6)}, entry
    assert {c.N for c in cs} >= {1, 63, 64, 65, 130, 1025, 4097}
    assert {c.K for c in cs if c.K} >= {12, 64, 256, 60, 120}
    assert any(c.B > 64 for c in cs if c.entry == "split16") and any(c.B > 64 for c in cs if c.entry == "proj16")
    assert any(c.pad == 128 and R.npad_of(c) == R.pad_to(c.N, 64) + 128 for c in cs)
    assert {c.ld for c in cs} == {1, 2, 3} and any(not c.walign for c in cs)
    assert {c.ns for c in cs if c.entry == "merge"} == {1, 3, 16}
    assert {b.parts for c in cs if c.entry in R.FP16_ENTRIES for b in c.blocks} >= {1, 2, 2 | 4, 2 | 8}
    assert {b.width for c in cs if c.entry in R.BF16_ENTRIES for b in c.blocks if b.rows} == {32, 48}
    assert {(b.rows, b.planes) for c in cs if c.entry == "split16" for b in c.blocks} == {(True, False), (False, True), (True, True)}
    assert any(len(c.blocks) == 2 for c in cs)
    assert sorted(R.MERGE_OPT_IN_CASES) == sorted(c.name for c in cs if c.entry == "merge" and c.E in (60, 120)) and len(R.MERGE_OPT_IN_CASES) >= 6
    for c in cs:
        x = R.build(c)
        for j, b in enumerate(c.blocks):
            if b.xyz == "big":
                th = R.angles(x.xyz[j], x.freq, c.E)
                assert (th.abs() >= 200).sum().item() > 100 and (th.abs() < 200).sum().item() > 100, c.name
                assert th.abs().max().item() < 1.1e4
            if b.xyz == "zeros":
                assert torch.signbit(x.xyz[j]).any() and (~torch.signbit(x.xyz[j])).any() and (x.xyz[j] == 0).all()
            if "exact" in c.name:
                assert R.is_exact(x, j), c.name
            elif c.entry != "merge":
                assert not R.is_exact(x, j) or b.xyz is None, c.name
        if c.vals == "sweep":
            v = (x.X if c.K else x.Y).abs().to(F64)
            assert v.min().item() < 2.0 ** -28 and 2.0 ** 14 < v.max().item() <= 2.0 ** 15
            s = c.blocks[0].scale
            assert ((v * s > 0) & (v * s < 2.0 ** -14)).any() and ((v * s > 2.0 ** -14) & (v * s < 2.0 ** -3)).any()   # subnormal hi, subnormal lo
        if c.entry == "merge":
            assert torch.isnan(x.dR[:, :, :, c.N:]).all() and torch.isnan(x.dR[..., 15]).all()
        if c.K and not c.walign:
            assert (x.W.data_ptr() - x.Pbuf.data_ptr()) % 16 == 4 and (x.bias is None or (x.bias.data_ptr() - x.Pbuf.data_ptr()) % 16 != 0)


# ------------------------------------------------------------------------------------------------ fair
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_fp32_emulation_passes_every_bound(sincos, name):
    x = R.build(name)
    c = x.case
    worst = 0.0
    for contract in (0, 1, 2):
        if c.entry == "merge":
            b = c.blocks[0]
            ref = R.merge(x.dR, x.N, x.xyz[0], x.freq, b.scale)
            got = R.emulate_merge(sincos, x.dR, x.N, x.xyz[0], x.freq, b.scale, contract=min(contract, 1))
            worst = max(worst, R.ratio(got.to(F64) - ref.val, ref.bound))
            continue
        for j in range(x.nb):
            T = R.emulate_forward(sincos, contract=contract, **R.block_inputs(x, j))
            out = R.expected_outputs(x, j, T)
            r, bad = R.evaluate(x, j, out)
            assert bad == [], (name, j, bad)
            worst = max(worst, r)
            if R.is_exact(x, j):
                assert r <= 1.0 and torch.equal(T.to(F64), R.forward(**R.block_inputs(x, j)).val), name     # the fp32 rows are exact
    print(f"[bounds] fp32 emulation of {name}: max(err / bound) = {worst:.3f}")
    assert worst <= 1.0, (name, worst)


# ------------------------------------------------------------------------------------------------ teeth
def _emul(sincos, name, j=0, enc=None, **mut):
    x = R.build(name)
    T = R.emulate_forward(sincos, **R.block_inputs(x, j), **mut)
    out = R.expected_outputs(x, j, T, **(enc or {}))
    r, bad = R.evaluate(x, j, out)
    print(f"[bounds] mutation on {name}: {mut or enc}: max(err / bound) = {r:.2f}, violations {bad}")
    return r, bad


def test_mutation_lo_part_truncated_or_dropped_fails_the_format_bound(sincos):
    for name in ("s16_v_e60_n64_rows8_exact", "s16_sweep_e60_exact", "p16_4_60_identity_sweep_exact"):
        assert _emul(sincos, name)[0] <= 1.0
        assert _emul(sincos, name, enc=dict(lo_mode="trunc"))[0] > 1.0, name
    for name in ("s16_q_e60_n1", "s16_e60_n4097", "p16_4_60_keq_qk_unaligned_w", "p16_8_120_k256_b70_nobias", "s16_big_theta_e60"):
        assert _emul(sincos, name, enc=dict(lo_mode="drop"))[0] > 1.0, name          # rotated / projected cases: the bound keeps its teeth


def test_mutation_flushed_subnormals_fail_the_sweep(sincos):
    for name in ("s16_sweep_e60_exact", "s16_sweep_e120_rot", "p16_4_60_identity_sweep_exact"):
        assert _emul(sincos, name, enc=dict(flush=True))[0] > 1.0, name
    # subnormal LO parts alone (hi normal): values in [2^-14, 2^-3) on a randn case lose them too
    assert _emul(sincos, "s16_v_e60_n64_rows8_exact", enc=dict(flush=True))[0] > 1.0


def test_mutation_sincos_off_by_1e6_fails(sincos):
    def off(th):
        sn, cs = sincos(th)
        return sn + 1e-6, cs - 1e-6
    for name in ("s16_e60_n4097", "s16_k_e120_n63_pad128_ld2", "rf_e120_n65_pad7_ld2", "sb_e60_rows48_planes"):
        assert _emul(off, name)[0] > 1.0, name
    x = R.build("m_e60_ns1")
    ref = R.merge(x.dR, x.N, x.xyz[0], x.freq, R.SC)
    assert R.ratio(R.emulate_merge(off, x.dR, x.N, x.xyz[0], x.freq, R.SC).to(F64) - ref.val, ref.bound) > 1.0


def test_mutation_rotation_sense_and_axis_order_fail(sincos):
    for name in ("s16_q_e60_n1", "p16_8_0_e90_k256", "sb_qk_e30_n65_pad128", "rf_e60_n1"):
        assert _emul(sincos, name, rot_sign=-1.0)[0] > 1e3, name
        assert _emul(sincos, name, axis_mode="mod3")[0] > 1e3, name
    x = R.build("m_e120_ns3_ld2")
    ref = R.merge(x.dR, x.N, x.xyz[0], x.freq, 1.0)
    assert R.ratio(R.emulate_merge(sincos, x.dR, x.N, x.xyz[0], x.freq, 1.0, rot_sign=-1.0).to(F64) - ref.val, ref.bound) > 1e3


def test_mutation_scale_applied_after_the_fp16_rounding_fails(sincos):
    """hi and lo formed from the UNSCALED rotated row and each multiplied by scale in fp16 afterwards."""
    name = "s16_e60_n4097"
    x = R.build(name)
    T = R.emulate_forward(sincos, apply_scale=False, **R.block_inputs(x, 0))
    rows = R.encode16(T, x.H, x.Npad, False)
    s = R.f32_value(R.SC)
    rows = (rows.float() * s).to(torch.float16)
    r, bad = R.evaluate(x, 0, dict(rows=rows, planes=None))
    print(f"[bounds] mutation on {name}: scale after the fp16 rounding: max(err / bound) = {r:.2f} {bad}")
    assert r > 1.0


def test_mutation_pad_rows_and_denominator_channel_fail_the_invariants(sincos):
    r, bad = _emul(sincos, "s16_k_e120_n63_pad128_ld2", enc=dict(pad_value=1e-3))
    assert any("pad rows not zero" in b for b in bad), bad
    x = R.build("s16_v_e60_n64_rows8_exact")
    out = R.expected_outputs(x, 0, R.emulate_forward(sincos, **R.block_inputs(x, 0)))
    assert R.evaluate(x, 0, out)[1] == []
    miss = dict(rows=out["rows"].clone(), planes=None)
    miss["rows"][..., 15] = 0.0                                                     # denominator channel missing
    assert any("channel 15" in b for b in R.evaluate(x, 0, miss)[1])
    real_only = dict(rows=out["rows"].clone(), planes=None)
    x2 = R.build("s16_e90_n1025_all_flags")
    out2 = R.expected_outputs(x2, 0, R.emulate_forward(sincos, **R.block_inputs(x2, 0)))
    assert R.evaluate(x2, 0, out2)[1] == []
    real_only = dict(rows=out2["rows"].clone(), planes=out2["planes"])
    real_only["rows"][:, :, x2.N:, 15] = 0.0                                        # 1.0 on the real rows only: not the writers' convention
    assert any("channel 15" in b for b in R.evaluate(x2, 0, real_only)[1])
    swapped = dict(rows=out2["rows"], planes=out2["planes"].clone())
    swapped["planes"][:, :, 1, 3, 5] = swapped["planes"][:, :, 1, 3, 6]
    assert any("different bits" in b for b in R.evaluate(x2, 0, swapped)[1])
    big_lo = dict(rows=out2["rows"].clone(), planes=None)
    big_lo["rows"][0, 0, 0, 16] = big_lo["rows"][0, 0, 0, 0] * 2.0 ** -9 + 2.0 ** -20   # a lo part above half an ulp of hi
    assert any("ulp" in b for b in R.evaluate(x2, 0, big_lo)[1])
