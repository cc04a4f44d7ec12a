"""Float64 reference, layout decoders, derived error bounds and the case table for the RoPE / projection operand writers and the
gradient merge (csrc/rope.hip, a3d_rope_rows_f32 of csrc/denoise.hip).

CPU-only module shared by tests/test_rope_operands_cpu.py (the reference is right, the bounds are fair and have teeth) and
tests/test_rope_operands_gpu.py (the kernels against them).  Nothing here imports the package under test; the sin / cos of the fp32
emulation is handed in by the caller (the CPU file passes the library's host mirror a3d_sincos_host).

The operation (rope_tile_to_lds / proj_rope_split_kernel):
    y = (X W^T + b) * scale          (the unfused writers are handed Y and compute y = Y * scale)
    third = E / 3, pair p = (channels 2p, 2p + 1), c = 2p, axis = c / third, k = (c mod third) / 2, theta = xyz[axis] * freq[k]
    o[2p] = y[2p] cos theta - y[2p + 1] sin theta,   o[2p + 1] = y[2p + 1] cos theta + y[2p] sin theta      (rotation by +theta)
    head split: channel c = h * 15 + d -> out[b][h][n][d]; d = 15 is padding (0, or 1.0 where the flags ask for the denominator channel)
freq (E / 6 fp32 values) is an INPUT of the kernels and of the reference: its own rounding is not under test.  xyz, X, W, b, Y and the
fp32 value of scale are taken to float64 exactly.  The merge is the transpose: dY = scale * R(xyz)^T sum_s dR[s].

Pad convention of the "16" writers (write_operand_formats16), pinned by format16_violations: rows n >= N are zero in channels 0-14 of
every part; channel 15 of the lo part is zero; channel 15 of the hi part is 1.0 on EVERY row below Npad (real and padded alike) when
the flag asks for it (parts | 8 for the rows, parts | 4 for the planes) and 0 otherwise.

Error bounds -- derived, not tuned.  u32 = 2^-24.  All are first-order sums multiplied by SECOND = 1 + 2^-10, which covers every product
of two first-order terms (each is below 2^-13 relative for K <= 2048) and the use of reference magnitudes in place of computed ones.

  projection   the fp32 MFMA 16x16x4 chain adds K products and the bias in some order, one rounding per operation (a fused
               multiply-add has fewer): for ANY order |fl(sum) - sum| <= gamma_{K+1} (sum_k |x_k w_k| + |b|), gamma_n = n u32 / (1 - n u32)
               (Higham, Accuracy and Stability, (3.5)).  Zero for the writers that are handed Y.
  scale        one fp32 product: u32 |y|; a power-of-two scale is exact (no value here is near fp32's subnormal range).
  angle        theta~ = fl(xyz * freq): |theta~ - theta| <= u32 |theta|, and sin, cos are 1-Lipschitz; the kernel's sin / cos of theta~ is
               within S of the true value, S = 1.2e-7 for |theta~| < 200 and 2e-7 above: the two figures that
               tests/test_host_cpu.py::test_rope_sincos_host_mirror_within_1e7_of_float64 asserts for the host mirror of fast_sincos
               (the same source compiled for the device; every multiply-add in it is an explicit fmaf).  eps_t = u32 |theta| + S.
  rotation     o = y0 cs - y1 sn in fp32: uncontracted it is fl(fl(y0 cs) - fl(y1 sn)) = two product roundings and one of the result,
               <= u32 (|y0 cs| + |y1 sn|) + u32 |o| <= 2 u32 (|y0| + |y1|); either fma contraction drops one of the product roundings.
               Together with the propagated errors:  e_o <= e_y0 + e_y1 + (|y0| + |y1|) (eps_t + 2 u32).
  format       what the operand carries against the fp32 value v it was split from:
               two-part fp16: hi = rne16(v), r = v - hi (exact), lo = rne16(r).  |r| <= ulp(hi) / 2 = 2^(e-11) for v in [2^e, 2^(e+1));
                 r is either that power of two exactly (representable) or lies in a binade below it, so ulp(lo) / 2 <= 2^(e-23):
                 2^-23 |v|.  Below 2^-14 fp16 is subnormal with spacing 2^-24: each rounding is at most 2^-25, and when hi is
                 subnormal r is at most 2^-25 and rounds to 0 or 2^-24: max(2^-23 |v|, 2^-25).  (tests/attn16_core_ref.py quotes the
                 looser 2^-22 for the same split; a lo part TRUNCATED toward zero errs by up to 2^-22 |v|, so the sharper constant
                 is what gives this term teeth.)
               one-part fp16 (planes with parts = 1): max(2^-11 |v|, 2^-25).
               two-part bf16 (8 significant bits): the same argument: 2^-17 |v|; three-part bf16 carries 8 + 1 + 8 + 1 + 8 bits >= fp32's
                 24: exact above bf16's subnormal range, stated as 2^-25 |v| ("fp32-grade").  bf16 has fp32's exponent range: no floor
                 for the values here.
               fp32 output (a3d_rope_rows_f32): none.
  merge        g = the fp32 sum over the splits in sequence: (nsplit - 1) u32 sum_s |dR|; the rotation as above on (G0, G1) = the sums of
               |dR| of the pair; the final product with scale u32 |dY|, and |dY| <= |scale| (G0 + G1):
               rotated:   |scale| (G0 + G1) ((nsplit + 2) u32 + eps_t)        unrotated:   |scale| G (nsplit u32)
"""
import math
from types import SimpleNamespace

import torch

import attn16_core_ref as C

HD = 15
U32 = 2.0 ** -24
S_SMALL, S_BIG, BIG_THETA = 1.2e-7, 2e-7, 200.0       # tests/test_host_cpu.py::test_rope_sincos_host_mirror_within_1e7_of_float64
SECOND = 1.0 + 2.0 ** -10
F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
LOG2E = 1.4426950408889634
SC = HD ** -0.5 * LOG2E                                # the scale the q rows of the split-fp16 family carry
pad_to = C.pad_to
ratio = C.ratio


def f32_value(s):
    """The value a C float argument holds."""
    return torch.tensor(s, dtype=F32).item()


def is_pow2(s):
    return s != 0 and math.frexp(abs(s))[0] == 0.5


def freq32(E):
    """The table ops.rope_freq builds (the reference project's div_term), fp32."""
    return torch.exp(torch.arange(0, E // 3, 2, dtype=F32) * (-math.log(10000.0) / (E // 3)))


# ------------------------------------------------------------------------------------------------ layouts
def heads(y, H):
    """[B][N][H * 15] -> [B][H][N][15]"""
    B, N, E = y.shape
    return y.view(B, N, H, E // H).permute(0, 2, 1, 3)


def unheads(x):
    """[B][H][N][15] -> [B][N][H * 15]"""
    B, H, N, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * d)


def planes_to_rows(planes):
    """planes [B][H][parts][16][Npad] -> rows [B][H][Npad][parts * 16] (the inverse of attn16_core_ref.rows_to_planes)."""
    B, H, P, _, Np = planes.shape
    return planes.permute(0, 1, 4, 2, 3).reshape(B, H, Np, P * 16)


def carried_rows(rows):
    """Sum of the 16-wide parts of a rows tensor (fp16 width 32, bf16 width 32 / 48, one-part width 16) in float64: [B][H][Npad][15]."""
    B, H, Np, W = rows.shape
    return rows.to(F64).view(B, H, Np, W // 16, 16).sum(-2)[..., :HD]


def split16(v, lo_mode="rne", flush=False):
    """fp32 -> (hi, lo) fp16 as rp_split_f16.  lo_mode / flush are the defects of the CPU file's mutation checks."""
    def ftz(h):
        return torch.where(h.abs().float() < 2.0 ** -14, torch.zeros_like(h), h) if flush else h
    v = v.to(F32)
    hi = ftz(v.to(F16))
    r = v - hi.float()                                                    # exact
    if lo_mode == "rne":
        lo = r.to(F16)
    elif lo_mode == "trunc":
        lo = r.to(F16)
        over = lo.float().abs() > r.abs()
        toward0 = torch.nextafter(lo, torch.zeros_like(lo))
        lo = torch.where(over, toward0, lo)
    elif lo_mode == "drop":
        lo = torch.zeros_like(hi)
    else:
        raise ValueError(lo_mode)
    return hi, ftz(lo)


def split_bf16_3(v):
    """fp32 -> (hi, lo, lo2) bf16 as a3d_common.h split_bf16_3 (split_bf16 is its first two parts)."""
    v = v.to(F32)
    hi = v.to(BF16)
    r1 = v - hi.float()
    lo = r1.to(BF16)
    lo2 = (r1 - lo.float()).to(BF16)
    return hi, lo, lo2


def encode16(T, H, Npad, rows_ones, lo_mode="rne", flush=False, pad_value=0.0):
    """fp32 [B][N][E] -> rows16 [B][H][Npad][32] with the writers' pad convention (module docstring)."""
    B, N, E = T.shape
    hi, lo = split16(heads(T, H), lo_mode, flush)
    rows = torch.zeros(B, H, Npad, 32, dtype=F16)
    rows[:, :, N:, :HD] = pad_value
    rows[:, :, :N, :HD] = hi
    rows[:, :, :N, 16:16 + HD] = lo
    if rows_ones:
        rows[:, :, :, HD] = 1.0
    return rows


def planes16_of(rows, parts):
    """The planes tensor the same call writes: the first (parts & 3) parts of the rows, channel 15 of the hi plane by the | 4 flag."""
    pl = C.rows_to_planes(rows)[:, :, :parts & 3].clone()
    pl[:, :, 0, HD, :] = 1.0 if parts & 4 else 0.0
    return pl


def encode_bf16(T, H, Npad, width):
    B, N, E = T.shape
    rows = torch.zeros(B, H, Npad, width, dtype=BF16)
    for i, part in enumerate(split_bf16_3(heads(T, H))[:width // 16]):
        rows[:, :, :N, 16 * i:16 * i + HD] = part
    return rows


def _ulp(h, p, spacing):
    """ulp of a p-significant-bit format at h (float64 tensor of representable values); `spacing` in the subnormal range and at 0."""
    _, e = torch.frexp(h)
    return torch.maximum(torch.exp2((e - p).to(F64)), torch.full_like(h, spacing)) * (h != 0) + spacing * (h == 0)


def format_violations(rows, planes, N, fmt, rows_ones=False, planes_ones=False):
    """Names of the format invariants an output violates (empty list: none).  rows [B][H][Npad][W] / planes [B][H][P][16][Npad], either
    may be None; fmt "f16" or "bf16"."""
    p, spacing = (11, 2.0 ** -24) if fmt == "f16" else (8, 2.0 ** -133)
    bad = []
    views = []
    if rows is not None:
        views.append(("rows", rows, rows_ones))
    if planes is not None:
        views.append(("planes", planes_to_rows(planes), planes_ones))
    for name, r, ones in views:
        r64 = r.to(F64)
        nparts = r.shape[-1] // 16
        if not torch.isfinite(r64).all():
            bad.append(f"{name}: not finite")
            continue
        for i in range(1, nparts):
            prev, cur = r64[..., 16 * (i - 1):16 * i], r64[..., 16 * i:16 * (i + 1)]
            if not (cur.abs() <= _ulp(prev, p, spacing) / 2).all():
                bad.append(f"{name}: |part {i}| > ulp(part {i - 1}) / 2")
        for i in range(nparts):
            if not (r64[:, :, N:, 16 * i:16 * i + HD] == 0).all():
                bad.append(f"{name}: pad rows not zero in part {i}")
            want = 1.0 if (ones and i == 0) else 0.0
            if not (r64[..., 16 * i + HD] == want).all():
                bad.append(f"{name}: channel 15 of part {i} is not {want} on every row below Npad")
    if rows is not None and planes is not None:
        P = planes.shape[2]
        a = rows[..., :P * 16].clone().view(torch.int16)
        b = planes_to_rows(planes).clone().view(torch.int16)
        a.view(*a.shape[:-1], P, 16)[..., HD] = 0                          # channel 15 follows each output's own flag (checked above)
        b.view(*b.shape[:-1], P, 16)[..., HD] = 0
        if not torch.equal(a, b):
            bad.append("rows and planes of one call carry different bits")
    return bad


# ------------------------------------------------------------------------------------------------ the operation, float64
def pair_maps(E, axis_mode="third"):
    """(axis, k) of each of the E / 2 channel pairs."""
    third = E // 3
    c = torch.arange(0, E, 2)
    if axis_mode == "third":
        axis = c // third
        k = (c - axis * third) // 2
    elif axis_mode == "mod3":                                              # the defect of the CPU file: interleaved axes
        axis = c % 3
        k = (c // 2) % (third // 2)
    else:
        raise ValueError(axis_mode)
    return axis, k


def angles(xyz, freq, E, dtype=F64, axis_mode="third"):
    """theta [B][N][E / 2] = xyz[axis] * freq[k] in `dtype` (float64: exact, both factors are fp32)."""
    axis, k = pair_maps(E, axis_mode)
    return xyz.to(dtype)[..., axis] * freq.to(dtype)[k]


def rotate(y, cs, sn):
    """Pairs (2p, 2p + 1) of y rotated by the angle whose cos / sin are given: the oracle's rotary_apply in pair form."""
    o = torch.empty_like(y)
    y0, y1 = y[..., 0::2], y[..., 1::2]
    o[..., 0::2] = y0 * cs - y1 * sn
    o[..., 1::2] = y1 * cs + y0 * sn
    return o


def _pairsum(a):
    """|a0| + |a1| of each pair, on both channels of the pair."""
    s = a[..., 0::2].abs() + a[..., 1::2].abs()
    return s.repeat_interleave(2, dim=-1)


def _eps_theta(th):
    s = torch.where(th.abs() >= BIG_THETA * (1 - 2.0 ** -20), torch.full_like(th, S_BIG), torch.full_like(th, S_SMALL))
    return (U32 * th.abs() + s).repeat_interleave(2, dim=-1)


def forward(Y=None, X=None, W=None, b=None, xyz=None, freq=None, scale=1.0):
    """Reference value [B][N][E] (float64) of the rotated, scaled rows and the arithmetic part of the bound (everything but the format
    term).  Either Y [B][N][E] or X [B][N][K], W [E][K] and optionally b [E]."""
    s = f32_value(scale)
    if Y is None:
        X64, W64 = X.to(F64), W.to(F64)
        y = X64 @ W64.t()
        A = X64.abs() @ W64.abs().t()
        if b is not None:
            y = y + b.to(F64)
            A = A + b.to(F64).abs()
        n = X.shape[-1] + 1
        e_y = n * U32 / (1 - n * U32) * A * abs(s)
    else:
        y = Y.to(F64)
        e_y = torch.zeros_like(y)
    y = y * s
    if not is_pow2(s):
        e_y = e_y + U32 * y.abs()
    E = y.shape[-1]
    if xyz is None:
        return SimpleNamespace(val=y, arith=SECOND * e_y, theta=None)
    th = angles(xyz, freq, E)
    o = rotate(y, torch.cos(th), torch.sin(th))
    e_o = _pairsum(e_y) + _pairsum(y) * (_eps_theta(th) + 2 * U32)
    return SimpleNamespace(val=o, arith=SECOND * e_o, theta=th)


def format_bound(v, kind):
    a = v.abs()
    if kind == "f16x2":
        return SECOND * torch.clamp_min(2.0 ** -23 * a, 2.0 ** -25)
    if kind == "f16x1":
        return SECOND * torch.clamp_min(2.0 ** -11 * a, 2.0 ** -25)
    if kind == "bf16x2":
        return SECOND * 2.0 ** -17 * a
    if kind == "bf16x3":
        return SECOND * 2.0 ** -25 * a
    if kind == "f32":
        return torch.zeros_like(a)
    raise ValueError(kind)


def merge(dR, N, xyz=None, freq=None, scale=1.0):
    """dY [B][N][E] = scale R(xyz)^T sum_s dR[s] in float64 from dR [nsplit][B][H][Npad][16] (rows >= N and channel 15 are not read),
    and its bound."""
    s = f32_value(scale)
    ns = dR.shape[0]
    d = dR[:, :, :, :N, :HD].to(F64)
    g = unheads(d.sum(0))
    G = unheads(d.abs().sum(0))
    if xyz is None:
        return SimpleNamespace(val=g * s, bound=SECOND * abs(s) * G * (ns * U32))
    th = angles(xyz, freq, g.shape[-1])
    y = rotate(g, torch.cos(th), -torch.sin(th)) * s
    return SimpleNamespace(val=y, bound=SECOND * abs(s) * _pairsum(G) * ((ns + 2) * U32 + _eps_theta(th)))


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def emulate_forward(sincos, Y=None, X=None, W=None, b=None, xyz=None, freq=None, scale=1.0, contract=0, rot_sign=1.0,
                    axis_mode="third", apply_scale=True):
    """The writers' arithmetic in fp32 on the CPU -> T [B][N][E] fp32 (what they hand to the format conversion).
    sincos(theta fp32 tensor) -> (sin, cos) fp32.  contract: 0 = every product and sum rounded, 1 / 2 = the first / second product of
    each rotation line fused into the sum.  rot_sign, axis_mode, apply_scale: the defects of the mutation checks."""
    s = torch.tensor(scale if apply_scale else 1.0, dtype=F32)
    if Y is None:
        y = X.to(F32) @ W.to(F32).t()
        if b is not None:
            y = y + b.to(F32)
    else:
        y = Y.to(F32)
    y = y * s
    if xyz is None:
        return y
    th = angles(xyz, freq, y.shape[-1], F32, axis_mode)
    sn, cs = sincos(th)
    sn = sn * rot_sign
    y0, y1 = y[..., 0::2], y[..., 1::2]

    def line(a, ca, bb, cb, sign):                                         # a * ca + sign * bb * cb
        if contract == 0:
            return a * ca + sign * (bb * cb)
        if contract == 1:
            return (a.double() * ca.double() + sign * (bb * cb).double()).float()
        return ((a * ca).double() + sign * bb.double() * cb.double()).float()

    o = torch.empty_like(y)
    o[..., 0::2] = line(y0, cs, y1, sn, -1.0)
    o[..., 1::2] = line(y1, cs, y0, sn, 1.0)
    return o


def emulate_merge(sincos, dR, N, xyz=None, freq=None, scale=1.0, contract=0, rot_sign=1.0):
    d = dR[:, :, :, :N, :HD].to(F32)
    g = torch.zeros_like(d[0])
    for i in range(d.shape[0]):
        g = g + d[i]
    g = unheads(g)
    s = torch.tensor(scale, dtype=F32)
    if xyz is None:
        return g * s
    th = angles(xyz, freq, g.shape[-1], F32)
    sn, cs = sincos(th)
    sn = sn * rot_sign
    g0, g1 = g[..., 0::2], g[..., 1::2]
    y = torch.empty_like(g)
    if contract == 0:
        y[..., 0::2] = cs * g0 + sn * g1
        y[..., 1::2] = cs * g1 - sn * g0
    else:
        y[..., 0::2] = (cs.double() * g0.double() + (sn * g1).double()).float()
        y[..., 1::2] = (cs.double() * g1.double() - (sn * g0).double()).float()
    return y * s


# ------------------------------------------------------------------------------------------------ cases
# One table for the CPU file (the fp32 emulation passes every bound) and the GPU file (the kernels).
#   entry: split16 | proj16 (fp16 family), split | split_qk | split_vt | proj (bf16 family), rows_f32, merge
#   blocks: output blocks of one launch (two only for proj16 / proj): xyz kind (None | "unit" [-0.5, 1.5] | "zeros" (signed) |
#           "big" (half of the rows up to 1e4: |theta| >= 200)), scale, parts (fp16 family: 1 | 2, + 4 / + 8) or rows width (bf16
#           family), which outputs are written
#   pad: Npad = ceil64(N) + pad;  ld: row stride of Y / X / dY in units of its width (the operand is the LAST column block of a packed
#   buffer);  walign: W and bias 16-byte aligned (False: 4-byte aligned only, as in a flat parameter buffer);  vals: "randn" |
#   "sweep" (log-uniform magnitudes 2^-30 .. 2^15, both signs);  ident: W = identity, no bias (the projection is then exact)
def blk(xyz="unit", scale=1.0, parts=2, rows=True, planes=False, width=48):
    return SimpleNamespace(xyz=xyz, scale=scale, parts=parts, rows=rows, planes=planes, width=width)


def _c(name, entry, E, B, N, blocks=None, K=None, pad=0, ld=1, walign=True, bias=True, vals="randn", ident=False, ns=1):
    return SimpleNamespace(name=name, entry=entry, E=E, H=E // HD, B=B, N=N, blocks=blocks or [blk()], K=K, pad=pad, ld=ld,
                           walign=walign, bias=bias, vals=vals, ident=ident, ns=ns)


Q, KB = dict(xyz="unit", scale=SC), dict(xyz="unit", scale=1.0)
V8, V4 = dict(xyz=None, scale=1.0, parts=2 | 8), dict(xyz=None, scale=1.0, parts=2 | 4, rows=False, planes=True)
CASES = [
    # ---- a3d_rope_split16 (rope_split_kernel, fmt16)
    _c("s16_q_e60_n1", "split16", 60, 2, 1, [blk(**Q, planes=True)]),
    _c("s16_k_e120_n63_pad128_ld2", "split16", 120, 1, 63, [blk(**KB)], pad=128, ld=2),
    _c("s16_v_e60_n64_rows8_exact", "split16", 60, 2, 64, [blk(**V8)]),
    _c("s16_v_e120_n65_planes4_ld3_exact", "split16", 120, 2, 65, [blk(**V4)], ld=3),
    _c("s16_e30_n130_parts1", "split16", 30, 3, 130, [blk(**Q, parts=1, planes=True)]),
    _c("s16_e90_n1025_all_flags", "split16", 90, 1, 1025, [blk(**KB, parts=2 | 4 | 8, planes=True)]),
    _c("s16_e60_n4097", "split16", 60, 1, 4097, [blk(**Q)]),
    _c("s16_e60_b70_n65_pad128", "split16", 60, 70, 65, [blk(**Q, planes=True)], pad=128),
    _c("s16_sweep_e60_exact", "split16", 60, 2, 130, [blk(xyz=None, scale=0.5, planes=True)], vals="sweep"),
    _c("s16_sweep_e120_rot", "split16", 120, 2, 130, [blk(**Q, planes=True)], vals="sweep"),
    _c("s16_signed_zero_xyz", "split16", 60, 2, 65, [blk(xyz="zeros", scale=0.5)]),
    _c("s16_big_theta_e60", "split16", 60, 2, 130, [blk(xyz="big", scale=SC, planes=True)]),
    # ---- a3d_proj_rope_split16: the six proj_rope_split_kernel instances
    _c("p16_4_60_keq_qk_unaligned_w", "proj16", 60, 2, 130, [blk(**Q), blk(**KB)], K=60, walign=False),
    _c("p16_4_60_k12_kv", "proj16", 60, 2, 65, [blk(**KB), blk(**V8)], K=12),
    _c("p16_4_60_k256_ld2", "proj16", 60, 1, 63, [blk(**Q, planes=True)], K=256, ld=2),
    _c("p16_8_120_keq_kv_planes_n1025", "proj16", 120, 1, 1025, [blk(**KB), blk(**V4)], K=120, walign=False),
    _c("p16_8_120_k64_pad128", "proj16", 120, 2, 64, [blk(**Q)], K=64, pad=128),
    _c("p16_8_120_k256_b70_nobias", "proj16", 120, 70, 65, [blk(**KB, planes=True)], K=256, bias=False),
    _c("p16_4_0_e30_k12", "proj16", 30, 2, 130, [blk(**Q), blk(**V8)], K=12, walign=False),
    _c("p16_4_0_e30_k64_n4097", "proj16", 30, 1, 4097, [blk(**KB)], K=64),
    _c("p16_8_0_e90_k256", "proj16", 90, 2, 65, [blk(**Q, planes=True), blk(**KB)], K=256),
    _c("p16_8_0_e90_k12_n1", "proj16", 90, 2, 1, [blk(**KB, parts=1, planes=True)], K=12, pad=128),
    _c("p16_4_60_identity_sweep_exact", "proj16", 60, 2, 130, [blk(xyz=None, scale=0.5, planes=True)], K=60, vals="sweep", ident=True, bias=False),
    _c("p16_8_120_keq_big_theta", "proj16", 120, 2, 65, [blk(xyz="big", scale=SC), blk(xyz="big", scale=1.0)], K=120),
    # ---- the bf16 family: a3d_rope_split (+ _qk, a3d_split_vt), a3d_proj_rope_split
    _c("sb_e60_rows48_planes", "split", 60, 2, 130, [blk(**Q, planes=True)]),
    _c("sb_e120_rows32_planes_exact", "split", 120, 2, 65, [blk(xyz=None, scale=1.0, width=32, planes=True)], ld=2),
    _c("sb_sweep_e60_rows48_exact", "split", 60, 2, 130, [blk(xyz=None, scale=0.5, planes=True)], vals="sweep"),
    _c("sb_qk_e30_n65_pad128", "split_qk", 30, 3, 65, [blk(**Q)], pad=128),
    _c("sb_vt_e90_n1025_exact", "split_vt", 90, 1, 1025, [blk(xyz=None, scale=1.0, rows=False, planes=True)], ld=3),
    _c("pb_4_60_keq_qk", "proj", 60, 2, 130, [blk(**Q), blk(**KB, planes=True)], K=60, walign=False),
    _c("pb_8_120_k64_kv", "proj", 120, 2, 65, [blk(**KB), blk(xyz=None, scale=1.0, width=32, planes=True)], K=64),
    _c("pb_4_0_e30_k256", "proj", 30, 2, 63, [blk(**Q, width=32)], K=256, pad=128),
    _c("pb_8_0_e90_k12_big_theta", "proj", 90, 1, 130, [blk(xyz="big", scale=SC, planes=True)], K=12),
    # ---- a3d_rope_rows_f32 (Npad need not be a multiple of 64)
    _c("rf_e60_n1", "rows_f32", 60, 5, 1, [blk(**Q)]),
    _c("rf_e120_n65_pad7_ld2", "rows_f32", 120, 2, 65, [blk(**KB)], pad=7, ld=2),
    _c("rf_e30_sweep_exact", "rows_f32", 30, 2, 130, [blk(xyz=None, scale=1.0)], vals="sweep"),
    _c("rf_e90_big_theta", "rows_f32", 90, 2, 130, [blk(xyz="big", scale=SC)]),
    # ---- a3d_rope_merge_bwd (default kernel in-process; E = 60 / 120 again under each opt-in kernel in a child process)
    _c("m_e60_ns1", "merge", 60, 2, 130, [blk(**Q)], ns=1),
    _c("m_e120_ns3_ld2", "merge", 120, 2, 65, [blk(**KB)], ns=3, ld=2, pad=128),
    _c("m_e60_ns16_n1025", "merge", 60, 1, 1025, [blk(**Q)], ns=16),
    _c("m_e120_ns16_noxyz", "merge", 120, 2, 63, [blk(xyz=None, scale=SC)], ns=16),
    _c("m_e30_ns3_ld3", "merge", 30, 3, 64, [blk(**Q)], ns=3, ld=3),
    _c("m_e90_ns1_n1", "merge", 90, 2, 1, [blk(**KB)], ns=1),
    _c("m_e60_b70_ns3", "merge", 60, 70, 65, [blk(**Q)], ns=3),
    _c("m_e120_n4097_ns3", "merge", 120, 1, 4097, [blk(**Q)], ns=3),
    _c("m_e60_big_theta_ns3_ld2", "merge", 60, 2, 130, [blk(xyz="big", scale=SC)], ns=3, ld=2),
]
CASE_BY_NAME = {c.name: c for c in CASES}
MERGE_OPT_IN_CASES = [c.name for c in CASES if c.entry == "merge" and c.E in (60, 120)]
FP16_ENTRIES, BF16_ENTRIES = ("split16", "proj16"), ("split", "split_qk", "split_vt", "proj")


def proj_instance(c):
    """The proj_rope_split_kernel<NT, EC, KEQ> instance the launch code selects for a projection case."""
    ec = c.E if c.E in (60, 120) else 0
    return (4 if c.E <= 64 else 8, ec, ec > 0 and c.K == c.E)


def npad_of(c):
    return (c.N if c.entry == "rows_f32" else pad_to(c.N, 64)) + c.pad


def _values(g, shape, kind):
    if kind == "randn":
        return torch.randn(*shape, generator=g, dtype=F32)
    mag = torch.exp2(torch.rand(*shape, generator=g, dtype=F64) * 45.0 - 30.0)
    sign = torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0).to(F64)
    return (mag * sign).to(F32)


def _xyz(g, kind, B, N):
    if kind is None:
        return None
    if kind == "unit":
        return torch.rand(B, N, 3, generator=g, dtype=F32) * 2 - 0.5
    if kind == "zeros":
        return torch.where(torch.rand(B, N, 3, generator=g) < 0.5, -0.0, 0.0).to(F32)
    if kind == "big":
        x = torch.rand(B, N, 3, generator=g, dtype=F32) * 2 - 0.5
        big = (torch.rand(B, N, 3, generator=g, dtype=F32) * 2 - 1) * 1e4
        return torch.where((torch.arange(N) % 2 == 0).view(1, N, 1), big, x)
    raise ValueError(kind)


def build(case):
    """Inputs of a case as fp32 CPU tensors in the buffers the kernels are handed (strides, column offsets, misaligned parameters)."""
    c = case if not isinstance(case, str) else CASE_BY_NAME[case]
    g = torch.Generator().manual_seed(4000 + 11 * CASES.index(c))
    B, N, E, H = c.B, c.N, c.E, c.H
    x = SimpleNamespace(case=c, B=B, N=N, E=E, H=H, Npad=npad_of(c), freq=freq32(E), nb=len(c.blocks))
    x.xyz = [_xyz(g, b_.xyz, B, N) for b_ in c.blocks]
    if c.entry == "merge":
        x.dR = torch.randn(c.ns, B, H, x.Npad, 16, generator=g, dtype=F32)
        x.dR[:, :, :, N:] = float("nan")                                   # must not be read
        x.dR[..., HD] = float("nan")
        x.ldy, x.off = E * c.ld, E * (c.ld - 1)
        return x
    if c.K is not None:
        K = c.K
        x.K, x.ldx = K, K * c.ld
        x.Xbuf = _values(g, (B, N, x.ldx), c.vals)
        x.X = x.Xbuf[..., x.ldx - K:]
        x.xoff = x.ldx - K
        nW = x.nb * E * K
        x.wshift = 0 if c.walign else 1                                    # floats in front of W in the parameter buffer
        x.Pbuf = torch.zeros(x.wshift + nW + 3 + x.nb * E)
        x.W = x.Pbuf[x.wshift:x.wshift + nW].view(x.nb * E, K)
        if c.ident:
            assert K == E and x.nb == 1 and not c.bias
            x.W.copy_(torch.eye(E))
        else:
            x.W.copy_(torch.randn(x.nb * E, K, generator=g) * K ** -0.5)
        x.boff = x.wshift + nW + (0 if c.walign else 2)
        x.bias = None
        if c.bias and not c.ident:
            x.bias = x.Pbuf[x.boff:x.boff + x.nb * E]
            x.bias.copy_(torch.randn(x.nb * E, generator=g))
    else:
        x.ldy, x.off = E * c.ld, E * (c.ld - 1)
        x.Ybuf = _values(g, (B, N, x.ldy), c.vals)
        x.Y = x.Ybuf[..., x.off:]
    return x


def block_inputs(x, j):
    """Keyword arguments of forward() / emulate_forward() for output block j."""
    b_ = x.case.blocks[j]
    kw = dict(xyz=x.xyz[j], freq=x.freq, scale=b_.scale)
    if x.case.K is not None:
        E = x.E
        kw.update(X=x.X, W=x.W[j * E:(j + 1) * E], b=None if x.bias is None else x.bias[j * E:(j + 1) * E])
    else:
        kw.update(Y=x.Y)
    return kw


def is_exact(x, j):
    """The block is a pure format conversion: no rotation, a power-of-two scale, no (or an identity) projection."""
    b_ = x.case.blocks[j]
    return b_.xyz is None and is_pow2(f32_value(b_.scale)) and (x.case.K is None or x.case.ident)


def expected_outputs(x, j, T, **mut):
    """The output tensors block j's writer produces from the fp32 rows T [B][N][E] (the format conversion alone, restated in torch):
    dict with "rows" / "planes" (None where the case writes none)."""
    c, b_ = x.case, x.case.blocks[j]
    out = dict(rows=None, planes=None)
    if c.entry in FP16_ENTRIES:
        rows = encode16(T, x.H, x.Npad, bool(b_.parts & 8), **mut)
        out["rows"] = rows if b_.rows else None
        out["planes"] = planes16_of(rows, b_.parts) if b_.planes else None
    elif c.entry in BF16_ENTRIES:
        rows = encode_bf16(T, x.H, x.Npad, b_.width)
        out["rows"] = rows if b_.rows else None
        out["planes"] = C.rows_to_planes(rows[..., :32].contiguous()) if b_.planes else None
    else:
        o = torch.zeros(x.B, x.H, x.Npad, 16, dtype=F32)
        o[:, :, :x.N, :HD] = heads(T, x.H)
        out["rows"] = o
    return out


def evaluate(x, j, out, ref=None):
    """Holds block j's outputs (CPU tensors, dict as expected_outputs) to the reference: returns (max(err / bound) over every output,
    list of violated format invariants)."""
    c, b_ = x.case, x.case.blocks[j]
    ref = ref or forward(**block_inputs(x, j))
    want = heads(ref.val, x.H)
    arith = heads(ref.arith, x.H)
    worst, bad = 0.0, []
    if c.entry == "rows_f32":
        o = out["rows"].to(F64)
        if not ((o[:, :, x.N:] == 0).all() and (o[..., HD] == 0).all()):
            bad.append("rows: pad rows / channel 15 not zero")
        return ratio(o[:, :, :x.N, :HD] - want, arith), bad
    fp16 = c.entry in FP16_ENTRIES
    if fp16:
        bad = format_violations(out["rows"], out["planes"], x.N, "f16", bool(b_.parts & 8), bool(b_.parts & 4))
    else:
        bad = format_violations(out["rows"], out["planes"], x.N, "bf16")
    for name in ("rows", "planes"):
        t = out[name]
        if t is None:
            continue
        r = t if name == "rows" else planes_to_rows(t)
        nparts = r.shape[-1] // 16
        kind = ("f16x%d" if fp16 else "bf16x%d") % nparts
        got = carried_rows(r)[:, :, :x.N]
        worst = max(worst, ratio(got - want, arith + format_bound(want, kind)))
    return worst, bad
