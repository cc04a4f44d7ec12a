"""Case builders, float64 references, fp32 twins and error bounds for the fused denoise kernels of csrc/denoise.hip
(a3d_dn_head, a3d_dn_cross, a3d_dn_rest, a3d_dn_tail / a3d_dn_tail_sched), one phase at a time.

CPU-only module shared by tests/test_denoise_ref_cpu.py (the references are right, the bounds are fair and have teeth) and
tests/test_denoise_kernels_gpu.py (the kernels against them).  Nothing here imports the package under test.  It reuses the operand
formats, the attention reference and the derived bound of tests/attn16_core_ref.py and the projection / scale / rotation model of
tests/rope_ref.py.

The operations (every function below takes a `dt`: torch.float64 is the reference, torch.float32 the twin -- the SAME function in fp32
on the CPU; parameters and inputs are fp32 tensors, exact in both):
  head   x = relu(traj W0^T + b0) W1^T + b1;  with instruction tokens: q = ((x + sem) Wq^T + bq) / sqrt(15), softmax attention per
         head over the tokens' k | v rows (lang_kv [B][S_lang][2E]), x = LN(x + o Wo^T + bo)
  cross  a = (x + sem)(1 + scale) + shift (mod = scale | shift);  q = rope((a Wq^T + bq) / sqrt(15)) by the rows' xyz;  softmax
         attention of head h's 15 channels over the CARRIED keys / values (hi + lo of the fp16 operands, built on the host by
         attn16_core_ref.make_rows16 / rows_to_planes: the test does not depend on the device's operand writer), keys >= S masked by
         position.  The kernel writes per-split partials (Op [nsplit][B][H][16][16] with sum p in column 15, Mp [nsplit][B][H][16] the
         natural-log running maximum, -inf for a split without a valid key); combine_partials() merges them in float64.
  rest   combine the partials -> out-proj -> LN12(x + .) -> self-attention block (q, k from AdaLN1(x + sem), v from AdaLN1(x), RoPE on
         q and k, key mask) -> LN1(x + .) -> y = AdaLNff(x), LN122(y + FFN(y))
  tail   mo = cat(traj_xyz + regressor_pos(pos_feats), regressor_rot(rot_feats));  in-paint (cond_mask -> cond_data);  terminal step:
         the result is mo;  otherwise c0 clamp(mo, -1, 1) + c1 traj + c2 noise with (c0, c1, c2) = row `row` of coef_pos (channels
         0-2) / coef_rot (the others)
  All keys masked (the self-attention's kmask, or every split of a head at -inf / a zero denominator in the combine): the kernels DEFINE
  the attention output as 0 (wg_small_attention: inv = l > 0 ? 1 / l : 0), the convention of attn16_core_ref for a fully masked sample.
  The reference follows it; torch.softmax would give NaN there.

oracle.blocks is not used for the references: its mha computes the RoPE tables in fp32 even under LIFT = float64 (rope3d_code), which
would put an fp32 sin / cos error into the reference, and its adaln takes the timestep embedding where the kernels take the modulation
row.  The local functions are pinned to oracle.blocks.parallel_attention_layer / mlp2 (LIFT = float64) by
tests/test_denoise_ref_cpu.py::test_references_agree_with_the_oracle_blocks.

Bounds.
  cross (derived).  attn16_core_ref.bounds(..., extra_score_err).O_adaptive: the adaptive forward bound (GAMMA_F, PHI_P, N_ACC, u16 times
    the sub-2^-LO_SPAN mass) with the per-(query, key) score error increased by what the kernel's own q carries:
      extra[q, k] = sum_d bound_q[q, d] |k_d| log2 e  +  2^-21 sum_d |q_d k_d| log2 e
    bound_q = rope_ref.forward(X = a, W = Wq, b = bq, xyz, freq, scale = 15^-1/2).arith: gamma_{K+1} (sum |a W| + |b|) |scale| holds for
    ANY summation order (Higham (3.5)), so the kernel's plain sequential k-order sum `acc += a[k] w[k]` is inside the model; + u32 |y| for
    the scale product; rotation with eps_t = u32 |theta| + S (fast_sincos) and 2 u32.  Two things that model does not hold, added here:
      * a is computed by the kernel in fp32: t1 = fl(x + sem), t2 = fl(1 + scale), t3 = fl(t1 t2), a = fl(t3 + shift) -- four roundings,
        |a~ - a| <= e_a = u32 (3 |x + sem| |1 + scale| + |a|) to first order; it reaches y as |scale| sum_k e_a[k] |W[c, k]|;
      * the kernel's scale constant is 1.0f / sqrtf(15.0f): two correctly rounded operations, within 2 u32 of 15^-1/2 relative, where
        rope_ref.forward assumes the fp32 value nearest to 15^-1/2: + 2 u32 |y|.
    Both go through the rotation as propagated errors (e_y0 + e_y1 on either channel of a pair).  The second term of extra is the two-part
    fp16 split of fl(q log2 e) (2^-23 |q2|, rope_ref's format bound), the fp32 product with log2 e and that constant's own rounding
    (2^-24 each): 2^-22 in all, stated as 2^-21.
  dense fp32 chains (head, rest, tail).  Per output tensor err(y) = max |y - ref64| / max |ref64| and the kernel must satisfy
      err(kernel) <= max(2^-20, 4 err(twin)).
    The project's precedent (cfg-4 gradients, tests/test_diffusion_gpu.py) is 3 x the fp32 oracle's own error; 4 here because wg_linear
    sums up to 512 products in one sequential fmaf chain where the CPU BLAS blocks them; 2^-20 = 16 u32 keeps cases whose twin is almost
    exact (L = 1, E = 30) from making the ratio meaningless.  Neither figure was chosen from a kernel's output.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as Fn

import attn16_core_ref as C
import rope_ref as R

HD = 15
F64, F32 = torch.float64, torch.float32
U32 = 2.0 ** -24
LOG2E = R.LOG2E
Q_SCALE = HD ** -0.5
TWIN_FLOOR = 2.0 ** -20
TWIN_MARGIN = 4.0
HEAD_LDS_BYTES, HEAD_STATIC_BYTES = 150 * 1024, 4 * 16 * 132 * 4      # a3d_dn_head: dynamic + static LDS must stay below 150 KiB


def max_s_lang(E):
    """Largest instruction-token count a3d_dn_head accepts: the k | v rows (2E floats per token) share the LDS with four [16][132] tiles."""
    return (HEAD_LDS_BYTES - HEAD_STATIC_BYTES) // (8 * E)


def rel_err(y, ref):
    """err(y) of the twin rule: max |y - ref| / max |ref|."""
    y, ref = y.to(F64), ref.to(F64)
    if not torch.isfinite(y).all():
        return math.inf
    return ((y - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def twin_limit(err_twin):
    return max(TWIN_FLOOR, TWIN_MARGIN * err_twin)


# ------------------------------------------------------------------------------------------------ small functions, any dtype
def linear(x, W, b, dt):
    y = x @ W.to(dt).t()
    return y if b is None else y + b.to(dt)


def layer_norm(x, g, b, dt, eps=1e-5):
    return Fn.layer_norm(x, (x.shape[-1],), g.to(dt), None if b is None else b.to(dt), eps)


def adaln(x, mod, dt, swap=False):
    """x (1 + scale) + shift with mod = scale | shift ([2E]); None: x."""
    if mod is None:
        return x
    E = x.shape[-1]
    sc, sh = mod[:E].to(dt), mod[E:].to(dt)
    if swap:
        sc, sh = sh, sc
    return x * (1 + sc) + sh


def rope(y, xyz, freq, dt, axis_mode="third"):
    """Pairs of y [B][L][E] rotated by theta = xyz[axis] * freq[k] (rope_ref's maps); the angle product, sin and cos in `dt`."""
    if freq is None:
        return y
    th = R.angles(xyz[..., :3], freq, y.shape[-1], dt, axis_mode)
    return R.rotate(y, torch.cos(th), torch.sin(th))


def attention(q, k, v, H, kmask, dt):
    """Softmax attention per head of q [B][L][E] (scaled, rotated) over k / v [B][S][E]; kmask [B][S] bool (True = masked) or None.
    A row whose keys are all masked gives 0 (module docstring)."""
    qh, kh, vh = R.heads(q, H), R.heads(k, H), R.heads(v, H)
    s = qh @ kh.transpose(-1, -2)
    if kmask is not None:
        s = s.masked_fill(kmask[:, None, None, :], -math.inf)
    m = s.amax(-1, keepdim=True)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m0)
    l = p.sum(-1, keepdim=True)
    w = torch.where(l > 0, p / l.clamp_min(1e-300), torch.zeros_like(p))
    return R.unheads(w @ vh)


def combine_partials(Op, Mp, dt=F64):
    """Op [ns][B][H][16][16] (column 15 = sum p), Mp [ns][B][H][16] -> O [B][H][16][15]: sum_s e^(Mp_s - m) Op_s / sum_s e^(Mp_s - m) l_s,
    0 where every split is at -inf or the denominator is 0."""
    Op, Mp = Op.to(dt), Mp.to(dt)
    m = Mp.amax(0)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    w = torch.exp(Mp - m0)
    num = (w[..., None] * Op[..., :HD]).sum(0)
    den = (w * Op[..., HD]).sum(0)[..., None]
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))


# ------------------------------------------------------------------------------------------------ generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _w(g, n_out, n_in, gain=1.0):
    return torch.randn(n_out, n_in, generator=g, dtype=F32) * (gain * n_in ** -0.5)


def _b(g, n, n_in):
    return torch.randn(n, generator=g, dtype=F32) * n_in ** -0.5


def _gain(g, n):
    return 1.0 + 0.1 * torch.randn(n, generator=g, dtype=F32)


def _mod(g, E):
    return 0.3 * torch.randn(2 * E, generator=g, dtype=F32)


def _traj(g, B, L, D):
    t = torch.randn(B, L, D, generator=g, dtype=F32)
    t[..., :3] = torch.rand(B, L, 3, generator=g, dtype=F32) * 2 - 1
    return t


# ================================================================================================ cross attention
def _x(name, E, S, Sp, ns, B=1, L=16, D=9, kind="rand", freq=True, mod=True, sem=True, garbage=False):
    return SimpleNamespace(name=name, E=E, H=E // HD, S=S, Sp=Sp, ns=ns, B=B, L=L, D=D, kind=kind, freq=freq, mod=mod, sem=sem,
                           garbage=garbage)


KEY_COUNT_LIST = [(1, 64, 1), (31, 64, 1), (33, 64, 1), (64, 64, 1), (65, 128, 1), (65, 256, 1), (65, 128, 64), (130, 192, 3),
                  (200, 256, 8), (1025, 1088, 1), (1025, 1088, 2), (1025, 1088, 3), (1025, 1216, 5), (4097, 4160, 1)]
SCORE_KINDS = ["flat", "spike_late", "staircase", "creep", "dominant_between_refreshes", "two_scales"]
CROSS_CASES = (
    [_x(f"keys_s{S}_sp{Sp}_ns{ns}", 30, S, Sp, ns) for S, Sp, ns in KEY_COUNT_LIST]
    + [_x(f"heads_e{E}", E, 200, 256, 2, B=3, L=7) for E in (60, 90, 120)]
    + [_x("rows_l1", 60, 200, 256, 2, L=1), _x("rows_l15", 60, 200, 256, 2, L=15)]
    + [_x("opt_d3", 60, 130, 192, 1, D=3), _x("opt_d10", 60, 130, 192, 1, D=10), _x("opt_no_freq", 60, 130, 192, 1, freq=False),
       _x("opt_no_mod", 60, 130, 192, 1, mod=False), _x("opt_no_sem", 60, 130, 192, 1, sem=False)]
    + [_x(f"score_{k}", 60, 1025, 1088, 1, kind=k) for k in SCORE_KINDS]
    + [_x("pad_garbage_s65_sp256", 30, 65, 256, 1, garbage=True)]
)
CROSS_BY_NAME = {c.name: c for c in CROSS_CASES}


def wave_ranges(Sp, nsplit):
    """[h_beg, h_end) in 32-key halves of every wave of every split (dn_cross_kernel: NH = Sp / 32, parts = 4 nsplit)."""
    NH, parts = Sp // 32, 4 * nsplit
    return [(NH * part // parts, NH * (part + 1) // parts) for part in range(parts)]


def build_cross(case):
    """Inputs of a cross case (fp32 CPU tensors), the fp16 cache operands built on the host and the values they carry."""
    c = case if not isinstance(case, str) else CROSS_BY_NAME[case]
    g = _gen(7000 + 13 * CROSS_CASES.index(c))
    B, L, D, E, H, S, Sp = c.B, c.L, c.D, c.E, c.H, c.S, c.Sp
    x = SimpleNamespace(case=c, B=B, L=L, D=D, E=E, H=H, S=S, Sp=Sp, ns=c.ns)
    x.x = torch.randn(B, L, E, generator=g, dtype=F32)
    x.traj = _traj(g, B, L, D)
    x.sem = torch.randn(L, E, generator=g, dtype=F32) if c.sem else None
    x.mod = _mod(g, E) if c.mod else None
    x.q_w, x.q_b = _w(g, E, E), _b(g, E, E)
    x.freq = R.freq32(E) if c.freq else None
    k = torch.randn(B, H, S, HD, generator=g, dtype=F64)
    v = torch.randn(B, H, S, HD, generator=g, dtype=F64)
    if c.kind != "rand":
        # a fixed, simple q: zero rows, no index embedding, no modulation, xyz = 0 (identity rotation): q = b_q / sqrt(15) with
        # channel 0 of every head = 1 in log2 units and the other channels 0, so that s2[q, k] = k[.., 0] = the profile t (log2 units)
        x.x.zero_()
        x.sem, x.mod = None, None
        x.traj[..., :3] = 0.0
        x.q_w.zero_()
        x.q_b.zero_()
        x.q_b[0::HD] = HD ** 0.5 / LOG2E
        j = torch.arange(S)
        hf = j // 32
        noise = torch.rand(S, generator=g, dtype=F64)
        rng = wave_ranges(Sp, c.ns)
        if c.kind == "flat":
            t = torch.full((S,), 3.0, dtype=F64)
        elif c.kind == "spike_late":                                       # one key 40 above the rest in the last half of wave 1's range
            t = -noise
            t[(rng[1][1] - 1) * 32 + 5] = 40.0
        elif c.kind == "staircase":                                        # + 9 per half: a rescale in every half
            t = 9.0 * hf - noise
        elif c.kind == "creep":                                            # one rise of 7.5 two halves into each wave's range: p up to 2^11.5, no rescale
            t = -noise
            for hb, he in rng:
                t[hb * 32] = 0.0                                           # the first half's maximum, exactly
                sel = (hf >= hb + 2) & (hf < he)
                t[sel] = 7.5 - noise[sel]
        elif c.kind == "dominant_between_refreshes":                       # half 5 of wave 2's range: the threshold was refreshed at half 0
            # two keys 7.5 and 7.13 above the range's first half (below P_THR: no rescale) and ~10 above the other keys, holding
            # far-apart values: 98 % of the mass, so that what a dropped low part costs them is far beyond what the bound allows the
            # sub-threshold keys
            t = -noise - 3.0
            t[rng[2][0] * 32] = 0.0
            ia = (rng[2][0] + 5) * 32 + 7
            t[ia], t[ia + 1] = 7.5, 7.13
            v[:, :, ia] += 6.0
            v[:, :, ia + 1] -= 6.0
        elif c.kind == "two_scales":                                       # every other key 30 below: p = 2^-26 of the maximum, under fp16's floor
            t = torch.where(j % 2 == 1, -30.0, 0.0).to(F64) - noise
        else:
            raise ValueError(c.kind)
        k = k * 0.1
        k[..., 0] = t
    x.Kf = C.make_rows16(k, npad=Sp)
    x.Vt = C.rows_to_planes(C.make_rows16(v, ones=True, npad=Sp))
    x.k, x.v = C.carried(x.Kf, S), C.carried(C.make_rows16(v, ones=True, npad=Sp), S)
    x.k_pad, x.v_pad = C.carried(x.Kf), C.carried(C.make_rows16(v, ones=True, npad=Sp))     # all Sp rows (the padding mutation)
    return x


def garbage_operands(x):
    """Kf / Vt of a case with rows [S, Sp) filled with finite garbage (+-6e4) in every channel of every part."""
    Kf, Vt = x.Kf.clone(), x.Vt.clone()
    n = x.Sp - x.S
    sign = torch.where(torch.arange(n * 32) % 3 == 0, -6e4, 6e4).to(torch.float16)
    Kf[:, :, x.S:] = sign.view(n, 32)
    Vt[:, :, :, :, x.S:] = sign.view(32, n)[:16]
    return Kf, Vt


def cross_a(x, dt, swap=False):
    a = x.x.to(dt)
    if x.sem is not None:
        a = a + x.sem.to(dt)
    return adaln(a, x.mod, dt, swap)


def cross_reference(x):
    """Float64 O [B][H][L][15], the attention reference and the derived bound (module docstring)."""
    a = cross_a(x, F64)
    xyz = x.traj[..., :3] if x.freq is not None else None
    fw = R.forward(X=a, W=x.q_w, b=x.q_b, xyz=xyz, freq=x.freq, scale=Q_SCALE)
    # what rope_ref.forward does not model: the fp32 AdaLN in front of the projection and the kernel's own scale constant
    e_a = x.x.to(F64)
    if x.sem is not None:
        e_a = e_a + x.sem.to(F64)
    e_a = e_a.abs()
    if x.mod is not None:
        e_a = 3.0 * e_a * (1 + x.mod[:x.E].to(F64)).abs()
    e_a = U32 * (e_a + a.abs())
    s = R.f32_value(Q_SCALE)
    y = (a @ x.q_w.to(F64).t() + x.q_b.to(F64)) * s
    extra_y = (e_a @ x.q_w.to(F64).abs().t()) * abs(s) + 2 * U32 * y.abs()
    bound_q = fw.arith + R.SECOND * (R._pairsum(extra_y) if xyz is not None else extra_y)
    q2 = R.heads(fw.val, x.H) * LOG2E                                     # [B][H][L][15], log2 units
    bq = R.heads(bound_q, x.H) * LOG2E
    ka = x.k.abs()
    extra = bq @ ka.transpose(-1, -2) + 2.0 ** -21 * (q2.abs() @ ka.transpose(-1, -2))
    ref = C.reference(q2, x.k, x.v, None)
    b = C.bounds(ref, q2, x.k, x.v, None, extra_score_err=extra)
    return SimpleNamespace(O=ref.O, bound=b.O_adaptive, bound_no_extra=C.bounds(ref, q2, x.k, x.v, None).O_adaptive, ref=ref, q2=q2,
                           bound_q=bound_q)


def _sincos(th):
    return torch.sin(th), torch.cos(th)


def cross_twin(x, p_mode="adaptive", mask_at="S", axis_mode="third", swap=False):
    """The kernel's arithmetic restated in fp32 on the CPU: fp32 AdaLN, projection, scale, rotation (rope_ref.emulate_forward), two-part
    fp16 q log2 e, fp32 softmax with P rounded to fp16 (two parts where the weight exceeds 2^-LO_SPAN: "adaptive"; "drop_lo": one part
    for every key -- the defect).  mask_at = "Sp": the padded keys take part (the defect)."""
    a = cross_a(x, F32, swap)
    xyz = x.traj[..., :3] if x.freq is not None else None
    T = R.emulate_forward(_sincos, X=a, W=x.q_w, b=x.q_b, xyz=xyz, freq=x.freq, scale=Q_SCALE, axis_mode=axis_mode)
    q2 = C.two_part16((T * torch.tensor(LOG2E, dtype=F32)).to(F64))
    q2 = R.heads(q2, x.H)
    k, v = (x.k, x.v) if mask_at == "S" else (x.k_pad, x.v_pad)

    def p_round(p, w):
        p64 = p.to(F64)
        if p_mode == "drop_lo":
            return C.round16(p64).to(p.dtype)
        return torch.where(w > 2.0 ** -C.LO_SPAN, C.two_part16(p64), C.round16(p64)).to(p.dtype)

    return C.attention(q2, k, v, None, None, F32, p_round=p_round).O.to(F64)


# ================================================================================================ rest of a layer
def _r(name, E, F, L=7, B=2, D=9, ns=3, kmask=None, sa=True, ffn=True, walign=True):
    return SimpleNamespace(name=name, E=E, H=E // HD, F=F, L=L, B=B, D=D, ns=ns, kmask=kmask, sa=sa, ffn=ffn, walign=walign)


REST_CASES = [
    _r("e30_f30", 30, 30), _r("e60_f60", 60, 60, ns=1), _r("e90_f100", 90, 100), _r("e120_f480", 120, 480, ns=8),
    _r("e120_f512", 120, 512), _r("e60_f240", 60, 240),
    _r("l1_e30", 30, 30, L=1, ns=1), _r("l1_e120", 120, 480, L=1), _r("l16_e120_ns8", 120, 480, L=16, ns=8), _r("l16_e90", 90, 100, L=16),
    _r("kmask_last3", 60, 240, L=16, B=3, kmask="last3"), _r("kmask_all_but_row0", 60, 240, L=16, B=3, kmask="all_but_0"),
    _r("kmask_all", 60, 240, L=7, B=3, kmask="all"), _r("kmask_last3_e120", 120, 480, L=7, B=3, kmask="last3"),
    _r("no_self_attention", 60, 240, sa=False), _r("no_ffn", 60, 240, ffn=False),
    _r("d10_e90", 90, 100, D=10, L=16), _r("d10_e30", 30, 30, D=10),
    _r("unaligned_weights_e60", 60, 240, L=16, walign=False),
]
REST_BY_NAME = {c.name: c for c in REST_CASES}
REST_WEIGHTS = ("c_out_w", "s_in_w", "s_out_w", "f_w1", "f_w2")


def build_rest(case):
    c = case if not isinstance(case, str) else REST_BY_NAME[case]
    g = _gen(8000 + 17 * REST_CASES.index(c))
    B, L, D, E, H, F, ns = c.B, c.L, c.D, c.E, c.H, c.F, c.ns
    x = SimpleNamespace(case=c, B=B, L=L, D=D, E=E, H=H, F=F, ns=ns)
    x.x = torch.randn(B, L, E, generator=g, dtype=F32)
    x.traj = _traj(g, B, L, D)
    x.sem = torch.randn(L, E, generator=g, dtype=F32)
    x.freq = R.freq32(E)
    # synthetic partials: finite everywhere, some splits at -inf (their Op rows hold finite values that must get weight 0), head 0 of
    # sample 0 at -inf in EVERY split (denominator 0 -> the combined output is 0)
    x.Op = torch.randn(ns, B, H, 16, 16, generator=g, dtype=F32)
    x.Op[..., HD] = torch.rand(ns, B, H, 16, generator=g, dtype=F32) * 20 + 0.5
    x.Op[..., :HD] *= x.Op[..., HD:]
    x.Mp = torch.randn(ns, B, H, 16, generator=g, dtype=F32) * 3
    for s in range(ns):
        for b in range(B):
            for h in range(H):
                if (ns > 1 and (s + b + h) % 3 == 0) or (b == 0 and h == 0):
                    x.Mp[s, b, h] = -math.inf
    p = SimpleNamespace()
    p.c_out_w, p.c_out_b, p.c_ln_g, p.c_ln_b = _w(g, E, E), _b(g, E, E), _gain(g, E), 0.1 * torch.randn(E, generator=g)
    p.s_mod, p.f_mod = _mod(g, E), _mod(g, E)
    p.s_in_w, p.s_in_b, p.s_out_w, p.s_out_b = _w(g, 3 * E, E), _b(g, 3 * E, E), _w(g, E, E), _b(g, E, E)
    p.s_ln_g, p.s_ln_b = _gain(g, E), 0.1 * torch.randn(E, generator=g)
    p.f_w1, p.f_b1, p.f_w2, p.f_b2 = _w(g, F, E), _b(g, F, E), _w(g, E, F), _b(g, E, F)
    p.f_ln_g, p.f_ln_b = _gain(g, E), 0.1 * torch.randn(E, generator=g)
    x.p = p
    x.kmask = None
    if c.kmask is not None:
        km = torch.zeros(B, L, dtype=torch.bool)
        if c.kmask == "last3":
            km[:, L - 3:] = True
        elif c.kmask == "all_but_0":
            km[:, 1:] = True
        elif c.kmask == "all":
            km[:] = True
        km[B - 1] = False                                                  # the last sample keeps every key
        x.kmask = km
    return x


def rest_forward(x, dt, mut=()):
    """x_out [B][L][E] in `dt`.  mut: names of deliberate defects (the mutation checks of the CPU file)."""
    c, p = x.case, x.p
    B, L, E, H = x.B, x.L, x.E, x.H
    eps = 1e-6 if "ln_eps" in mut else 1e-5
    swap = "adaln_swap" in mut
    o = R.unheads(combine_partials(x.Op, x.Mp, dt)[:, :, :L])
    h = layer_norm(x.x.to(dt) + linear(o, p.c_out_w, p.c_out_b, dt), p.c_ln_g, p.c_ln_b, dt, eps)
    if c.sa:
        qk_in = adaln(h + x.sem.to(dt), p.s_mod, dt, swap)
        v_in = adaln(h + x.sem.to(dt) if "sem_in_v" in mut else h, p.s_mod, dt, swap)
        q = linear(qk_in, p.s_in_w[:E], p.s_in_b[:E], dt) * torch.tensor(Q_SCALE, dtype=F32).to(dt)
        k = linear(qk_in, p.s_in_w[E:2 * E], p.s_in_b[E:2 * E], dt)
        v = linear(v_in, p.s_in_w[2 * E:], p.s_in_b[2 * E:], dt)
        am = "mod3" if "rope_axis" in mut else "third"
        q, k = rope(q, x.traj, x.freq, dt, am), rope(k, x.traj, x.freq, dt, am)
        km = x.kmask
        if km is not None and "kmask_shift" in mut:
            km = torch.roll(km, 1, dims=1)
        o = attention(q, k, v, H, km, dt)
        h = layer_norm(h + linear(o, p.s_out_w, p.s_out_b, dt), p.s_ln_g, p.s_ln_b, dt, eps)
    if c.ffn:
        y = adaln(h, p.f_mod, dt, swap)
        f = linear(torch.relu(linear(y, p.f_w1, p.f_b1, dt)), p.f_w2, p.f_b2, dt)
        h = layer_norm((h if "ffn_res_x" in mut else y) + f, p.f_ln_g, p.f_ln_b, dt, eps)
    return h


# ================================================================================================ head
def _h(name, E, D, L, S_lang, B=3):
    return SimpleNamespace(name=name, E=E, H=E // HD, D=D, L=L, S_lang=S_lang, B=B)


HEAD_CASES = [
    _h("e30_d4_l1_s1", 30, 4, 1, 1), _h("e30_d9_l16_smax", 30, 9, 16, max_s_lang(30)), _h("e30_d9_l1_nolang", 30, 9, 1, None),
    _h("e60_d16_l16_s53", 60, 16, 16, 53), _h("e60_d9_l16_smax", 60, 9, 16, max_s_lang(60)), _h("e60_d4_l16_s1", 60, 4, 16, 1),
    _h("e120_d9_l16_s53", 120, 9, 16, 53), _h("e120_d4_l1_smax", 120, 4, 1, max_s_lang(120)), _h("e120_d16_l16_nolang", 120, 16, 16, None),
]
HEAD_BY_NAME = {c.name: c for c in HEAD_CASES}


def build_head(case):
    c = case if not isinstance(case, str) else HEAD_BY_NAME[case]
    g = _gen(9000 + 19 * HEAD_CASES.index(c))
    B, L, D, E = c.B, c.L, c.D, c.E
    x = SimpleNamespace(case=c, B=B, L=L, D=D, E=E, H=c.H, S_lang=c.S_lang)
    x.traj = _traj(g, B, L, D)
    p = SimpleNamespace()
    p.enc_w0, p.enc_b0, p.enc_w1, p.enc_b1 = _w(g, E, D), _b(g, E, D), _w(g, E, E), _b(g, E, E)
    p.sem = torch.randn(L, E, generator=g, dtype=F32)
    p.q_w, p.q_b, p.out_w, p.out_b = _w(g, E, E), _b(g, E, E), _w(g, E, E), _b(g, E, E)
    p.ln_g, p.ln_b = _gain(g, E), 0.1 * torch.randn(E, generator=g)
    x.lang_kv = None if c.S_lang is None else torch.randn(B, c.S_lang, 2 * E, generator=g, dtype=F32)
    x.p = p
    return x


def head_forward(x, dt, mut=()):
    p, E = x.p, x.E
    h = linear(torch.relu(linear(x.traj.to(dt), p.enc_w0, p.enc_b0, dt)), p.enc_w1, p.enc_b1, dt)
    if x.lang_kv is not None:
        q = linear(h + p.sem.to(dt), p.q_w, p.q_b, dt) * torch.tensor(Q_SCALE, dtype=F32).to(dt)
        kv = x.lang_kv.to(dt)
        o = attention(q, kv[..., :E].contiguous(), kv[..., E:].contiguous(), x.H, None, dt)
        h = layer_norm(h + linear(o, p.out_w, p.out_b, dt), p.ln_g, p.ln_b, dt, 1e-6 if "ln_eps" in mut else 1e-5)
    return h


# ================================================================================================ tail
T_ROWS = 10                                        # rows of the posterior coefficient tables of the tail cases


def _tl(name, E, D, L, mask, noise, entry, row, terminal=0, B=3):
    """entry "tail": a3d_dn_tail(t_step = row), terminal when row == 0;  "sched": a3d_dn_tail_sched(row, terminal)."""
    return SimpleNamespace(name=name, E=E, D=D, L=L, mask=mask, noise=noise, entry=entry, row=row,
                           terminal=int(row == 0) if entry == "tail" else terminal, B=B)


TAIL_CASES = [
    _tl("e30_d4_l1_last_row", 30, 4, 1, None, True, "tail", T_ROWS - 1),
    _tl("e30_d9_l16_scatter_t0_terminal", 30, 9, 16, "scatter", True, "tail", 0),
    _tl("e120_d9_l16_rows_t5", 120, 9, 16, "rows", True, "tail", 5),
    _tl("e120_d16_l16_scatter_nonoise_t1", 120, 16, 16, "scatter", False, "tail", 1),
    _tl("sched_e120_d16_l16_scatter_row0", 120, 16, 16, "scatter", False, "sched", 0, 0),
    _tl("sched_e120_d9_l1_last_row_terminal", 120, 9, 1, None, True, "sched", T_ROWS - 1, 1),
    _tl("sched_e30_d16_l16_rows_last_row", 30, 16, 16, "rows", False, "sched", T_ROWS - 1, 0),
    _tl("sched_e120_d4_l16_scatter_row3", 120, 4, 16, "scatter", True, "sched", 3, 0),
    _tl("sched_e30_d9_l16_rows_row0_terminal", 30, 9, 16, "rows", True, "sched", 0, 1),
]
TAIL_BY_NAME = {c.name: c for c in TAIL_CASES}


def build_tail(case):
    c = case if not isinstance(case, str) else TAIL_BY_NAME[case]
    g = _gen(10000 + 23 * TAIL_CASES.index(c))
    B, L, D, E = c.B, c.L, c.D, c.E
    x = SimpleNamespace(case=c, B=B, L=L, D=D, E=E, row=c.row, terminal=c.terminal)
    x.pos_feats = torch.randn(B, L, E, generator=g, dtype=F32)
    x.rot_feats = torch.randn(B, L, E, generator=g, dtype=F32)
    x.traj = _traj(g, B, L, D)
    p = SimpleNamespace()
    # second layers scaled by sqrt(2): the ReLU halves the hidden units' second moment, so the outputs have unit variance and about a
    # third of |x0| exceeds 1 (asserted by the CPU file)
    p.pos_w0, p.pos_b0, p.pos_w1, p.pos_b1 = _w(g, E, E), _b(g, E, E), _w(g, 3, E, 2 ** 0.5), _b(g, 3, E)
    p.rot_w0, p.rot_b0, p.rot_w1, p.rot_b1 = _w(g, E, E), _b(g, E, E), _w(g, D - 3, E, 2 ** 0.5), _b(g, D - 3, E)
    p.coef_pos = torch.randn(T_ROWS, 3, generator=g, dtype=F32)
    p.coef_rot = torch.randn(T_ROWS, 3, generator=g, dtype=F32)
    p.noise = torch.randn(B, L, D, generator=g, dtype=F32) if c.noise else None
    p.cond_data, p.cond_mask = None, None
    if c.mask is not None:
        p.cond_data = 1.5 * torch.randn(B, L, D, generator=g, dtype=F32)
        if c.mask == "scatter":
            p.cond_mask = torch.rand(B, L, D, generator=g) < 0.3
        else:
            p.cond_mask = torch.zeros(B, L, D, dtype=torch.bool)
            p.cond_mask[:, 0] = True
            p.cond_mask[:, L - 1] = True
    x.p = p
    return x


def tail_network_output(x, dt):
    p = x.p
    pos = linear(torch.relu(linear(x.pos_feats.to(dt), p.pos_w0, p.pos_b0, dt)), p.pos_w1, p.pos_b1, dt)
    rot = linear(torch.relu(linear(x.rot_feats.to(dt), p.rot_w0, p.rot_b0, dt)), p.rot_w1, p.rot_b1, dt)
    return torch.cat((x.traj[..., :3].to(dt) + pos, rot), dim=-1)


def tail_forward(x, dt, mut=()):
    p = x.p
    mo = tail_network_output(x, dt)
    if "clamp_first" in mut:
        mo = mo.clamp(-1.0, 1.0)
    if p.cond_mask is not None:
        mo = torch.where(p.cond_mask, p.cond_data.to(dt), mo)
    if x.terminal and "terminal_coef" not in mut:
        return mo
    x0 = mo if "clamp_first" in mut else mo.clamp(-1.0, 1.0)
    cf = torch.cat((p.coef_pos[x.row].expand(3, 3), p.coef_rot[x.row].expand(x.D - 3, 3)), 0).to(dt)      # [D][3]
    out = cf[:, 0] * x0 + cf[:, 1] * x.traj.to(dt)
    if p.noise is not None:
        out = out + cf[:, 2] * p.noise.to(dt)
    return out


# ------------------------------------------------------------------------------------------------ shared (reference, twin error) cache
FORWARD = {"rest": (build_rest, rest_forward), "head": (build_head, head_forward), "tail": (build_tail, tail_forward)}
_PREPARED = {}


def prepared(kind, name):
    """(inputs, float64 reference, err(twin)) of a dense-chain case, computed once per process."""
    key = (kind, name)
    if key not in _PREPARED:
        build, fwd = FORWARD[kind]
        x = build(name)
        ref = fwd(x, F64)
        _PREPARED[key] = (x, ref, rel_err(fwd(x, F32), ref))
    return _PREPARED[key]
