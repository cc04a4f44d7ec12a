"""Operands, a float64 reference and derived error bounds for the split-fp16 attention core (csrc/attention16.hip).

CPU-only module shared by tests/test_attn16_core_cpu.py (the reference and the bounds have teeth) and
tests/test_attn16_core_gpu.py (the kernels against them).  Nothing here imports the package under test.

Conventions (pinned by the known-answer case of the CPU file and again on the device):
  * operands are rows16 tensors [B][H][Npad][32] fp16, hi(16) | lo(16) of the 16-padded head row (head dim 15); value rows carry
    1.0 in channel 15 of the hi part of every row below Npad; padded rows are zero otherwise.  The value an operand CARRIES is hi + lo, exact in float64: the
    reference is computed from carried values, so operand rounding is not part of the error under test.
  * scores are in log2 units: s2 = q . k (q already holds scale * log2 e), w = 2^s2 / sum_k 2^s2, LSE2 = m + log2 sum_k 2^(s2 - m).
  * dQ, dK, dV are the plain derivatives of sum(O * dO) with respect to the carried q, k, v: the ln 2 of d w / d s2 is inside
    (the kernel folds it into dOn = dO ln2 2^-e; dV is multiplied by log2 e again), and the softmax scale that the carried q
    holds is applied later by a3d_rope_merge_bwd, not by the core.  G = ln2 * w * (dP - D), dQ = G K, dK = G^T Q, dV = w^T dO.
  * a fully masked sample: O = 0, LSE2 = -inf, all gradients zero.

Error bounds -- derived, not tuned.  u16 = 2^-11 (half an ulp of fp16), u32 = 2^-24.

  score error.  A score is two K = 32 MFMAs (all four hi/lo products, so the products are exact) accumulated in fp32 on top of the
  accumulator init P_OFF - m.  Modelled as C_DOT = 12 fp32 roundings (an MFMA adds its 32 exact products in a tree, 5 levels, and
  then the accumulator: 6 per instruction, two instructions) of partial sums no larger than
  A_qk = sum_d |q_d k_d| + max_k |s2_qk| + P_OFF + P_THR:
      eps_s(q, k) = C_DOT u32 A_qk   (absolute, log2 units)  ->  relative weight error ln2 eps_s.
  An fp32 CPU evaluation has the same term (15 products, blocked by the BLAS).

  GAMMA_F = 2^-20: relative error of one weight as the PV product sees it, besides the score error.  Two-part fp16 P: |p - hi - lo| <=
  u16 |lo| <= u16^2 |p| = 2^-22.  Hardware exp2: 1 ulp = 2^-23, taken as 2^-22.  Sum 2^-21, times 2 for the second-order terms, the
  combine kernel's per-split factor (one exp2f and two fp32 products, common to all keys of a split) and the final division.
  The output is an exactly normalised average (the denominator is accumulated from the SAME rounded P through the ones channel of V),
  so a weight error e_k moves O by sum_k w_k e_k (v_k - o): the deviation from the mean, not |v|.

  PHI_P = 2^-28 per live key: the absolute floor of fp16.  p = 2^(s2 - m_run + P_OFF) and the largest key of a row has p >= 2^P_OFF =
  16, so the denominator is >= 16; below 2^-14 fp16 is subnormal with spacing 2^-24: hi and lo each err by <= 2^-25 absolute, together
  2^-24 / 16 = 2^-28 of the denominator per key, whatever the key's weight.

  N_ACC(n) = n / 16 + 16 fp32 roundings for a contraction over n elements: one per MFMA accumulation step (at most 4 MFMAs per 64
  elements and accumulator) plus 16 for the final sums, scalings and the combine.  A blocked fp32 CPU sum (SIMD partial sums) is
  inside the same count.  Enters as u32 N_ACC (sum |terms|).

  forward, both parts (PP = 3):  |O - O64|_qd <= sum_k (w_qk (GAMMA_F + ln2 eps_s) + PHI_P) |v_kd - o_qd| + u32 N_ACC(S) (sum_k w |v| + |o|)
  forward, adaptive (PP = 2):    the above + u16 sum_{k: w_qk <= 2^-LO_SPAN} w_qk |v_kd - o_qd|   (the kernel's own claim: only keys
                                 below 2^-6 of the denominator may lose their low part, each by at most half an fp16 ulp)
  LSE2: sum_k w (GAMMA_F / ln2 + eps_s) + (PHI_P n_live + u32 N_ACC(S)) / ln2 + 2^-22 (|LSE2| + |m| + 32)   [+ u16 / ln2 * sub-threshold mass]
        (the last term: v_log_f32 at 1 ulp of a result below 32 and the fp32 sum m + log2 l).

  backward.  The kernels recompute the weights from the forward's LSE2 (relative error ln2 (eps_s + bound_LSE2)), use D = dOn . O from
  the forward's O (error <= sum_d |dO| bound_O + rounding), and dOn = two-part fp16 of dO ln2 2^-e: per element 2^-21 |dO| (two-part
  rounding, the fp32 product with ln2) + 2^-23 max_d |dO_q| (fp16's subnormal spacing against a row maximum in [0.5, 1)).
  dP - D is one K = 32 MFMA pair on the init -D: C_DOT u32 (sum_d |dO||v| + sum_d |dO||o|).
      E_G(q, k) = ln2 w_qk [ (gamma + ln2 (eps_s + bound_LSE2)) |dP - D| + C_DOT u32 A2 + sum_d dOerr_qd |v_kd - o_qd| + bound_D_q ]
  GAMMA_DQ  = 2^-20: G is two-part fp16 (2^-22) + exp2 (2^-22), times 2 as above.  Floor: G' = 2^B_OFF p (dPn - Dn) in fp16
              subnormals errs by 2^-24 absolute, i.e. 2^-24 2^-B_OFF 2^e_q <= 2^-29 ln2 max_d |dO_q| per key in output units.
  GAMMA_DKV = 1.25 * 2^-14: P' and G' enter the dV / dK MFMAs as split bf16 BY TRUNCATION (attn_ring.h pk_bf16_2t: hi keeps 8 bits,
              lo 8 bits of the remainder: 15 significant bits truncated toward zero = 2^-14 relative, one-sided); the Q^T / dOn^T planes are
              rounded split bf16 (2^-17), exp2 2^-22: together under a quarter of the first term.  bf16 has fp32's exponent range, so
              the only floor is fp32's own: P' = 2^(B_OFF + s2 - lse2 + e_q - E_c) (E_c: the largest row exponent of the 64 sorted rows
              that hold q) and G' = P' (dPn - Dn) are flushed below 2^-126, i.e. a weight floor PHI32_q = 2^(E_c - e_q - 126 - B_OFF)
              per (row, key): sum_q PHI32_q |dO| in dV, ln2 sum_q PHI32_q (|dP - D| + 2 max_d |dO_q|) |q| in dK.  (A staircase of 9
              log2 units per chunk over 17 chunks has weights of 2^-144: fp32 itself cannot hold them.)
      dQ <= sum_k E_G |k_kd| + floor + u32 N_ACC(S) sum_k |G||k|;   dK <= sum_q E_G |q_qd| + u32 N_ACC(Lq) sum_q |G||q|;
      dV <= sum_q w (gamma + ln2 (eps_s + bound_LSE2)) |dO| + sum_q w dOerr + u32 N_ACC(Lq) sum_q w |dO|.
  DROP_SPAN: rows whose exponent is more than 60 below the largest live row of their (b, h) may be dropped from dK / dV; the allowance
  is exactly their own contribution (sum over those rows of w |dO| resp. |G||q|), computed here in float64 -- no looser gamma.
"""
import math
from types import SimpleNamespace

import torch

HD = 15
LN2 = math.log(2.0)
U16 = 2.0 ** -11
U32 = 2.0 ** -24
LO_SPAN, P_OFF, P_THR, B_OFF, DROP_SPAN = 6.0, 4.0, 8.0, 6.0, 60
C_DOT = 12.0
GAMMA_F = 2.0 ** -20
GAMMA_DQ = 2.0 ** -20
GAMMA_DKV = 1.25 * 2.0 ** -14
PHI_P = 2.0 ** -28
F64 = torch.float64


def n_acc(n):
    return n / 16.0 + 16.0


def pad_to(n, m):
    return (n + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ operands
def make_rows16(x, ones=False, npad=None):
    """[B][H][N][15] float -> rows16 [B][H][Npad][32] fp16 (hi | lo); ones: 1.0 in channel 15 of the hi part of EVERY row below Npad,
    padded rows included -- the convention of the product's writer (write_operand_formats16 with parts | 8, pinned by
    tests/test_rope_operands_gpu.py); keys >= S are masked by position in the kernels, so the padded ones are never weighted."""
    B, H, N, d = x.shape
    assert d == HD
    npad = pad_to(N, 64) if npad is None else npad
    xd = x.to(F64)
    hi = xd.to(torch.float16)
    lo = (xd - hi.to(F64)).to(torch.float16)
    rows = torch.zeros(B, H, npad, 32, dtype=torch.float16)
    rows[:, :, :N, :HD] = hi
    rows[:, :, :N, 16:16 + HD] = lo
    if ones:
        rows[:, :, :, HD] = 1.0
    return rows


def carried(rows, n=None):
    """The value a rows16 operand carries: hi + lo in float64, [B][H][n][15]."""
    r = rows.to(F64)
    c = r[..., :HD] + r[..., 16:16 + HD]
    return c if n is None else c[:, :, :n]


def rows_to_planes(rows):
    """rows16 [B][H][Npad][32] -> planes16 [B][H][2][16][Npad]."""
    B, H, Np, _ = rows.shape
    return rows.view(B, H, Np, 2, 16).permute(0, 1, 3, 4, 2).contiguous()


def to_kernel_layout(x):
    """[B][H][Lq][15] -> the kernels' O / dO layout [B][Lq][H * 15]."""
    B, H, Lq, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, Lq, H * d).contiguous()


def from_kernel_layout(x, H):
    B, Lq, E = x.shape
    return x.view(B, Lq, H, E // H).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------------------ the operation
def attention(q, k, v, kmask, dO=None, dtype=F64, p_round=None, o_for_d=None, dkv_row_filter=None):
    """Plain softmax attention in log2 units and its gradients, in `dtype`.  q [B,H,Lq,15], k / v [B,H,S,15], kmask [B,S] bool
    (True = masked) or None, dO [B,H,Lq,15].  The three hooks exist for the mutation checks of the CPU file:
    p_round(p, w): replaces the un-normalised weights p = 2^(s2 - m + P_OFF) the PV product and the denominator see;
    o_for_d: D = dO . o_for_d instead of dO . O;  dkv_row_filter(dO): the upstream gradient the dK / dV contraction sees."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    s = q @ k.transpose(-1, -2)
    if kmask is not None:
        s = s.masked_fill(kmask[:, None, None, :], -math.inf)
    m = s.amax(-1, keepdim=True)
    dead = torch.isinf(m)
    m0 = torch.where(dead, torch.zeros_like(m), m)
    p = torch.exp2(s - m0 + P_OFF)
    if p_round is not None:
        p = p_round(p, p / p.sum(-1, keepdim=True).clamp_min(1e-300))
    l = p.sum(-1, keepdim=True)
    ls = torch.where(dead, torch.ones_like(l), l)
    w = p / ls
    o = w @ v
    out = SimpleNamespace(O=o, LSE2=torch.where(dead, torch.full_like(m, -math.inf), m0 - P_OFF + torch.log2(ls)).squeeze(-1), w=w, s=s)
    if dO is not None:
        dO = dO.to(dtype)
        od = o if o_for_d is None else o_for_d.to(dtype)

        def g_of(d):
            return LN2 * w * (d @ v.transpose(-1, -2) - (d * od).sum(-1, keepdim=True))

        G = g_of(dO)
        out.G = G
        out.dQ = G @ k
        dOk = dO if dkv_row_filter is None else dkv_row_filter(dO)
        Gk = G if dkv_row_filter is None else g_of(dOk)
        out.dK = Gk.transpose(-1, -2) @ q
        out.dV = w.transpose(-1, -2) @ dOk
    return out


def reference(q, k, v, kmask, dO=None):
    return attention(q, k, v, kmask, dO, F64)


# ------------------------------------------------------------------------------------------------ bounds
def _wdev(Wt, v, o):
    """sum_k Wt[q, k] |v[k, d] - o[q, d]|  ->  [B,H,Lq,15]"""
    out = torch.empty_like(o)
    for d in range(HD):
        out[..., d] = (Wt * (v[..., None, :, d] - o[..., :, None, d]).abs()).sum(-1)
    return out


def row_exponent(dO):
    """e_q of the prep kernel: max_d |dO ln2| / 2^e in [0.5, 1); None-like -1000 for all-zero rows.  [B,H,Lq] int64"""
    mx = dO.abs().amax(-1) * LN2
    _, e = torch.frexp(mx)
    return torch.where(mx > 0, e.to(torch.int64), torch.full_like(e, -1000, dtype=torch.int64))


def bounds(ref, q, k, v, kmask, dO=None, extra_score_err=None):
    """Component-wise bounds from the float64 reference quantities (module docstring).  Returns a namespace with O, O_adaptive, LSE2,
    LSE2_adaptive and, with dO, dQ, dK, dV, plus dK_dropped / dV_dropped (the DROP_SPAN allowance, zero where nothing may be dropped).
    extra_score_err [B,H,Lq,S] (log2 units, default none): added to eps_s -- the error of a q the kernel under test computes ITSELF
    instead of being handed as an operand (tests/denoise_ref.py: the cross attention of csrc/denoise.hip)."""
    B, H, Lq, _ = q.shape
    S = k.shape[2]
    w, o = ref.w, ref.O
    live = torch.ones(B, 1, 1, S, dtype=F64) if kmask is None else (~kmask)[:, None, None, :].to(F64)
    dead = torch.isinf(ref.LSE2)[..., None]                                         # [B,H,Lq,1]
    s_abs = torch.where(torch.isinf(ref.s), torch.zeros_like(ref.s), ref.s.abs()).amax(-1, keepdim=True)
    A = q.abs() @ k.abs().transpose(-1, -2) + s_abs + P_OFF + P_THR
    eps_s = C_DOT * U32 * A
    if extra_score_err is not None:
        eps_s = eps_s + extra_score_err
    rho = GAMMA_F + LN2 * eps_s
    alive = (~dead).to(F64)
    acc = U32 * n_acc(S) * (w @ v.abs() + o.abs())
    sub = w * (w <= 2.0 ** -LO_SPAN)
    b = SimpleNamespace()
    b.O = _wdev(w * rho + PHI_P * live * alive, v, o) + acc
    b.O_adaptive = b.O + U16 * _wdev(sub, v, o)
    lse = torch.where(dead.squeeze(-1), torch.zeros_like(ref.LSE2), ref.LSE2)
    b.LSE2 = ((w * (GAMMA_F / LN2 + eps_s)).sum(-1) + (PHI_P * live.sum(-1) + U32 * n_acc(S)) / LN2
              + 2.0 ** -22 * (lse.abs() + s_abs.squeeze(-1) + 32.0)) * alive.squeeze(-1)
    b.LSE2_adaptive = b.LSE2 + U16 / LN2 * sub.sum(-1)
    if dO is None:
        return b
    dOa = dO.abs()
    rowmax = dOa.amax(-1, keepdim=True)
    dOerr = 2.0 ** -21 * dOa + 2.0 ** -23 * rowmax
    T = (ref.G / LN2).abs()                                                         # w |dP - D|
    A2 = dOa @ v.abs().transpose(-1, -2) + (dOa * o.abs()).sum(-1, keepdim=True)
    bD = (dOa * b.O).sum(-1, keepdim=True) + (dOerr * o.abs()).sum(-1, keepdim=True) + C_DOT * U32 * (dOa * o.abs()).sum(-1, keepdim=True)
    devO = torch.zeros_like(w)
    for d in range(HD):
        devO += dOerr[..., :, None, d] * (v[..., None, :, d] - o[..., :, None, d]).abs()
    rel = LN2 * (eps_s + b.LSE2[..., None])
    common = LN2 * w * (C_DOT * U32 * A2 + devO + bD)
    EGq = (GAMMA_DQ + rel) * LN2 * T + common
    EGk = (GAMMA_DKV + rel) * LN2 * T + common
    Ga = ref.G.abs()
    b.dQ = (EGq @ k.abs() + 2.0 ** -29 * LN2 * rowmax * alive * (live.permute(0, 1, 3, 2) * k.abs()).sum(-2, keepdim=True)
            + U32 * n_acc(S) * (Ga @ k.abs()))
    # the prep kernel's order: rows sorted by exponent (descending, stable), 64 per chunk, E_c = the chunk's first row
    e = row_exponent(dO)
    e_live = torch.where(dead.squeeze(-1), torch.full_like(e, -1000), e)
    order = torch.sort(-e_live, dim=-1, stable=True).indices
    e_sorted = torch.gather(e_live, -1, order)
    pos = torch.empty_like(order)
    pos.scatter_(-1, order, torch.arange(Lq).expand_as(order).contiguous())
    E_c = torch.gather(e_sorted, -1, pos // 64 * 64)
    phi32 = (torch.exp2((E_c - e_live).clamp(0, 200).to(F64) - 126.0 - B_OFF) * (e_live > -1000))[..., None] * live  # [B,H,Lq,S]
    b.dK = (EGk.transpose(-1, -2) @ q.abs() + U32 * n_acc(Lq) * (Ga.transpose(-1, -2) @ q.abs())
            + LN2 * (phi32 * ((dO @ v.transpose(-1, -2) - (dO * o).sum(-1, keepdim=True)).abs() + 2.0 * rowmax)).transpose(-1, -2) @ q.abs())
    b.dV = ((w * (GAMMA_DKV + rel)).transpose(-1, -2) @ dOa + w.transpose(-1, -2) @ dOerr
            + U32 * n_acc(Lq) * (w.transpose(-1, -2) @ dOa) + phi32.transpose(-1, -2) @ dOa)
    # DROP_SPAN allowance: rows more than 2^60 below the largest LIVE row of their (b, h)
    dropped = ((e < e_live.amax(-1, keepdim=True) - DROP_SPAN) & (e > -1000))[..., None].to(F64)   # [B,H,Lq,1]
    b.n_droppable = int(dropped.sum().item())
    b.dK_dropped = (Ga * dropped).transpose(-1, -2) @ q.abs()
    b.dV_dropped = (w * dropped).transpose(-1, -2) @ dOa
    return b


def ratio(err, bound):
    """max(err / bound) with 0 / 0 = 0 and x / 0 = inf (a zero bound demands an exact result)."""
    err, bound = err.to(F64).abs(), bound.to(F64)
    if not torch.isfinite(err).all():
        return math.inf
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return r.max().item() if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ cases
# One table for the CPU file (fp32 evaluation passes every bound; mutations fail) and the GPU file (the kernels).
#   kind: how q, k, v are generated;  mask: None | "ragged" (ragged tails, sample 0 random holes, LAST sample fully masked,
#   the one before it a single live key);  do: upstream gradient family (None = forward only);  ns: explicit nsplit;
#   lqp: padded query count (default pad to 64);  planes: also run the rows + planes forward.
def _c(name, B, H, Lq, S, kind="rand", gain=1.0, ns=1, mask=None, do="randn", lqp=None, planes=False, seed=0, **kw):
    return SimpleNamespace(name=name, B=B, H=H, Lq=Lq, S=S, kind=kind, gain=gain, ns=ns, mask=mask, do=do, lqp=lqp, planes=planes,
                           seed=seed, kw=kw)


CODOM_S = 3457            # 55 chunks: with nsplit = 3 a split holds 19 chunks, so "chunk c after the split start" exists for c <= 17
CASES = [
    # ---- shapes / dispatch (random logits, gain 1)
    _c("shape_q1_s1", 2, 4, 1, 1),
    _c("shape_q16_s63", 2, 8, 16, 63),
    _c("shape_q17_s64", 2, 4, 17, 64),
    _c("shape_q64_s65_nsfull", 2, 8, 64, 65, ns=2),                      # nsplit = Sp / 64
    _c("shape_q65_s131_ns3", 2, 4, 65, 131, ns=3),
    _c("shape_q128_s1025_emptysplit", 1, 8, 128, 1025, ns=7),           # 17 chunks in 7 splits of 3: the 7th starts at chunk 18 -- empty
    _c("shape_q333_s4097_ns3", 1, 4, 333, 4097, ns=3),
    _c("shape_q333_s1025_nsfull", 1, 4, 333, 1025, ns=17),              # nsplit = Sp / 64 = 17
    _c("shape_q1_s4097_ns64", 2, 4, 1, 4097, ns=64),                    # the C-ABI's largest nsplit: 65 chunks, 2 per split, 31 empty splits
    _c("shape_lqp48", 2, 4, 40, 131, lqp=48, do=None),                  # Lqp % 16 == 0, not % 64 (forward only: the backward needs % 64)
    _c("shape_lqp80_qt2", 2, 4, 70, 131, lqp=80, do=None, ns=2),
    _c("mask_ragged_q37_s131", 4, 4, 37, 131, mask="ragged"),
    _c("mask_ragged_q130_s1025_ns3", 4, 4, 130, 1025, mask="ragged", ns=3),
    _c("planes_q100_s300", 2, 4, 100, 300, planes=True, ns=2),
    _c("kt2_b8_h8_q66_s2000", 8, 8, 66, 2000),                         # B H Sp / 128 = 1024, Lq > 16: KT = 2
    _c("kt1_b1_h8_q66_s2000", 1, 8, 66, 2000),                         # the same keys (sample 0 of the above): KT = 1
    # ---- softmax shape
    _c("gain05", 2, 4, 100, 1025, gain=0.5, ns=2),
    _c("gain3", 2, 4, 100, 1025, gain=3.0, ns=2),
    _c("gain3_q130_s4097", 1, 4, 130, 4097, gain=3.0),
    _c("uniform", 2, 4, 70, 300, kind="uniform"),
    _c("codom_ns1", 18, 2, 20, CODOM_S, kind="codom", start=0),
    _c("codom_ns3", 18, 2, 20, CODOM_S, kind="codom", ns=3, start=19),
    _c("codom_onequery_ns1", 18, 2, 16, CODOM_S, kind="codom", start=0, one_query=5),
    _c("codom_onequery_ns3", 18, 2, 16, CODOM_S, kind="codom", ns=3, start=19, one_query=5),
    _c("rise3", 1, 4, 40, 1025, kind="stairs", step=3.0),
    _c("rise3_ns3", 1, 4, 40, 1025, kind="stairs", step=3.0, ns=3),
    _c("rise9", 1, 4, 80, 1025, kind="stairs", step=9.0),
    _c("fall3", 1, 4, 40, 1025, kind="stairs", step=-3.0),
    _c("spike_tail", 2, 4, 40, 1030, kind="spike", spikes=((1028, 20.0),)),
    _c("spike_after_refresh", 2, 4, 40, 1025, kind="spike", spikes=((9 * 64 + 3, 12.0), (13 * 64 + 40, 30.0))),
    _c("spike_after_refresh_ns3", 2, 4, 40, 1025, kind="spike", spikes=((9 * 64 + 3, 12.0), (13 * 64 + 40, 30.0)), ns=3),
    # ---- upstream gradient
    _c("do_wide", 2, 4, 200, 40, kind="pointer", do="wide"),
    _c("do_span70", 2, 4, 200, 40, kind="pointer", do="span70"),
    _c("do_zero_rows", 2, 4, 100, 131, do="zero_rows", ns=2),
    # ---- forward / backward consistency
    _c("uniform_common_mode", 2, 4, 40, 8, kind="uniform", do="common_mode", kmean=1.0),
    _c("uniform_common_mode_tiny", 2, 4, 2, 3, kind="uniform", do="common_mode", kmean=1.0),
]
CASE_BY_NAME = {c.name: c for c in CASES}
CODOM_CASES = [c.name for c in CASES if c.kind == "codom"]


def _structured(g, B, H, Lq, S, t, b=None, ind=None, qn=0.05):
    """s2[q, k] = t[k] + ind[q] b[k] + noise: channel 0 of q is 1 and of k the profile t, channel 1 holds ind / b, the other 13
    channels small random rows (logit noise of standard deviation qn * sqrt(13))."""
    q = torch.randn(B, H, Lq, HD, generator=g, dtype=F64) * qn
    k = torch.randn(B, H, S, HD, generator=g, dtype=F64)
    q[..., 0] = 1.0
    k[..., 0] = t
    q[..., 1] = 0.0 if ind is None else ind
    k[..., 1] = 0.0 if b is None else b
    return q, k


def build(case):
    """Operands (rows16 fp16 tensors), the carried float64 values, mask, upstream gradient and launch geometry of a case."""
    c = case if not isinstance(case, str) else CASE_BY_NAME[case]
    B, H, Lq, S = c.B, c.H, c.Lq, c.S
    if c.name == "kt1_b1_h8_q66_s2000":                                   # sample 0 of the KT = 2 case
        big = build("kt2_b8_h8_q66_s2000")
        return SimpleNamespace(case=c, B=1, H=H, Lq=Lq, S=S, Lqp=big.Lqp, Sp=big.Sp, ns=c.ns, Qr=big.Qr[:1].contiguous(),
                               Kr=big.Kr[:1].contiguous(), Vr=big.Vr[:1].contiguous(), q=big.q[:1], k=big.k[:1], v=big.v[:1],
                               kmask=None, dO=big.dO[:1].contiguous())
    g = torch.Generator().manual_seed(1000 + 7 * CASES.index(c) + c.seed)
    kw = c.kw
    v = torch.randn(B, H, S, HD, generator=g, dtype=F64)
    if c.kind == "rand":
        q = torch.randn(B, H, Lq, HD, generator=g, dtype=F64) * (c.gain * HD ** -0.5 * math.log2(math.e))
        k = torch.randn(B, H, S, HD, generator=g, dtype=F64) * c.gain
    elif c.kind == "uniform":                                              # all logits within 2^-3
        q = torch.randn(B, H, Lq, HD, generator=g, dtype=F64) * 0.0015
        k = torch.randn(B, H, S, HD, generator=g, dtype=F64) + kw.get("kmean", 0.0)
    elif c.kind == "codom":
        # sample i: key A in the split's first chunk, key B (0.37 below A) in chunk i after it; every other key 30 below (>= 8, and
        # far enough that 3455 of them hold 2e-6 of the mass: the sub-threshold mass is negligible); the two dominant keys hold
        # far-apart values.  one_query: only that query of the 16-query tile sees A and B, the others see near-uniform logits.
        one = kw.get("one_query")
        t = -(torch.rand(B, 1, S, generator=g, dtype=F64)) - (0.0 if one is not None else 30.0)
        bb = torch.zeros(B, 1, S, dtype=F64)
        for i in range(B):
            ia, ib = kw["start"] * 64 + 5, (kw["start"] + i) * 64 + 7
            if one is None:
                t[i, 0, ia], t[i, 0, ib] = 0.0, -0.37
            else:
                t[i, 0, ia], t[i, 0, ib] = 0.0, 0.0
                bb[i, 0, ia], bb[i, 0, ib] = 31.0, 30.63
            v[i, :, ia] = 6.0 + v[i, :, ia]
            v[i, :, ib] = -6.0 + v[i, :, ib]
        ind = None
        if one is not None:
            ind = torch.zeros(1, 1, Lq, dtype=F64)
            ind[..., one] = 1.0
        q, k = _structured(g, B, H, Lq, S, t, bb, ind)
    elif c.kind == "stairs":                                               # each chunk's maximum `step` above the previous one
        t = (torch.arange(S, dtype=F64) // 64) * kw["step"] - torch.rand(S, generator=g, dtype=F64)
        q, k = _structured(g, B, H, Lq, S, t.view(1, 1, S))
    elif c.kind == "spike":
        t = -torch.rand(S, generator=g, dtype=F64)
        for idx, h_ in kw["spikes"]:
            t[idx] = h_
        q, k = _structured(g, B, H, Lq, S, t.view(1, 1, S))
    elif c.kind == "pointer":
        # query i points at key i % S (own score 14.7, the others 14.7 cos(angle): weight > 0.5); channel 0 separates the two halves
        # of the keys by 40 log2 units, so a key of the second half is attended by the queries of the second half ONLY
        k = torch.randn(B, H, S, HD, generator=g, dtype=F64)
        k[..., 0] = 0.0
        k = k / k.norm(dim=-1, keepdim=True) * 3.5
        q = k[:, :, torch.arange(Lq) % S] * 1.2
        k[..., 0] = torch.where(torch.arange(S) < S // 2, 5.0, -5.0).to(F64)
        q[..., 0] = torch.where(torch.arange(Lq) % S < S // 2, 4.0, -4.0).to(F64)
    else:
        raise ValueError(c.kind)
    kmask = None
    if c.mask == "ragged":
        kmask = torch.zeros(B, S, dtype=torch.bool)
        for i in range(1, B):
            kmask[i, S - (i * 37) % (S // 2):] = True
        kmask[0] |= torch.rand(S, generator=g) < 0.3
        kmask[0, 0] = False
        kmask[B - 1] = True                                                # fully masked sample
        kmask[B - 2] = True
        kmask[B - 2, S // 3] = False                                       # a single live key
    Lqp = c.lqp or pad_to(Lq, 64)
    Qr = make_rows16(q, npad=Lqp)
    Kr = make_rows16(k)
    Vr = make_rows16(v, ones=True)
    dO = None
    if c.do is not None:
        dO = torch.randn(B, H, Lq, HD, generator=g, dtype=F64)
        grp = (torch.arange(Lq) % S) * 4 // S if c.kind == "pointer" else None   # key quarter the query points at
        if c.do == "wide":
            # keys of quarters 0, 1: rows at 2^0 .. 2^-5; quarters 2, 3: attended ONLY by small rows, 2^-25 .. 2^-50
            e = torch.where(grp < 2, torch.arange(Lq) % 6, 25 + (torch.arange(Lq) * 7) % 26)
            dO = dO * torch.exp2(-e.to(F64)).view(1, 1, Lq, 1)
        elif c.do == "span70":
            # quarter 3: rows at 2^-70 (beyond DROP_SPAN), quarter 2: 2^-40 .. 2^-50 (inside it), the rest 2^0 .. 2^-5
            e = torch.where(grp == 3, torch.full((Lq,), 70), torch.where(grp == 2, 40 + torch.arange(Lq) % 11, torch.arange(Lq) % 6))
            dO = dO * torch.exp2(-e.to(F64)).view(1, 1, Lq, 1)
        elif c.do == "zero_rows":
            dO[:, :, ::3] = 0.0
            dO[:, 1] = 0.0                                                 # a whole (b, h) without any gradient
        elif c.do == "common_mode":
            dO = 64.0 + dO * 2.0 ** -6
        dO = dO.to(torch.float32).to(F64)                                  # the kernels take fp32 dO: exactly representable
    return SimpleNamespace(case=c, B=B, H=H, Lq=Lq, S=S, Lqp=Lqp, Sp=Kr.shape[2], ns=c.ns, Qr=Qr, Kr=Kr, Vr=Vr,
                           q=carried(Qr, Lq), k=carried(Kr, S), v=carried(Vr, S), kmask=kmask, dO=dO)


_PREPARED = {}


def prepared(name):
    """(operands, float64 reference, bounds) of a case; the last few are kept (the variants of one case run back to back)."""
    if name not in _PREPARED:
        while len(_PREPARED) >= 2:
            _PREPARED.pop(next(iter(_PREPARED)))
        x = build(name)
        ref = reference(x.q, x.k, x.v, x.kmask, x.dO)
        _PREPARED[name] = (x, ref, bounds(ref, x.q, x.k, x.v, x.kmask, x.dO))
    return _PREPARED[name]


# ------------------------------------------------------------------------------------------------ fp16 emulation (mutation checks)
def round16(p):
    return p.to(torch.float16).to(F64)


def two_part16(p):
    hi = round16(p)
    return hi + round16(p - hi)
