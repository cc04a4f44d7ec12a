"""The split-fp16 attention kernels (csrc/attention16.hip) on their own terms: ops.attn_core_fwd / ops.attn_core_bwd on hand-built
operands with an explicit nsplit, against the float64 reference and the DERIVED component-wise bounds of tests/attn16_core_ref.py
(fair and with teeth: tests/test_attn16_core_cpu.py).  No tolerance is chosen here.

Launch variants (attention16.hip, the launch code at the end of the file):
  PP  parts of P in the forward: 3 = both parts everywhere (nograd=False, a backward follows), 2 = adaptive low part (nograd=True)
  QT  16-query tiles per wave of the forward and dQ kernels: 2 when Lq > 64, else 1
  KT  key tiles per wave of the dK / dV kernel: 2 when B H (Sp / 128) >= 1024 and Lq > 16, else 1
  VR  value ROWS (a3d_attn16_fwd_rows, the default operand set) or rows + planes (a3d_attn16_fwd, VR = false: PP = 3 only)
  ns  nsplit > 1: partial results + attn16_combine_kernel (forward), per-split dQ partials summed here in float64

  case                              QT KT  ns  what it reaches
  shape_q1_s1                        1  1   1  one query, one key: 63 padded keys, 63 padded queries
  shape_q16_s63 / q17_s64            1  1   1  H = 8 / 4; exactly one tile / one query into the second tile; S = Sp
  shape_q64_s65_nsfull               1  1   2  nsplit = Sp / 64 (one chunk per split), second chunk holds one key
  shape_q65_s131_ns3                 2  1   3  first QT = 2 size; one chunk per split
  shape_q128_s1025_emptysplit        2  1   7  17 chunks, 3 per split: the LAST SPLIT IS EMPTY (c_beg >= c_end)
  shape_q333_s4097_ns3 / s1025_nsfull 2 1 3/17 the ghost-attention shape; nsplit = Sp / 64 = 17
  shape_q1_s4097_ns64                1  1  64  the C-ABI's largest nsplit: 31 empty splits
  shape_lqp48 / shape_lqp80_qt2      1/2 -  1/2 Lqp % 16 == 0 but not % 64 (forward only; a3d_attn16_bwd requires % 64)
  mask_ragged_*                      1/2 1  1/3 key mask: random holes, ragged tails, ONE LIVE KEY (sample B-2), FULLY MASKED (sample B-1)
  planes_q100_s300                   2  1   2  + the rows + planes forward (VR = false)
  kt2_b8_h8_q66_s2000               2  2   1  the only KT = 2 shape;  kt1_b1_h8_q66_s2000: the same keys at KT = 1
  gain05 / gain3 / gain3_q130_s4097  2  1  2/1 random logits, |log2-logit| up to ~100 at gain 3
  uniform                            2  1   1  all logits within 2^-3
  codom_ns1 / codom_ns3              1  1  1/3 two co-dominant keys with far-apart values; sample i has the second one i chunks after
                                               the split's first chunk, i = 0..17: every phase of the every-8th-chunk threshold refresh
  codom_onequery_*                   1  1  1/3 the same, seen by ONE query of the 16-query tile (the test is wave-uniform)
  rise3 / rise3_ns3 / rise9 / fall3  1/2 1 1/3 staircases: +3 per chunk (a rescale every third chunk, the threshold shifted each time),
                                               +9 per chunk (a rescale on EVERY chunk), -3 per chunk (never)
  spike_tail                         1  1   1  a spike of 2^20 in the last, partly padded chunk
  spike_after_refresh(_ns3)          1  1  1/3 spikes > 2^P_THR above the running maximum after a threshold refresh
  do_wide / do_span70 / do_zero_rows 2  1  1/2 dO rows over 2^0 .. 2^-50 (keys attended only by small rows) / rows at 2^-70 beyond DROP_SPAN /
                                               all-zero rows and a whole (b, h) without gradient
  uniform_common_mode(_tiny)         1  1   1  near-uniform attention, dO = 64 + small: sum_k G = 0 must survive (D against dP)
Every case runs PP = 3 and PP = 2; every case with an upstream gradient runs the backward on the PP = 3 forward's O and LSE2.

Documented padding behaviour, pinned below: O has no padded rows ([B][Lq][E]); LSE2 rows >= Lq are not specified; dQ partial rows of
the 16-query tile that holds the last real query are exact zeros, later rows are never written; dK / dV rows of padded and of masked
keys and channel 15 of every row are exact zeros.  The backward is handed LSE2 with its padded rows set to NaN: they must not be read.
(dO itself is [B][Lq][E] -- the ABI has no padded dO rows to poison.)
The kernels use no float atomics (dQ partials are per split): two launches must agree bit for bit.
"""
import math

import pytest
import torch

import attn16_core_ref as R

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _variants(x):
    qt = 2 if x.Lq > 64 else 1
    kt = 2 if (x.B * x.H * (x.Sp // 128) >= 1024 and x.Lq > 16) else 1
    return qt, kt


def _dev_operands(x, dev, planes=False):
    km = None if x.kmask is None else x.kmask.to(torch.uint8).to(dev)
    V = R.rows_to_planes(x.Vr) if planes else x.Vr
    return x.Qr.to(dev), x.Kr.to(dev), V.to(dev), km


def _forward(a3d, dev, x, nograd, planes=False):
    O_ = a3d.ops
    Q, K, V, km = _dev_operands(x, dev, planes)
    old = O_.ATTN_MODE
    O_.ATTN_MODE = "f16"
    try:
        O, LSE = O_.attn_core_fwd(Q, K, V, km, x.B, x.H, x.Lq, x.Lqp, x.S, x.Sp, x.ns, nograd=nograd)
    finally:
        O_.ATTN_MODE = old
    torch.cuda.synchronize()
    return O, LSE


def _check_forward(x, r, b, O, LSE, adaptive, tag):
    Og = R.from_kernel_layout(O.double().cpu(), x.H)
    Lg = LSE[:, :, :x.Lq].double().cpu()
    dead = torch.isinf(r.LSE2)
    assert torch.isfinite(Og).all(), tag
    assert torch.equal(torch.isinf(Lg) & (Lg < 0), dead), f"{tag}: LSE2 = -inf exactly on the fully masked rows"
    assert torch.isfinite(Lg[~dead]).all(), tag
    ro = R.ratio(Og - r.O, b.O_adaptive if adaptive else b.O)
    rl = R.ratio(torch.where(dead, torch.zeros_like(Lg), Lg - r.LSE2), b.LSE2_adaptive if adaptive else b.LSE2)
    rb = R.ratio(Og - r.O, b.O)
    print(f"[parity] attn16 core {tag}: O max(err/bound)={ro:.3f} (max_abs_err {(Og - r.O).abs().max():.2e}; vs the both-parts bound "
          f"{rb:.3f})  LSE2 max(err/bound)={rl:.3f} (max_abs_err {torch.where(dead, torch.zeros_like(Lg), Lg - r.LSE2).abs().max():.2e})")
    assert ro <= 1.0, (tag, ro)
    assert rl <= 1.0, (tag, rl)
    return Og


# the variants of one case run back to back: its float64 reference (the dominant cost of this file) is computed once
RUNS = [(c.name, v) for c in R.CASES for v in ("fwd-PP3", "fwd-PP2") + (("bwd",) if c.do is not None else ())]


@pytest.mark.parametrize("name,variant", RUNS, ids=[f"{n}-{v}" for n, v in RUNS])
def test_kernels_within_the_derived_bounds(a3d, dev, name, variant):
    if variant == "bwd":
        _backward_case(a3d, dev, name)
    else:
        _forward_case(a3d, dev, name, variant == "fwd-PP2")


def _forward_case(a3d, dev, name, nograd):
    x, r, b = R.prepared(name)
    qt, _ = _variants(x)
    tag = f"fwd {name} PP={2 if nograd else 3} QT={qt} VR=1 nsplit={x.ns} Lqp={x.Lqp}{' masked' if x.kmask is not None else ''}"
    O, LSE = _forward(a3d, dev, x, nograd)
    Og = _check_forward(x, r, b, O, LSE, nograd, tag)
    if nograd and name in R.CODOM_CASES:
        # the promise of the adaptive variant: where the sub-threshold mass is negligible it is as good as both parts everywhere
        one = x.case.kw.get("one_query")
        sel = (lambda t: t) if one is None else (lambda t: t[:, :, one:one + 1])
        rb = R.ratio(sel(Og - r.O), sel(b.O))
        print(f"[parity] attn16 core {tag}: the dominant queries against the BOTH-PARTS bound: max(err/bound)={rb:.3f}")
        assert rb <= 1.0, (tag, rb)


def test_forward_rows_plus_planes_operand_set(a3d, dev):
    """VR = false (a3d_attn16_fwd): the value planes layout [B][H][2][16][Sp]; same bound, and the same bits as the rows launch
    (same fragments, same MFMA order)."""
    x, r, b = R.prepared("planes_q100_s300")
    assert x.case.planes
    O, LSE = _forward(a3d, dev, x, False, planes=True)
    _check_forward(x, r, b, O, LSE, False, f"fwd planes_q100_s300 PP=3 QT=2 VR=0 nsplit={x.ns}")
    O2, LSE2 = _forward(a3d, dev, x, False)
    assert torch.equal(O, O2) and torch.equal(LSE[:, :, :x.Lq], LSE2[:, :, :x.Lq])


def _backward(a3d, dev, x, O, LSE):
    O_ = a3d.ops
    Q, K, V, km = _dev_operands(x, dev)
    dO = R.to_kernel_layout(x.dO).float().to(dev)
    lse_in = LSE.clone()
    lse_in[:, :, x.Lq:] = float("nan")                       # padded rows of LSE2 must not be read
    dQp, dK, dV = O_.attn_core_bwd(Q, K, V, km, O, dO, lse_in, x.B, x.H, x.Lq, x.Lqp, x.S, x.Sp, x.ns, extra=(None, None, V))
    torch.cuda.synchronize()
    return dQp, dK, dV


def _backward_case(a3d, dev, name):
    x, r, b = R.prepared(name)
    qt, kt = _variants(x)
    tag = f"bwd {name} QT={qt} KT={kt} nsplit={x.ns} dO={x.case.do}{' masked' if x.kmask is not None else ''}"
    O, LSE = _forward(a3d, dev, x, False)
    dQp, dK, dV = _backward(a3d, dev, x, O, LSE)
    assert dQp.shape == (x.ns, x.B, x.H, x.Lqp, 16)
    lq16 = R.pad_to(x.Lq, 16)
    dQp, dK, dV = dQp.double().cpu(), dK.double().cpu(), dV.double().cpu()
    assert torch.isfinite(dQp[:, :, :, :lq16]).all() and torch.isfinite(dK).all() and torch.isfinite(dV).all(), tag
    # padding: the rest of the last real 16-query tile, channel 15, padded and masked keys -- exact zeros
    assert (dQp[:, :, :, x.Lq:lq16] == 0).all() and (dQp[:, :, :, :lq16, 15] == 0).all(), tag
    assert (dK[:, :, x.S:] == 0).all() and (dV[:, :, x.S:] == 0).all() and (dK[..., 15] == 0).all() and (dV[..., 15] == 0).all(), tag
    if x.kmask is not None:
        km = x.kmask[:, None, :, None].expand(x.B, x.H, x.S, 16)
        assert (dK[:, :, :x.S][km] == 0).all() and (dV[:, :, :x.S][km] == 0).all(), tag
    dQ = dQp.sum(0)[:, :, :x.Lq, :15]
    rq = R.ratio(dQ - r.dQ, b.dQ)
    rk = R.ratio(dK[:, :, :x.S, :15] - r.dK, b.dK + b.dK_dropped)
    rv = R.ratio(dV[:, :, :x.S, :15] - r.dV, b.dV + b.dV_dropped)
    print(f"[parity] attn16 core {tag}: max(err/bound) dQ={rq:.3f} dK={rk:.3f} dV={rv:.3f}  (max_abs_err dQ {(dQ - r.dQ).abs().max():.2e} of "
          f"{r.dQ.abs().max():.2e}, dK {(dK[:, :, :x.S, :15] - r.dK).abs().max():.2e} of {r.dK.abs().max():.2e}, dV "
          f"{(dV[:, :, :x.S, :15] - r.dV).abs().max():.2e} of {r.dV.abs().max():.2e}; rows beyond DROP_SPAN: {b.n_droppable})")
    assert rq <= 1.0 and rk <= 1.0 and rv <= 1.0, (tag, rq, rk, rv)


def test_known_answer_pins_the_gradient_units_on_the_device(a3d, dev):
    """The hand-derived case of test_attn16_core_cpu.py::test_reference_known_answer_pins_the_units through the kernels: log2 scores,
    ln 2 inside dQ / dK, none in dV, no softmax scale on dQ."""
    q = torch.zeros(1, 1, 1, 15, dtype=F64)
    k = torch.zeros(1, 1, 2, 15, dtype=F64)
    v = torch.zeros(1, 1, 2, 15, dtype=F64)
    dO = torch.zeros(1, 1, 1, 15, dtype=F64)
    q[..., 0], q[..., 1] = 3.0, 1.0
    k[0, 0, 0, :3] = torch.tensor([1.0, 2.0, 5.0], dtype=F64)
    k[0, 0, 1, :3] = torch.tensor([2.0, -1.0, -7.0], dtype=F64)
    v[0, 0, 0, 0] = 1.0
    dO[..., 0] = 1.0
    x = R.SimpleNamespace(B=1, H=1, Lq=1, S=2, Lqp=64, Sp=64, ns=1, Qr=R.make_rows16(q), Kr=R.make_rows16(k),
                          Vr=R.make_rows16(v, ones=True), kmask=None, dO=dO)
    O, LSE = _forward(a3d, dev, x, False)
    dQp, dK, dV = _backward(a3d, dev, x, O, LSE)
    c = math.log(2.0) / 4
    assert abs(O[0, 0, 0].item() - 0.5) < 1e-6 and abs(LSE[0, 0, 0].item() - 6.0) < 1e-5
    assert (dQp[0, 0, 0, 0, :15].double().cpu() - c * (k[0, 0, 0] - k[0, 0, 1])).abs().max() < 1e-5
    assert (dK[0, 0, :2, :15].double().cpu() - torch.stack([c * q[0, 0, 0], -c * q[0, 0, 0]])).abs().max() < 1e-5
    # dV goes through the truncated split-bf16 weights: GAMMA_DKV relative (observed 1.0e-6 of 0.5)
    assert (dV[0, 0, :2, 0].double().cpu() - 0.5).abs().max() <= R.GAMMA_DKV * 0.5 and (dV[0, 0, :2, 1:] == 0).all()


@pytest.mark.parametrize("name", ["mask_ragged_q130_s1025_ns3", "do_wide"])
def test_two_launches_agree_bit_for_bit(a3d, dev, name):
    """No float atomics anywhere in the family (attention16.hip header; the prep kernel's LDS atomics count integers): forward (both
    P variants), dQ partials, dK and dV of two launches on the same inputs are identical."""
    x, _, _ = R.prepared(name)
    lq16 = R.pad_to(x.Lq, 16)
    runs = []
    for _ in range(2):
        O, LSE = _forward(a3d, dev, x, False)
        O2, _ = _forward(a3d, dev, x, True)
        dQp, dK, dV = _backward(a3d, dev, x, O, LSE)
        runs.append((O, LSE[:, :, :x.Lq], O2, dQp[:, :, :, :lq16], dK, dV))
    for a, b_, what in zip(runs[0], runs[1], ("O", "LSE2", "O (adaptive)", "dQ partials", "dK", "dV")):
        assert torch.equal(a, b_), f"{name}: {what} differs between two launches"
