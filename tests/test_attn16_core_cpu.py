"""The float64 reference and the derived bounds of tests/attn16_core_ref.py have teeth -- no GPU, no code under test.

 * reference() equals torch.autograd on a plain float64 softmax attention (masks and fully masked rows included) and a hand-derived
   known answer that pins the unit conventions (log2 scores, ln 2 inside the gradients, no q scale);
 * the operand builders carry what they are given;
 * FAIR: for every case of tests/test_attn16_core_gpu.py (same generators, same seeds) a plain fp32 torch evaluation of the carried
   operands passes every bound;
 * TEETH: four kernel defects, emulated in float64, each fail the bound they target on a case built for them.
"""
import math

import pytest
import torch

import attn16_core_ref as R

F64 = torch.float64


def _autograd(q, k, v, kmask, dO):
    q, k, v = (t.clone().requires_grad_() for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * math.log(2.0)                   # 2^s2 = e^(s2 ln2)
    if kmask is not None:
        s = s.masked_fill(kmask[:, None, None, :], -math.inf)
    dead = torch.isinf(s).all(-1, keepdim=True)
    w = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    o = w @ v
    (o * dO).sum().backward()
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("masked", [False, True])
def test_reference_gradients_equal_autograd(masked):
    g = torch.Generator().manual_seed(3)
    B, H, Lq, S = 3, 2, 9, 21
    q, k, v = (torch.randn(B, H, n, 15, generator=g, dtype=F64) for n in (Lq, S, S))
    dO = torch.randn(B, H, Lq, 15, generator=g, dtype=F64)
    kmask = None
    if masked:
        kmask = torch.rand(B, S, generator=g) < 0.4
        kmask[1] = True                                            # a fully masked sample
        kmask[2] = True
        kmask[2, 4] = False                                        # a single live key
    r = R.reference(q, k, v, kmask, dO)
    o, dq, dk, dv = _autograd(q, k, v, kmask, dO)
    for name, got, want in (("O", r.O, o), ("dQ", r.dQ, dq), ("dK", r.dK, dk), ("dV", r.dV, dv)):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), name
    if masked:
        assert torch.isinf(r.LSE2[1]).all() and (r.LSE2[1] < 0).all()
        for t in (r.O[1], r.dQ[1], r.dK[1], r.dV[1]):
            assert (t == 0).all()
        assert (r.LSE2[2] - (q[2] @ k[2, :, 4:5].transpose(-1, -2)).squeeze(-1)).abs().max() < 1e-12      # one key: LSE2 = its score


def test_reference_known_answer_pins_the_units():
    """One query, two keys with equal scores, v0 = e0, v1 = 0, dO = e0:  w = (1/2, 1/2), O = e0 / 2, LSE2 = s + 1 (log2 units),
    dP = (1, 0), D = 1/2, G = ln2 * (1/4, -1/4), dQ = ln2 / 4 (k0 - k1), dK = +- ln2 / 4 q, dV = (e0 / 2, e0 / 2): the ln 2 is inside,
    no softmax scale is applied to dQ."""
    q = torch.zeros(1, 1, 1, 15, dtype=F64)
    k = torch.zeros(1, 1, 2, 15, dtype=F64)
    v = torch.zeros(1, 1, 2, 15, dtype=F64)
    dO = torch.zeros(1, 1, 1, 15, dtype=F64)
    q[..., 0], q[..., 1] = 3.0, 1.0
    k[0, 0, 0, :3] = torch.tensor([1.0, 2.0, 5.0], dtype=F64)
    k[0, 0, 1, :3] = torch.tensor([2.0, -1.0, -7.0], dtype=F64)     # both scores 5
    v[0, 0, 0, 0] = 1.0
    dO[..., 0] = 1.0
    r = R.reference(q, k, v, None, dO)
    e0 = torch.zeros(15, dtype=F64)
    e0[0] = 1.0
    assert torch.equal(r.O[0, 0, 0], e0 / 2) and r.LSE2.item() == 6.0
    c = math.log(2.0) / 4
    assert torch.allclose(r.dQ[0, 0, 0], c * (k[0, 0, 0] - k[0, 0, 1]), rtol=0, atol=1e-15)
    assert torch.allclose(r.dK[0, 0], torch.stack([c * q[0, 0, 0], -c * q[0, 0, 0]]), rtol=0, atol=1e-15)
    assert torch.equal(r.dV[0, 0], torch.stack([e0 / 2, e0 / 2]))


def test_operand_builders_carry_what_they_are_given():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 37, 15, generator=g, dtype=F64) * 4
    rows = R.make_rows16(x, ones=True)
    assert rows.shape == (2, 3, 64, 32) and rows.dtype == torch.float16
    c = R.carried(rows, 37)
    # two roundings to half an fp16 ulp; below 2^-14 fp16 is subnormal (spacing 2^-24), which caps the low part's accuracy
    assert ((c - x).abs() <= 2.0 ** -22 * x.abs() + 2.0 ** -25).all()
    # the writers' convention: the 1.0 of the denominator channel sits on every row below Npad, padded rows are zero otherwise
    assert (rows[:, :, :, 15] == 1).all() and (rows[:, :, 37:, :15] == 0).all() and (rows[:, :, 37:, 16:] == 0).all() and (rows[:, :, :, 31] == 0).all()
    grid = torch.randint(-2048, 2049, (2, 3, 37, 15), generator=g).to(F64) / 64      # on the fp16 grid: carried exactly
    rg = R.make_rows16(grid)
    assert torch.equal(R.carried(rg, 37), grid) and (rg[..., 16:] == 0).all()
    pl = R.rows_to_planes(rows)
    assert pl.shape == (2, 3, 2, 16, 64)
    assert torch.equal(pl[1, 2, 0, :, 5], rows[1, 2, 5, :16]) and torch.equal(pl[1, 2, 1, :, 5], rows[1, 2, 5, 16:])
    assert torch.equal(R.from_kernel_layout(R.to_kernel_layout(x), 3), x)


def test_case_constructions_have_the_properties_their_names_claim():
    x, r, _ = R.prepared("uniform")
    assert (r.s.amax(-1) - r.s.amin(-1)).max().item() < 2.0 ** -3
    for name in ("uniform_common_mode", "uniform_common_mode_tiny"):
        x, r, _ = R.prepared(name)
        assert (r.s.amax(-1) - r.s.amin(-1)).max().item() < 2.0 ** -3
    for name in R.CODOM_CASES:
        x, r, _ = R.prepared(name)
        one = x.case.kw.get("one_query")
        w = r.w if one is None else r.w[:, :, one:one + 1]
        top2 = w.topk(2, -1).values
        assert (top2[..., 1] > 0.25).all(), name                                     # two co-dominant keys ...
        assert ((w * (w <= 2.0 ** -6)).sum(-1) < 1e-5).all(), name                   # ... and a negligible sub-threshold mass
        ia = x.case.kw["start"] * 64 + 5
        for i in range(x.B):                                                         # sample i: the second key sits i chunks later
            idx = set(w[i, 0, 0].topk(2).indices.tolist())
            assert idx == {ia, ia + i * 64 + 2}, (name, i, idx)
    x, r, b = R.prepared("do_wide")
    e = R.row_exponent(x.dO)
    attended = r.w > 0.5
    small_only = (attended & (e[..., None] < -20)).any(2) & ~(attended & (e[..., None] >= -20)).any(2)
    assert small_only.sum(-1).min().item() >= 5                                       # keys that only rows 2^-20 and below attend
    assert e.max().item() - e.min().item() >= 45 and b.n_droppable == 0
    x, r, b = R.prepared("do_span70")
    assert b.n_droppable > 0 and (b.dV_dropped.amax(-1) > 0).any()


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_fp32_evaluation_passes_every_bound(name):
    """Fairness: plain fp32 torch on the same carried operands is inside every bound, so no bound asks for more than fp32 gives and
    the inputs are well enough conditioned for the comparison to mean something."""
    x, r, b = R.prepared(name)
    f = R.attention(x.q, x.k, x.v, x.kmask, x.dO, dtype=torch.float32)
    dead = torch.isinf(r.LSE2)
    assert torch.equal(torch.isinf(f.LSE2), dead)
    rat = {"O": R.ratio(f.O - r.O, b.O), "LSE2": R.ratio(torch.where(dead, torch.zeros_like(r.LSE2), f.LSE2.to(F64) - r.LSE2), b.LSE2)}
    if x.dO is not None:
        rat.update(dQ=R.ratio(f.dQ - r.dQ, b.dQ), dK=R.ratio(f.dK - r.dK, b.dK), dV=R.ratio(f.dV - r.dV, b.dV))
    print(f"[bounds] fp32 evaluation of {name}: max(err / bound) " + " ".join(f"{k}={v:.3f}" for k, v in rat.items()))
    assert all(v <= 1.0 for v in rat.values()), rat


def _fails(name, what, err, bound):
    rr = R.ratio(err, bound)
    print(f"[bounds] mutation on {name}: {what} max(err / bound) = {rr:.2f}")
    return rr > 1.0


def test_mutation_single_part_p_fails_the_both_parts_forward_bound():
    """P rounded to ONE fp16 part everywhere (the A3D_ATTN_FAST kernel) must not pass as the both-parts kernel."""
    failed = []
    for name in ("gain3", "rise3", "uniform") + tuple(R.CODOM_CASES):
        x, r, b = R.prepared(name)
        mut = R.attention(x.q, x.k, x.v, x.kmask, p_round=lambda p, w: R.round16(p))
        if _fails(name, "single-part P vs the both-parts bound on O:", mut.O - r.O, b.O):
            failed.append(name)
    print("[bounds] single-part P fails on:", failed)
    assert "gain3" in failed and set(R.CODOM_CASES) <= set(failed), failed


def test_mutation_adaptive_p_dropping_a_codominant_low_part_fails_the_adaptive_bound():
    """Only the largest key of a query keeps both parts: the second co-dominant key (w > 0.25 >> 2^-6) loses its low part.  The correct
    adaptive rule (both parts for w > 2^-6), emulated the same way, passes the adaptive AND the both-parts bound on the same cases."""
    failed = []
    for name in R.CODOM_CASES:
        x, r, b = R.prepared(name)
        one = x.case.kw.get("one_query")
        sel = (lambda t: t) if one is None else (lambda t: t[:, :, one:one + 1])
        good = R.attention(x.q, x.k, x.v, x.kmask, p_round=lambda p, w: torch.where(w > 2.0 ** -6, R.two_part16(p), R.round16(p)))
        assert R.ratio(good.O - r.O, b.O_adaptive) <= 1.0 and R.ratio(sel(good.O - r.O), sel(b.O)) <= 1.0, name
        mut = R.attention(x.q, x.k, x.v, x.kmask,
                          p_round=lambda p, w: torch.where(w >= w.amax(-1, keepdim=True), R.two_part16(p), R.round16(p)))
        if _fails(name, "low part dropped for the second co-dominant key vs the adaptive bound on O:", mut.O - r.O, b.O_adaptive):
            failed.append(name)
    assert failed == R.CODOM_CASES, failed


def test_mutation_flushing_small_do_rows_fails_the_wide_range_backward():
    """dK / dV with the dO rows 2^-20 below the largest row of their (b, h) flushed to zero (one fp16 exponent range for all rows)."""
    x, r, b = R.prepared("do_wide")

    def flush(dO):
        mx = dO.abs().amax(-1, keepdim=True)
        return torch.where(mx < 2.0 ** -20 * mx.amax(-2, keepdim=True), torch.zeros_like(dO), dO)

    mut = R.attention(x.q, x.k, x.v, x.kmask, x.dO, dkv_row_filter=flush)
    assert R.ratio(mut.dQ - r.dQ, b.dQ) <= 1.0                                        # dQ is per row: untouched
    assert _fails("do_wide", "flushed rows vs the dV bound:", mut.dV - r.dV, b.dV + b.dV_dropped)
    assert _fails("do_wide", "flushed rows vs the dK bound:", mut.dK - r.dK, b.dK + b.dK_dropped)


def test_mutation_d_from_a_single_part_p_output_fails_the_common_mode_backward():
    """D = dO . O~ with O~ off by the single-part-P rounding (forward and backward disagreeing about O): sum_k G_qk = 0 breaks, which
    shows along the mean key in dQ and as a common factor in dK."""
    fq, fk = [], []
    for name in ("uniform_common_mode", "uniform_common_mode_tiny"):
        x, r, b = R.prepared(name)
        o_mut = R.attention(x.q, x.k, x.v, x.kmask, p_round=lambda p, w: R.round16(p)).O
        mut = R.attention(x.q, x.k, x.v, x.kmask, x.dO, o_for_d=o_mut)
        if _fails(name, "D from a single-part-P output vs the dQ bound:", mut.dQ - r.dQ, b.dQ):
            fq.append(name)
        if _fails(name, "D from a single-part-P output vs the dK bound:", mut.dK - r.dK, b.dK + b.dK_dropped):
            fk.append(name)
    assert fq and fk, (fq, fk)
