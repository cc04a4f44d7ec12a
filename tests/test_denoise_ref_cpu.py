"""tests/denoise_ref.py is right, fair and has teeth -- without a GPU.

  * known answers of each float64 reference (one key: O = v; equal logits: the mean; identity weights pass rows through; all keys masked: 0);
  * the local reference functions agree with oracle.blocks (parallel_attention_layer, mlp2 under LIFT = float64);
  * the fp32 twin (the same function in fp32 on the CPU; for the cross attention the kernel's arithmetic restated in fp32 with fp16 P)
    passes every bound of every case tests/test_denoise_kernels_gpu.py asserts on the device;
  * every mutated twin fails its bound on a named case;
  * the cross case table covers the wave ranges the streaming loop distinguishes;
  * the C-ABI refuses the arguments the kernels cannot serve (the library loads without a GPU; nothing is launched).
"""
import ctypes
import math

import pytest
import torch

import attn16_core_ref as C
import denoise_ref as DR
import rope_ref as R

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answer_one_key_gives_its_value():
    x = DR.build_cross("keys_s1_sp64_ns1")
    r = DR.cross_reference(x)
    assert torch.equal(r.O, x.v.expand(-1, -1, 1, -1).expand_as(r.O))
    q = torch.randn(2, 5, 30, dtype=F64)
    kv = torch.randn(2, 1, 30, dtype=F64)
    assert torch.equal(DR.attention(q, kv, kv, 2, None, F64), kv.expand(2, 5, 30))


def test_known_answer_equal_logits_give_the_mean():
    x = DR.build_cross("score_flat")
    r = DR.cross_reference(x)
    s = r.ref.s
    assert (s.amax(-1) - s.amin(-1)).max() < 1e-12 and abs(s.mean().item() - 3.0) < 1e-5        # the profile, in log2 units
    assert (r.O - x.v.mean(2, keepdim=True)).abs().max() < 1e-12
    q = torch.zeros(2, 5, 30, dtype=F64)
    k, v = torch.randn(2, 9, 30, dtype=F64), torch.randn(2, 9, 30, dtype=F64)
    assert (DR.attention(q, k, v, 2, None, F64) - v.mean(1, keepdim=True)).abs().max() < 1e-14


def test_known_answer_all_keys_masked_give_zero():
    q, k, v = (torch.randn(2, 5, 30, dtype=F64) for _ in range(3))
    km = torch.zeros(2, 5, dtype=torch.bool)
    km[0] = True
    o = DR.attention(q, k, v, 2, km, F64)
    assert (o[0] == 0).all() and torch.isfinite(o).all() and (o[1] != 0).any()
    Op, Mp = torch.randn(3, 1, 2, 16, 16, dtype=F64), torch.randn(3, 1, 2, 16, dtype=F64)
    Op[..., 15] = 2.0
    Mp[:, 0, 0] = -math.inf
    Mp[1, 0, 1] = -math.inf
    o = DR.combine_partials(Op, Mp)
    assert (o[0, 0] == 0).all()
    w = torch.exp(Mp[[0, 2], 0, 1] - Mp[[0, 2], 0, 1].amax(0))
    want = (w[..., None] * Op[[0, 2], 0, 1, :, :15]).sum(0) / (2.0 * w.sum(0))[..., None]
    assert (o[0, 1] - want).abs().max() < 1e-14
    Op[..., 15] = 0.0                                                       # a zero denominator
    assert (DR.combine_partials(Op, Mp) == 0).all()


def test_known_answer_identity_weights_pass_rows_through():
    x = DR.build_rest("no_ffn")
    x.case = DR.SimpleNamespace(**{**vars(x.case), "sa": False, "ffn": False})
    x.p.c_out_w, x.p.c_out_b = torch.eye(x.E), torch.zeros(x.E)
    x.p.c_ln_g, x.p.c_ln_b = torch.ones(x.E), torch.zeros(x.E)
    o = R.unheads(DR.combine_partials(x.Op, x.Mp)[:, :, :x.L])
    assert (o[0, :, :15] == 0).all()                                        # head 0 of sample 0: every split at -inf
    want = torch.nn.functional.layer_norm(x.x.to(F64) + o, (x.E,))
    assert torch.equal(DR.rest_forward(x, F64), want)
    t = DR.build_tail("sched_e30_d9_l16_rows_row0_terminal")
    t.p.pos_w1.zero_(), t.p.rot_w1.zero_()
    t.p.cond_mask = None
    want = torch.cat((t.traj[..., :3].to(F64) + t.p.pos_b1.to(F64), t.p.rot_b1.to(F64).expand(t.B, t.L, t.D - 3)), -1)
    assert torch.equal(DR.tail_forward(t, F64), want)
    h = DR.build_head("e30_d9_l1_nolang")
    h.p.enc_w1, h.p.enc_b1 = torch.eye(h.E), torch.zeros(h.E)
    assert torch.equal(DR.head_forward(h, F64), torch.relu(DR.linear(h.traj.to(F64), h.p.enc_w0, h.p.enc_b0, F64)))


def test_references_agree_with_the_oracle_blocks():
    """cross + rest against oracle.blocks.parallel_attention_layer and the tail's regressors against mlp2, both in float64 (the oracle's
    RoPE tables are fp32 values: agreement to 1e-6 of scale, far below any structural difference)."""
    from oracle import blocks as OB
    x = DR.build_rest("kmask_last3")
    B, L, E, H, S = x.B, x.L, x.E, x.H, 37
    g = torch.Generator().manual_seed(5)
    ctx, cxyz = torch.randn(B, S, E, generator=g), torch.rand(B, S, 3, generator=g)
    cw, cb, cmod = DR._w(g, 3 * E, E), DR._b(g, 3 * E, E), DR._mod(g, E)
    # this module's route: q as the cross kernel forms it, k / v as the cache holds them, partials of one split
    q = DR.rope(DR.linear(DR.adaln(x.x.to(F64) + x.sem.to(F64), cmod, F64), cw[:E], cb[:E], F64) * DR.Q_SCALE, x.traj, x.freq, F64)
    k = DR.rope(DR.linear(ctx.to(F64), cw[E:2 * E], cb[E:2 * E], F64), cxyz, x.freq, F64)
    v = DR.linear(ctx.to(F64), cw[2 * E:], cb[2 * E:], F64)
    O = R.heads(DR.attention(q, k, v, H, None, F64), H)
    x.Op = torch.zeros(1, B, H, 16, 16, dtype=F64)
    x.Op[0, :, :, :L, :15], x.Op[..., 15] = O, 1.0
    x.Mp = torch.zeros(1, B, H, 16, dtype=F64)
    got = DR.rest_forward(x, F64)
    p = x.p
    pre = "l"
    P = {f"{pre}.cross_12.in_proj_weight": cw, f"{pre}.cross_12.in_proj_bias": cb, f"{pre}.cross_12.out_proj.weight": p.c_out_w,
         f"{pre}.cross_12.out_proj.bias": p.c_out_b, f"{pre}.norm_12.weight": p.c_ln_g, f"{pre}.norm_12.bias": p.c_ln_b,
         f"{pre}.sa1.in_proj_weight": p.s_in_w, f"{pre}.sa1.in_proj_bias": p.s_in_b, f"{pre}.sa1.out_proj.weight": p.s_out_w,
         f"{pre}.sa1.out_proj.bias": p.s_out_b, f"{pre}.norm_1.weight": p.s_ln_g, f"{pre}.norm_1.bias": p.s_ln_b,
         f"{pre}.ffn_12.0.weight": p.f_w1, f"{pre}.ffn_12.0.bias": p.f_b1, f"{pre}.ffn_12.3.weight": p.f_w2, f"{pre}.ffn_12.3.bias": p.f_b2,
         f"{pre}.norm_122.weight": p.f_ln_g, f"{pre}.norm_122.bias": p.f_ln_b}
    for name, mod in (("adaln_12", cmod), ("adaln_1", p.s_mod), ("adaln_ff1", p.f_mod)):      # Linear(SiLU(t)) with zero weights: mod = bias
        P[f"{pre}.{name}.modulation.1.weight"] = torch.zeros(2 * E, 4)
        P[f"{pre}.{name}.modulation.1.bias"] = mod
    P = {n: t.to(F64) for n, t in P.items()}
    keep = OB.LIFT
    OB.LIFT = F64
    try:
        want = OB.parallel_attention_layer(P, pre, x.x.to(F64), x.kmask, ctx.to(F64), H, seq1_xyz=x.traj[..., :3], seq2_xyz=cxyz,
                                           seq1_sem=x.sem.to(F64)[None], ada=torch.zeros(B, 4, dtype=F64))
        t = DR.build_tail("e120_d9_l16_rows_t5")
        TP = {"r.0.weight": t.p.pos_w0, "r.0.bias": t.p.pos_b0, "r.2.weight": t.p.pos_w1, "r.2.bias": t.p.pos_b1}
        pos = OB.mlp2(t.pos_feats.to(F64), {n: w.to(F64) for n, w in TP.items()}, "r")
    finally:
        OB.LIFT = keep
    assert DR.rel_err(got, want) < 1e-6, DR.rel_err(got, want)
    assert DR.rel_err(DR.tail_network_output(t, F64)[..., :3] - t.traj[..., :3].to(F64), pos) < 1e-12


# ------------------------------------------------------------------------------------------------ the twins pass
_CROSS = {}


def _cross(name):
    if name not in _CROSS:
        x = DR.build_cross(name)
        _CROSS[name] = (x, DR.cross_reference(x))
    return _CROSS[name]


@pytest.mark.parametrize("name", [c.name for c in DR.CROSS_CASES])
def test_cross_twin_within_the_derived_bound(name):
    x, r = _cross(name)
    ratio = C.ratio(DR.cross_twin(x) - r.O, r.bound)
    assert ratio <= 1.0, (name, ratio)
    assert (r.bound >= r.bound_no_extra).all()


@pytest.mark.parametrize("kind,name", [(k, c.name) for k, cs in (("rest", DR.REST_CASES), ("head", DR.HEAD_CASES), ("tail", DR.TAIL_CASES))
                                       for c in cs])
def test_dense_twin_inside_its_own_rule(kind, name):
    """err(twin) <= max(2^-20, 4 err(twin)) is trivially true; what this pins is that the twin is an fp32-grade evaluation (the rule's
    right-hand side stays within 2^-18: a kernel cannot hide a structural error behind a sloppy twin) and that the case is not degenerate."""
    x, ref, e = DR.prepared(kind, name)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0.1
    assert 0 < DR.twin_limit(e) <= 2.0 ** -18, (name, e)


def test_tail_clamp_matters():
    for c in DR.TAIL_CASES:
        if c.L == 16:
            frac = (DR.tail_network_output(DR.build_tail(c.name), F64).abs() > 1).double().mean().item()
            assert 0.2 < frac < 0.5, (c.name, frac)


# ------------------------------------------------------------------------------------------------ mutations
def test_mutation_p_low_part_dropped():
    """One-part fp16 P for every key is what the kernel is ALLOWED where every key is below 2^-LO_SPAN (flat): inside the bound there,
    outside it as soon as a key dominates."""
    x, r = _cross("score_flat")
    assert C.ratio(DR.cross_twin(x, p_mode="drop_lo") - r.O, r.bound) <= 1.0
    failed = [n for n in ("score_dominant_between_refreshes", "score_creep", "keys_s31_sp64_ns1")
              if C.ratio(DR.cross_twin(_cross(n)[0], p_mode="drop_lo") - _cross(n)[1].O, _cross(n)[1].bound) > 1.0]
    assert failed == ["score_dominant_between_refreshes", "keys_s31_sp64_ns1"], failed     # creep: ~700 keys share the mass, all below 2^-6


def test_mutation_keys_masked_at_sp():
    x, r = _cross("keys_s65_sp256_ns1")
    assert C.ratio(DR.cross_twin(x, mask_at="Sp") - r.O, r.bound) > 100
    x, r = _cross("keys_s64_sp64_ns1")                                    # nothing to mask: the same mutation is harmless
    assert C.ratio(DR.cross_twin(x, mask_at="Sp") - r.O, r.bound) <= 1.0


def test_mutation_cross_rope_axis_and_adaln_swap():
    x, r = _cross("heads_e60")
    assert C.ratio(DR.cross_twin(x, axis_mode="mod3") - r.O, r.bound) > 100
    assert C.ratio(DR.cross_twin(x, swap=True) - r.O, r.bound) > 100


REST_MUTATIONS = [("kmask_shift", "kmask_last3"), ("kmask_shift", "kmask_all_but_row0"), ("sem_in_v", "e60_f240"), ("ffn_res_x", "e60_f240"),
                  ("adaln_swap", "e120_f480"), ("adaln_swap", "no_self_attention"), ("ln_eps", "e30_f30"), ("ln_eps", "no_ffn"),
                  ("rope_axis", "e90_f100"), ("rope_axis", "d10_e30")]


@pytest.mark.parametrize("mut,name", REST_MUTATIONS)
def test_mutation_rest(mut, name):
    x, ref, e = DR.prepared("rest", name)
    em = DR.rel_err(DR.rest_forward(x, F32, mut=(mut,)), ref)
    assert em > DR.twin_limit(e), (mut, name, em, DR.twin_limit(e))


def test_mutation_head_ln_eps():
    x, ref, e = DR.prepared("head", "e60_d16_l16_s53")
    assert DR.rel_err(DR.head_forward(x, F32, mut=("ln_eps",)), ref) > DR.twin_limit(e)


@pytest.mark.parametrize("mut,name", [("clamp_first", "e120_d9_l16_rows_t5"), ("clamp_first", "sched_e120_d4_l16_scatter_row3"),
                                      ("terminal_coef", "e30_d9_l16_scatter_t0_terminal"),
                                      ("terminal_coef", "sched_e120_d9_l1_last_row_terminal")])
def test_mutation_tail(mut, name):
    x, ref, e = DR.prepared("tail", name)
    em = DR.rel_err(DR.tail_forward(x, F32, mut=(mut,)), ref)
    assert em > DR.twin_limit(e), (mut, name, em)


# ------------------------------------------------------------------------------------------------ wave ranges
def test_cross_case_table_covers_the_wave_ranges():
    lengths, dead, into_dead = set(), False, False
    for c in DR.CROSS_CASES:
        for hb, he in DR.wave_ranges(c.Sp, c.ns):
            lengths.add(he - hb)
            if he > hb and hb * 32 >= c.S:
                dead = True                                                # the whole range lies in the padding
            if he > hb and hb * 32 < c.S and (he - 1) * 32 >= c.S:
                into_dead = True                                           # begins on valid keys, runs into a dead half
    assert {0, 1, 2, 3, 4, 5} <= lengths and any(9 <= n < 32 for n in lengths) and any(n >= 32 for n in lengths), sorted(lengths)
    assert dead and into_dead
    listed = {he - hb for S, Sp, ns in DR.KEY_COUNT_LIST for hb, he in DR.wave_ranges(Sp, ns)}
    assert listed == {0, 1, 2, 3, 4, 5, 8, 9, 32, 33}, sorted(listed)
    # the remainders of the 3-deep unrolled loop
    assert {n % 3 for n in lengths} == {0, 1, 2}


def test_score_cases_hit_the_branches_they_are_named_for():
    """In log2 units, per wave range of the nsplit = 1 launch: what the lazy maximum of dn_stream_consume sees."""
    rng = DR.wave_ranges(1088, 1)

    def profile(name):
        x, r = _cross(name)
        return r.ref.s[0, 0, 0]                                            # every row and head sees the same profile

    def excess(s, hb, he):                                                 # per half: its maximum above the maximum of the halves before it
        mx = [s[h * 32:(h + 1) * 32].max().item() for h in range(hb, min(he, (1025 + 31) // 32))]
        return [mx[i] - max(mx[:i]) for i in range(1, len(mx))]

    s = profile("score_staircase")
    assert all(all(e > C.P_THR for e in excess(s, hb, he)) for hb, he in rng)             # a rescale in every half
    s = profile("score_creep")
    ex = [excess(s, hb, he) for hb, he in rng]
    assert all(max(e) < C.P_THR for e in ex) and all(max(e) > 6.0 for e in ex)            # a large rise, never a rescale
    s = profile("score_spike_late")
    hb, he = rng[1]
    assert excess(s, hb, he)[-1] > 39.0 and max(excess(s, hb, he)[:-1]) < 1.0
    s = profile("score_dominant_between_refreshes")
    hb, he = rng[2]
    w = _cross("score_dominant_between_refreshes")[1].ref.w[0, 0, 0]
    assert w.argmax().item() // 32 == hb + 5 and w.max() > 2.0 ** -C.LO_SPAN and (w > 2.0 ** -C.LO_SPAN).sum() == 2
    w = _cross("score_flat")[1].ref.w
    assert (w < 2.0 ** -C.LO_SPAN).all()
    w = _cross("score_two_scales")[1].ref.w[0, 0, 0]
    assert (w[1::2].max() / w[0::2].max()) < 2.0 ** -28                                    # under fp16's subnormal floor relative to p = 16


# ------------------------------------------------------------------------------------------------ argument refusals
ERR_ARG = -22
PTR = 0x1000                                       # a non-null pointer no refused call dereferences


def _params(a3d, cls, **kw):
    p = cls()
    for n, t in cls._fields_:
        setattr(p, n, PTR if t is ctypes.c_void_p else 0)
    for n, v in kw.items():
        setattr(p, n, v)
    return p


def _refused(a3d, name, *args):
    lib = a3d.lib.load()
    rc = getattr(lib, name)(*args)
    msg = lib.a3d_last_error_string()
    assert rc == ERR_ARG and name.encode() in msg, (name, rc, msg)


def test_argument_refusals(a3d):
    L_ = a3d.lib
    cp = ctypes.byref(_params(a3d, L_.DnCrossParams))
    B, L, E, H, D = 1, 16, 60, 4, 9

    def cross(D=D, E=E, H=H, S=65, Sp=128, ns=1):
        _refused(a3d, "a3d_dn_cross", PTR, PTR, D, cp, PTR, B, L, E, H, S, Sp, ns, None)

    cross(Sp=96)                                   # Sp % 64 != 0
    cross(S=129)                                   # Sp < S
    cross(ns=0)
    cross(ns=65)
    cross(D=2)
    cross(E=45, H=3)
    cross(E=126, H=8)

    def rest(D=D, L=L, E=E, H=H, **kw):
        rp = _params(a3d, L_.DnRestParams, F=kw.pop("F", 240), **kw)
        _refused(a3d, "a3d_dn_rest", PTR, PTR, D, PTR, ctypes.byref(rp), PTR, B, L, E, H, 1, None)

    rest(F=513)
    rest(L=7, D=23)                                # L * D = 161 > the 160-float staging area
    rest(s_out_w=None)                             # s_in_w without s_out_w
    rest(E=45, H=3)
    rest(E=126, H=8)

    def head(D=D, E=E, H=H, S_lang=53):
        hp = _params(a3d, L_.DnHeadParams, S_lang=S_lang)
        _refused(a3d, "a3d_dn_head", PTR, D, ctypes.byref(hp), PTR, B, L, E, H, None)

    head(D=17)
    head(E=45, H=3)
    head(E=126, H=8)
    assert DR.max_s_lang(120) == 124 and DR.max_s_lang(30) == 499
    for E_ in (30, 60, 120):
        head(E=E_, H=E_ // 15, S_lang=DR.max_s_lang(E_) + 1)           # the first S_lang that no longer fits
        assert DR.max_s_lang(E_) * 8 * E_ + DR.HEAD_STATIC_BYTES <= DR.HEAD_LDS_BYTES < (DR.max_s_lang(E_) + 1) * 8 * E_ + DR.HEAD_STATIC_BYTES
