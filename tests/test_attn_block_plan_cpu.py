"""ops.attn_block_plan on the host: which launches serve one attention block, decided from the mode, the shapes, the module switches
and the library's size queries alone (no GPU, nothing launched).  The expected routes and lists are written out by hand from the
rules of the code the plan replaced, not produced by the function:

  family        split-fp16 operands unless ATTN_MODE is "bf16x3" or a backward would follow with ceil64(Lq) > ATTN16_BWD_MAX_LQP (the
                fp16 backward's query limit); "fp8" names the e4m3 forward core, which only a gradient-free, dropout-free forward takes
  operand set   rows only with ROWS_ONLY, except under ATTN_MODE "fp8" (attention8 packs its value operand from planes) and in the
                bf16x3 family (always rows + planes)
  projection    "context" when the caller supplies the k | v rows (mode "kv" only); fused when FUSED_PROJ and E % 4 == 0 and E <= 128
  forward       per group one a3d_proj_rope_split[16]; unfused: per group one a3d_linear_fwd, then per role one a3d_rope_split[16];
                the core; the out-projection (the residual dropout folded into it with DROP_FOLD); a3d_add_layernorm_fwd
  backward      LayerNorm: E <= 64 and E % 4 == 0 with DEFER_REDUCE -> a3d_add_layernorm_bwd_partials (+ its own table launch when no
                queue takes the records) + a3d_dropout; else a3d_add_layernorm_bwd[_drop].  Out-projection dgrad and wgrad, the core,
                then per group: one a3d_rope_merge_bwd per role, the weight gradient (two-stage from 1024 rows: a3d_linear_wgrad_partials
                when a queue takes the reduction, else a3d_linear_wgrad_ws), one a3d_linear_fwd when an input of the group needs a
                gradient.  A group parked in a sink (CTX_DEFER) issues only its rotations.
"""
import pytest

from conftest import load_pkg

P16, P, S16, S = "a3d_proj_rope_split16", "a3d_proj_rope_split", "a3d_rope_split16", "a3d_rope_split"
LIN, LIN_DROP, DROPOUT, LNF = "a3d_linear_fwd", "a3d_linear_fwd_drop", "a3d_dropout", "a3d_add_layernorm_fwd"
ROWS, F16, F8, BF, BF_DROP = "a3d_attn16_fwd_rows", "a3d_attn16_fwd", "a3d_attn8_fwd", "a3d_attn_fwd", "a3d_attn_fwd_dropout"
B16, BBF, BBF_DROP = "a3d_attn16_bwd", "a3d_attn_bwd_bf16", "a3d_attn_bwd_bf16_dropout"
LNB, LNB_DROP, LNP = "a3d_add_layernorm_bwd", "a3d_add_layernorm_bwd_drop", "a3d_add_layernorm_bwd_partials"
TABLE = ["a3d_grad_reduce_table_plan", "a3d_grad_reduce_table_upload", "a3d_grad_reduce_table"]
MERGE, WS, PART = "a3d_rope_merge_bwd", "a3d_linear_wgrad_ws", "a3d_linear_wgrad_partials"

SHAPES = {"kv": (2, 37, 131, 60, 4), "qk": (2, 16, 16, 120, 8), "none": (1, 5, 64, 60, 4)}
# default switches, every input needs a gradient, no queue
FWD = {"kv": [P16, P16, ROWS, LIN, LNF], "qk": [P16, P16, ROWS, LIN, LNF], "none": [P16, P16, P16, ROWS, LIN, LNF]}
UNFUSED = {"kv": [LIN, LIN, S16, S16, S16], "qk": [LIN, LIN, S16, S16, S16], "none": [LIN, LIN, LIN, S16, S16, S16]}
LN60, LN120 = [LNP] + TABLE, [LNB]                                        # E = 60: per-workgroup partials; E = 120: the atomics kernel
BWD = {
    "kv": LN60 + [LIN, WS, B16] + [MERGE, WS, LIN] + [MERGE, MERGE, WS, LIN],
    "qk": LN120 + [LIN, WS, B16] + [MERGE, MERGE, WS, LIN] + [MERGE, WS, LIN],
    "none": LN60 + [LIN, WS, B16] + [MERGE, WS, LIN] + [MERGE, WS, LIN] + [MERGE, WS, LIN],
}
MODES = list(SHAPES)


@pytest.fixture()
def O(monkeypatch):
    ops = load_pkg().ops
    for k, v in dict(ATTN_MODE="f16", ROWS_ONLY=True, FUSED_PROJ=True, DROP_FOLD=True, DEFER_REDUCE=True, CTX_DEFER=True,
                     ATTN16_BWD_MAX_LQP=7296).items():
        monkeypatch.setattr(ops, k, v)                                  # the defaults, whatever the environment says
    return ops


def swap(names, **to):
    return [to.get(n, n) for n in names]


def route_of(r):
    return r.family, r.operands, r.projection, r.core_fwd, r.core_bwd


def test_group_table_and_its_pointer_arithmetic(O):
    assert O.PROJ_GROUPS == {"kv": ((0, 0, ("q",)), (1, 1, ("k", "v"))),
                             "qk": ((0, 0, ("q", "k")), (2, 2, ("v",))),
                             "none": ((0, 0, ("q",)), (1, 1, ("k",)), (2, 2, ("v",)))}
    # (weight byte offset, bias byte offset, column byte offsets, leading dimension) of fp32 [3E][E] / [3E] / [rows][len(roles) E]
    assert O.group_layout(1, ("k", "v"), 60) == (60 * 60 * 4, 60 * 4, (0, 240), 120)                  # "kv": k | v of the context
    assert O.group_layout(0, ("q", "k"), 120) == (0, 0, (0, 480), 240)                               # "qk": q | k of the query
    assert O.group_layout(2, ("v",), 120) == (2 * 120 * 120 * 4, 960, (0,), 120)
    assert O.group_layout(1, ("k",), 60) == (14400, 240, (0,), 60)                                   # "none": k alone


@pytest.mark.parametrize("mode", MODES)
def test_default_route(O, mode):
    r = O.attn_block_plan(mode, *SHAPES[mode])
    assert route_of(r) == ("f16", "rows", "fused", ROWS, B16)
    assert r.nsplit == {"kv": 3, "qk": 1, "none": 1}[mode]               # min(16, Sp // 64, ...): 192 // 64 keys splits, else one
    assert r.groups == O.PROJ_GROUPS[mode] and r.f16
    assert r.launches_forward() == FWD[mode]
    assert r.launches_backward() == BWD[mode]


@pytest.mark.parametrize("mode", MODES)
def test_unfused_projection(O, monkeypatch, mode):
    monkeypatch.setattr(O, "FUSED_PROJ", False)
    r = O.attn_block_plan(mode, *SHAPES[mode])
    assert route_of(r) == ("f16", "rows", "unfused", ROWS, B16)
    assert r.launches_forward() == UNFUSED[mode] + [ROWS, LIN, LNF]
    assert r.launches_backward() == BWD[mode]


@pytest.mark.parametrize("mode", MODES)
def test_rows_and_planes_operand_set(O, monkeypatch, mode):
    monkeypatch.setattr(O, "ROWS_ONLY", False)
    r = O.attn_block_plan(mode, *SHAPES[mode])
    assert route_of(r) == ("f16", "rows+planes", "fused", F16, B16)
    assert r.launches_forward() == swap(FWD[mode], **{ROWS: F16})
    assert r.launches_backward() == BWD[mode]


@pytest.mark.parametrize("mode", MODES)
def test_bf16x3_family(O, monkeypatch, mode):
    monkeypatch.setattr(O, "ATTN_MODE", "bf16x3")
    r = O.attn_block_plan(mode, *SHAPES[mode])
    assert route_of(r) == ("bf16x3", "rows+planes", "fused", BF, BBF) and not r.f16
    assert r.launches_forward() == swap(FWD[mode], **{P16: P, ROWS: BF})
    assert r.launches_backward() == swap(BWD[mode], **{B16: BBF})
    monkeypatch.setattr(O, "FUSED_PROJ", False)
    assert O.attn_block_plan(mode, *SHAPES[mode]).launches_forward() == swap(UNFUSED[mode], **{S16: S}) + [BF, LIN, LNF]


@pytest.mark.parametrize("mode", MODES)
def test_fp8_serves_only_gradient_free_dropout_free_forwards(O, monkeypatch, mode):
    monkeypatch.setattr(O, "ATTN_MODE", "fp8")
    shape = SHAPES[mode]
    r = O.attn_block_plan(mode, *shape, need_bwd=False)
    assert route_of(r) == ("fp8", "rows+planes", "fused", F8, None)
    assert r.launches_forward() == swap(FWD[mode], **{ROWS: F8}) and r.launches_backward() == []
    r = O.attn_block_plan(mode, *shape, need_bwd=True)                   # a backward follows: the split-fp16 kernels on the planes set
    assert route_of(r) == ("f16", "rows+planes", "fused", F16, B16)
    assert r.launches_forward() == swap(FWD[mode], **{ROWS: F16}) and r.launches_backward() == BWD[mode]
    r = O.attn_block_plan(mode, *shape, need_bwd=False, dropping=True)
    assert route_of(r) == ("f16", "rows+planes", "fused", F16, None)
    assert r.launches_forward() == swap(FWD[mode], **{ROWS: F16, LIN: LIN_DROP})
    r = O.attn_block_plan(mode, *shape, need_bwd=True, dropping=True)
    assert route_of(r) == ("f16", "rows+planes", "fused", F16, B16)


@pytest.mark.parametrize("mode", MODES)
def test_no_backward(O, mode):
    r = O.attn_block_plan(mode, *SHAPES[mode], need_bwd=False)
    assert route_of(r) == ("f16", "rows", "fused", ROWS, None)
    assert r.launches_forward() == FWD[mode] and r.launches_backward() == []


@pytest.mark.parametrize("mode", MODES)
def test_dropout(O, monkeypatch, mode):
    shape = SHAPES[mode]
    ln = {60: [LNP] + TABLE + [DROPOUT], 120: [LNB_DROP]}[shape[3]]      # the partials kernel has no dropout form
    r = O.attn_block_plan(mode, *shape, dropping=True)
    assert route_of(r) == ("f16", "rows", "fused", ROWS, B16)
    assert r.launches_forward() == swap(FWD[mode], **{LIN: LIN_DROP})
    assert r.launches_backward() == ln + BWD[mode][len(LN60 if shape[3] == 60 else LN120):]
    monkeypatch.setattr(O, "DROP_FOLD", False)                           # separate a3d_dropout launches
    ln = {60: [LNP] + TABLE + [DROPOUT], 120: [LNB, DROPOUT]}[shape[3]]
    r = O.attn_block_plan(mode, *shape, dropping=True)
    assert r.launches_forward() == FWD[mode][:-2] + [LIN, DROPOUT, LNF]
    assert r.launches_backward() == ln + BWD[mode][len(LN60 if shape[3] == 60 else LN120):]
    monkeypatch.setattr(O, "DROP_FOLD", True)
    monkeypatch.setattr(O, "ATTN_MODE", "bf16x3")
    r = O.attn_block_plan(mode, *shape, dropping=True)
    assert route_of(r) == ("bf16x3", "rows+planes", "fused", BF_DROP, BBF_DROP)
    assert r.launches_forward() == swap(FWD[mode], **{P16: P, ROWS: BF_DROP, LIN: LIN_DROP})


def test_reductions_in_place_without_defer_reduce(O, monkeypatch):
    monkeypatch.setattr(O, "DEFER_REDUCE", False)
    assert O.attn_block_plan("kv", *SHAPES["kv"]).launches_backward() == [LNB] + BWD["kv"][len(LN60):]
    assert O.attn_block_plan("kv", *SHAPES["kv"], dropping=True).launches_backward() == [LNB_DROP] + BWD["kv"][len(LN60):]


def test_context_operands(O):
    r = O.attn_block_plan("kv", *SHAPES["kv"], kv_pair=True)
    assert route_of(r) == ("f16", "rows", "context", ROWS, B16)
    assert r.groups == (O.PROJ_GROUPS["kv"][0],)                         # only the q group is written
    assert r.launches_forward() == [P16, ROWS, LIN, LNF]
    assert r.launches_backward() == BWD["kv"]
    for mode in ("qk", "none"):
        with pytest.raises(RuntimeError, match=r"AttnBlockFn: precomputed context operands need the packed k,v projection \(key is value\)"):
            O.attn_block_plan(mode, *SHAPES[mode], kv_pair=True)


def test_sink(O, monkeypatch):
    head = LN60 + [LIN, WS, B16] + [MERGE, WS, LIN]
    for kv_pair in (False, True):
        r = O.attn_block_plan("kv", *SHAPES["kv"], sink=True, kv_pair=kv_pair)
        assert r.sink and r.launches_backward() == head + [MERGE, MERGE]    # parked: both GEMMs of the group are the gate's
    monkeypatch.setattr(O, "CTX_DEFER", False)
    assert O.attn_block_plan("kv", *SHAPES["kv"], sink=True).launches_backward() == head + [MERGE, MERGE, WS, LIN]
    monkeypatch.setattr(O, "CTX_DEFER", True)
    # a sink is taken only by the packed k,v projection of a context that needs a gradient, in a pass a backward follows
    assert not O.attn_block_plan("qk", *SHAPES["qk"], sink=True).sink
    assert not O.attn_block_plan("none", *SHAPES["none"], sink=True).sink
    assert not O.attn_block_plan("kv", *SHAPES["kv"], sink=True, needs=(True, False, False, True)).sink
    assert not O.attn_block_plan("kv", *SHAPES["kv"], sink=True, need_bwd=False).sink
    assert O.attn_block_plan("qk", *SHAPES["qk"], sink=True).launches_backward() == BWD["qk"]


def test_q_is_resid_and_which_inputs_need_gradients(O, monkeypatch):
    for mode in MODES:                                                   # the fold is the same launch, added into the LayerNorm's dS
        assert O.attn_block_plan(mode, *SHAPES[mode], q_is_resid=True).launches_backward() == BWD[mode]
    g = O._group_grad_route
    assert g(("q",), (True, True, True, True), False, True) == "fold" and g(("q", "k"), (False, True, False, True), False, True) == "fold"
    assert g(("q",), (True, True, True, True), False, False) == "fresh" and g(("k", "v"), (True, True, True, True), False, True) == "fresh"
    assert g(("k", "v"), (True, True, False, True), True, False) == "parked" and g(("q",), (False, True, True, True), True, True) is None
    monkeypatch.setattr(O, "CTX_DEFER", False)
    assert g(("k", "v"), (True, True, False, True), True, False) == "sink"
    head = LN60 + [LIN, WS, B16]
    r = O.attn_block_plan("kv", *SHAPES["kv"], needs=(False, True, False, False))
    assert r.launches_backward() == head + [MERGE, WS] + [MERGE, MERGE, WS, LIN]
    r = O.attn_block_plan("kv", *SHAPES["kv"], needs=(False, False, False, False))      # only the parameters: no input-gradient GEMM
    assert r.launches_backward() == head + [MERGE, WS] + [MERGE, MERGE, WS]
    r = O.attn_block_plan("none", *SHAPES["none"], needs=(True, False, True, False))
    assert r.launches_backward() == head + [MERGE, WS, LIN] + [MERGE, WS] + [MERGE, WS, LIN]
    r = O.attn_block_plan("qk", *SHAPES["qk"], needs=(False, True, False, False))        # the q | k group serves either of its inputs
    assert r.launches_backward() == BWD["qk"][:-1]


def test_long_queries_fall_to_the_bf16_family(O, monkeypatch):
    B, _, S, E, H = SHAPES["kv"]
    assert route_of(O.attn_block_plan("kv", B, 7296, S, E, H))[:2] == ("f16", "rows")
    r = O.attn_block_plan("kv", B, 7297, S, E, H)                         # ceil64 = 7360 > 7296: 12 B per query no longer fit the LDS sort
    assert route_of(r) == ("bf16x3", "rows+planes", "fused", BF, BBF)
    assert route_of(O.attn_block_plan("kv", B, 7297, S, E, H, need_bwd=False)) == ("f16", "rows", "fused", ROWS, None)
    monkeypatch.setattr(O, "ATTN16_BWD_MAX_LQP", 0)
    r = O.attn_block_plan("kv", *SHAPES["kv"])
    assert route_of(r) == ("bf16x3", "rows+planes", "fused", BF, BBF)
    assert r.launches_forward() == swap(FWD["kv"], **{P16: P, ROWS: BF}) and r.launches_backward() == swap(BWD["kv"], **{B16: BBF})
    assert route_of(O.attn_block_plan("kv", *SHAPES["kv"], need_bwd=False)) == ("f16", "rows", "fused", ROWS, None)


def test_wide_embedding_is_unfused(O):
    r = O.attn_block_plan("kv", 2, 37, 131, 132, 4)                      # 132 % 4 == 0 but not <= 128
    assert route_of(r) == ("f16", "rows", "unfused", ROWS, B16)
    assert r.launches_forward() == UNFUSED["kv"] + [ROWS, LIN, LNF]
    assert r.launches_backward() == [LNB] + BWD["kv"][len(LN60):]        # E > 64: the atomics LayerNorm backward
    assert O.attn_block_plan("kv", 2, 37, 131, 128, 4).projection == "fused"
    assert O.attn_block_plan("kv", 2, 37, 131, 126, 4).projection == "unfused"          # E % 4 != 0


def test_reduce_queue_and_two_stage_weight_gradients(O):
    B, Lq, S, E, H = 8, 37, 131, 60, 4                                   # 8 * 131 = 1048 context rows: two-stage; 296 query rows: one-stage
    kv_tail = [MERGE, WS, LIN] + [MERGE, MERGE]
    assert O.attn_block_plan("kv", B, Lq, S, E, H).launches_backward() == LN60 + [LIN, WS, B16] + kv_tail + [WS, LIN]
    r = O.attn_block_plan("kv", B, Lq, S, E, H, queue=True)              # the queue takes the LayerNorm records and the two-stage reduce
    assert r.launches_backward() == [LNP] + [LIN, WS, B16] + kv_tail + [PART, LIN]
    r = O.attn_block_plan("kv", B, 128, S, E, H, queue=True)             # 1024 query rows: out-projection and q group two-stage as well
    assert r.launches_backward() == [LNP] + [LIN, PART, B16] + [MERGE, PART, LIN] + [MERGE, MERGE, PART, LIN]
    r = O.attn_block_plan("kv", B, 127, S, E, H, queue=True)             # 1016 rows: one below the threshold
    assert r.launches_backward() == [LNP] + [LIN, WS, B16] + [MERGE, WS, LIN] + [MERGE, MERGE, PART, LIN]
