"""The attention-block cases shared by tests/test_attn_block_plan_gpu.py and profiles/attn_block_plan_equivalence.py: the smallest
shapes that reach every branch of ops.AttnBlockFn, each under the switch values that apply to it, and one runner that records the entry
names of the forward and of the backward at lib.call and returns every tensor the block computes.

  "kv"    B=2, Lq=37, S=131, E=60, H=4    partial query and key tiles, RoPE; alone: context operands, sink, reduce queue
  "qk"    B=2, Lq=S=16, E=120, H=8        masked keys, RoPE
  "none"  B=1, Lq=5, S=64, E=60, H=4      three inputs, no RoPE
"""
import torch

SHAPES = {"kv": (2, 37, 131, 60, 4), "qk": (2, 16, 16, 120, 8), "none": (1, 5, 64, 60, 4)}
GATE_PARKED = ["a3d_linear_fwd", "a3d_linear_wgrad_ws"]                  # what the sink's gate issues for one parked block (M < 1024)
TABLE_FLUSH = ["a3d_grad_reduce_table_plan", "a3d_grad_reduce_table_upload", "a3d_grad_reduce_table"]


def case(name, mode, switches=None, p=0.0, grad=True, kv_pair=False, sink=False, q_is_resid=False, queue=False, after=()):
    """switches: attributes of ops set for the case; p: dropout probability; grad: a backward follows; after: the launches that are
    recorded behind the block's backward and are not its own (the sink gate's, the reduce queue's flush)."""
    return dict(name=name, mode=mode, switches=dict(switches or {}), p=p, grad=grad, kv_pair=kv_pair, sink=sink, q_is_resid=q_is_resid,
                queue=queue, after=list(after))


# every mode under every switch value of tests/test_attn_block_plan_cpu.py that is not tied to the context ("kv") alone
FP8, BF16X3, LONG = dict(ATTN_MODE="fp8"), dict(ATTN_MODE="bf16x3"), dict(ATTN16_BWD_MAX_LQP=0)
CASES = []
for m in SHAPES:
    CASES += [
        case(m + " default", m),
        case(m + " unfused", m, dict(FUSED_PROJ=False)),
        case(m + " rows+planes", m, dict(ROWS_ONLY=False)),
        case(m + " bf16x3", m, BF16X3),
        case(m + " bf16x3 unfused", m, dict(BF16X3, FUSED_PROJ=False)),
        case(m + " no grad", m, grad=False),
        case(m + " fp8", m, FP8),
        case(m + " fp8 no grad", m, FP8, grad=False),                    # the only forward a3d_attn8_fwd serves
        case(m + " fp8 dropout", m, FP8, p=0.1),
        case(m + " fp8 dropout no grad", m, FP8, p=0.1, grad=False),
        case(m + " dropout", m, p=0.1),
        case(m + " dropout unfolded", m, dict(DROP_FOLD=False), p=0.1),
        case(m + " bf16x3 dropout", m, BF16X3, p=0.1),
        case(m + " long query", m, LONG),                                # the bf16x3 family through the fp16 backward's query limit
        case(m + " long query no grad", m, LONG, grad=False),
        case(m + " q is resid", m, q_is_resid=True),
    ]
CASES += [
    case("kv context operands", "kv", kv_pair=True),
    case("kv context operands, sink", "kv", kv_pair=True, sink=True, after=GATE_PARKED),
    case("kv sink", "kv", sink=True, after=GATE_PARKED),
    case("kv sink undeferred", "kv", dict(CTX_DEFER=False), sink=True),
    case("kv no immediate reductions", "kv", dict(DEFER_REDUCE=False)),
    case("kv reduce queue", "kv", queue=True, after=TABLE_FLUSH),
]
CACHED_SHAPE = (2, 8, 70, 120, 8)                                          # kv_cache_build + attn_block_cached


def recorded(a3d, fn):
    """(entry names fn() launches, in order, recorded at lib.call as in test_backbone_plan_gpu.py; fn's result)"""
    seen, call = [], a3d.lib.call
    a3d.ops.L.call = lambda entry, *args: (seen.append(entry), call(entry, *args))[1]
    try:
        result = fn()
    finally:
        a3d.ops.L.call = call
    return seen, result


def modules(dev, E, H, seed=0):
    """(mha, norm) with the attributes ops.attn_block reads, biases and the norm away from their trivial initial values"""
    torch.manual_seed(seed)
    mha, norm = torch.nn.MultiheadAttention(E, H), torch.nn.LayerNorm(E)
    for p in list(mha.parameters()) + list(norm.parameters()):
        if p.dim() == 1:
            torch.nn.init.normal_(p, mean=1.0 if p is norm.weight else 0.0, std=0.5)
    return mha.to(dev), norm.to(dev)


def run_case(a3d, dev, c):
    """One attn_block forward (and backward) of case c under the switches ALREADY set by the caller -> dict(fwd, bwd: the recorded
    entry names; plan: the arguments for ops.attn_block_plan; tensors: {name: tensor} of y and every gradient)."""
    O = a3d.ops
    B, Lq, S, E, H = SHAPES[c["mode"]]
    mha, norm = modules(dev, E, H)
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    leaves = {"q_in": rnd(B, Lq, E).requires_grad_(c["grad"])}
    q_in = leaves["q_in"]
    if c["mode"] == "qk":
        k_in = q_in
    else:
        k_in = leaves["k_in"] = rnd(B, S, E).requires_grad_(c["grad"])
    if c["mode"] == "kv":
        v_in = k_in
    else:
        v_in = leaves["v_in"] = rnd(B, S, E).requires_grad_(c["grad"])
    if c["q_is_resid"]:
        resid = q_in
    else:
        resid = leaves["resid"] = rnd(B, Lq, E).requires_grad_(c["grad"])
    q_xyz = k_xyz = kmask = None
    if c["mode"] != "none":
        q_xyz = (torch.rand(B, Lq, 3, generator=g) * 2 - 0.5).to(dev)
        k_xyz = q_xyz if c["mode"] == "qk" else (torch.rand(B, S, 3, generator=g) * 2 - 0.5).to(dev)
    if c["mode"] == "qk":
        kmask = torch.zeros(B, S, dtype=torch.bool)
        kmask[1, -3:] = True
        kmask = kmask.to(dev)
    dy = rnd(B, Lq, E)
    drop = O.DropCtx(torch.tensor([1234, 0], dtype=torch.int64, device=dev), c["p"]) if c["p"] > 0 else None
    O.ReduceQueue.current = None
    if c["queue"]:
        O.begin_grad_sinks()                                      # as Act3D.forward: this is where the queue is created
    sink, pair = None, None
    if c["sink"]:
        k_in = v_in = O.attach_grad_sink(k_in * 1.0, [])          # a non-leaf context behind the gate node that owns the sink
        sink = k_in._a3d_sink
    if c["kv_pair"]:
        assert O.ctx_kv_applicable(k_in, k_xyz, [mha], H, Lq)
        with torch.no_grad():
            pair = O.ctx_kv_operands16(k_in, k_xyz, [mha], H)[0]
    with torch.set_grad_enabled(c["grad"]):
        fwd, y = recorded(a3d, lambda: O.attn_block(q_in, k_in, v_in, resid, q_xyz, k_xyz, kmask, mha, norm, H, drop=drop, site=8,
                                                    sink=sink, kv_pair=pair))
    tensors = {"y": y.detach()}
    bwd = None
    if c["grad"]:
        bwd, _ = recorded(a3d, lambda: y.backward(dy))
        tensors.update({"d_" + n: t.grad for n, t in leaves.items()})
        tensors.update({"g_in_proj_weight": mha.in_proj_weight.grad, "g_in_proj_bias": mha.in_proj_bias.grad,
                        "g_out_proj_weight": mha.out_proj.weight.grad, "g_out_proj_bias": mha.out_proj.bias.grad,
                        "g_norm_weight": norm.weight.grad, "g_norm_bias": norm.bias.grad})
    torch.cuda.synchronize()
    O.ReduceQueue.current = None
    plan = dict(mode=c["mode"], B=B, Lq=Lq, S=S, E=E, H=H, need_bwd=c["grad"], dropping=c["p"] > 0, kv_pair=c["kv_pair"], sink=c["sink"],
                q_is_resid=c["q_is_resid"], needs=(c["grad"],) * 4, queue=c["queue"])
    return dict(fwd=fwd, bwd=bwd, plan=plan, tensors=tensors)


def run_cached(a3d, dev):
    """kv_cache_build + attn_block_cached at CACHED_SHAPE under the switches already set -> (build launches, block launches, y)"""
    O = a3d.ops
    B, Lq, S, E, H = CACHED_SHAPE
    mha, norm = modules(dev, E, H, seed=3)
    g = torch.Generator().manual_seed(12)
    q_in, k_in, resid = (torch.randn(B, n, E, generator=g).to(dev) for n in (Lq, S, Lq))
    q_xyz, k_xyz = ((torch.rand(B, n, 3, generator=g) * 2 - 0.5).to(dev) for n in (Lq, S))
    build, cache = recorded(a3d, lambda: O.kv_cache_build(k_in, k_xyz, mha, H))
    block, y = recorded(a3d, lambda: O.attn_block_cached(q_in, resid, q_xyz, cache, mha, norm, H))
    torch.cuda.synchronize()
    return build, block, y
