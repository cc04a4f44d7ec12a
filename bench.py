#!/usr/bin/env python3
"""bench.py -- Act3D keypose training step (BASELINE.json configs[1]) on N MI355X GPUs of one node.

  python bench.py --gpus 1 --steps 20 --warmup 5                  the headline step only: set up, warm up, time, print
  python bench.py --gpus 1 --steps 20 --warmup 5 --full           + every other leg (sequential step, hot path only, kernel
                                                                  rooflines, `secondary` workloads, CPU baseline)
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs D what the last timed step computed, as D/<name>.npy
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

One step = zero_grad + forward (frozen synthetic CLIP-RN50-shaped backbone, FPN, coarse-to-fine ghost-point
attention) + loss + backward + fused AdamW (+ gradient all-reduce over RCCL for N > 1), on a synthetic batch of the
18-PerAct-task shapes: 4 cameras 256x256, 3 ghost-point levels, 1000 ghost points, E=60.  Prints ONE JSON line.
`value` = keyframe samples/s over all ranks; inputs are resident in HBM before the timed region.  Inputs, initial weights
and the device sampler are seeded: the same arguments give the same inputs in every run.  The backward kernels accumulate
with atomics and AdamW's first steps are sign-like, so two runs of ONE build drift apart step by step: after 25 steps the
dumped parameters of two such runs differed by 4e-3 of their norm and the loss by 13 % (9.10 vs 7.89), after 105 steps the
loss by 0.5 %; the first step's loss is bit-identical.  Compare builds against that spread.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# The frozen backbone of the NEXT batch runs on a side stream inside the current step's graph (engine.GraphedStep(prefetch=...)): every
# timed step still executes one backbone pass, one FPN / hot-path forward + backward and one AdamW step; the backbone pass it executes
# belongs to the batch the next step consumes (the maps the first timed step reads come from the last warm-up step, the maps the last
# timed step writes are read after the timed region: K timed steps = K backbone passes + K of everything else).  The line also
# carries `sequential_step` under --full: the same K steps with the backbone inside its own step (A3D_PREFETCH_BACKBONE=0 makes that the headline).
PREFETCH_BACKBONE = os.environ.get("A3D_PREFETCH_BACKBONE", "1") == "1"
PERACT_BOUNDS = np.array([[-0.1101, -0.5558, 0.7129], [0.6481, 0.5184, 1.5116]])


def synthetic_batch(B, ncam, device, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.tensor(PERACT_BOUNDS[0], dtype=torch.float32)
    hi = torch.tensor(PERACT_BOUNDS[1], dtype=torch.float32)
    rgbs = torch.rand(B, ncam, 3, 256, 256, generator=g)
    coarse = torch.rand(B, ncam, 3, 16, 16, generator=g)
    base = torch.nn.functional.interpolate(coarse.flatten(0, 1), scale_factor=16, mode="nearest").view(B, ncam, 3, 256, 256)
    base = (base + 0.05 * torch.randn(B, ncam, 3, 256, 256, generator=g)).clamp(0, 1)
    pcds = lo.view(1, 1, 3, 1, 1) + base * (hi - lo).view(1, 1, 3, 1, 1)
    shrink = 0.1 * (hi - lo)

    def pose():
        xyz = lo + shrink + torch.rand(B, 3, generator=g) * (hi - lo - 2 * shrink)
        q = torch.randn(B, 4, generator=g)
        q = q / q.norm(dim=-1, keepdim=True)
        return torch.cat([xyz, q, torch.randint(0, 2, (B, 1), generator=g).float()], -1)

    s = {"rgbs": rgbs, "pcds": pcds, "curr_gripper": pose(), "action": pose(), "instr": torch.randn(B, 53, 512, generator=g),
         "task": ["synthetic"] * B}
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in s.items()}


def build_model(a3d, device, backbone_dtype, levels=3, ghost_points=1000):
    torch.manual_seed(0)
    m = a3d.Act3D(backbone="clip", image_size=(256, 256), embedding_dim=60, num_attn_heads=4,
                  gripper_loc_bounds=PERACT_BOUNDS, num_ghost_points=ghost_points, num_ghost_points_val=10000,
                  num_sampling_level=levels, weight_tying=True, gp_emb_tying=True, use_instruction=False)
    m.to(device)
    m.backbone_dtype = backbone_dtype
    m.fpn_dtype = backbone_dtype
    m.train()
    return m


MIOPEN_DB = os.path.join(ROOT, "profiles", "miopen_db")


def prepare_convolution_search():
    """Keeps MIOpen's find mode (torch.backends.cudnn.benchmark) from dominating the set-up.  The frozen backbone / FPN run 16
    convolution problems through MIOpen; searched from nothing, find mode spent 90 s on them at the first forward / backward:
      * it compiles and times the naive direct solvers (ConvDirectNaiveConv{Fwd,Bwd,Wrw}: reference implementations, 140 - 1900 ms
        per call where the chosen implicit-GEMM solvers take 0.02 - 0.45 ms).  They are never picked; they are excluded;
      * it searches the kernel instance of every tunable solver.  profiles/miopen_db/ holds the user find database and user
        performance database one such search wrote (solver ranking and kernel instance per problem; names carry the MIOpen version,
        another version ignores them and searches).  MIOpen gets a temporary copy as its user database directory, so it neither
        writes into the tree nor depends on the home directory.
    The solvers picked are the ones the full search picks.  Anything already set in the environment wins."""
    for d in ("FWD", "BWD", "WRW"):
        os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + d, "0")
    if "MIOPEN_USER_DB_PATH" not in os.environ and os.path.isdir(MIOPEN_DB):
        import atexit
        import shutil
        import tempfile
        tmp = tempfile.mkdtemp(prefix="a3d_miopen_db_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        for f in os.listdir(MIOPEN_DB):
            shutil.copy(os.path.join(MIOPEN_DB, f), tmp)
        os.environ["MIOPEN_USER_DB_PATH"] = tmp


DUMP_MAX_ELEMS = 4 << 20          # per array: 16 MiB of float32, the whole dump stays far under 64 MB


def dump_outputs(path, arrays):
    """Writes what a caller of the timed step holds after its last call as path/<name>.npy (float32).  An array longer than
    DUMP_MAX_ELEMS is stored as a fixed sample: the elements at seeded, sorted positions (the same positions in every run)."""
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().to(torch.float32).cpu().numpy().reshape(-1)
        if a.size > DUMP_MAX_ELEMS:
            a = a[np.sort(np.random.RandomState(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def cpu_baseline(a3d, B_cpu, steps):
    """The CPU restatement (oracle/, kind="port") of the same step on the host cores: torch-CPU backbone + FPN modules,
    oracle hot path, torch AdamW.  Bounded sample: B_cpu keyframes per step."""
    from oracle import act3d as OA
    from oracle import sampling as OS
    # torch's CPU kernels stop scaling (and oversubscribe badly) beyond a few dozen threads at these op sizes:
    # 256 threads measured 219 s/step on the GPU box's host, so the baseline uses at most 32 and says so.
    ncores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(ncores)
    m = build_model(a3d, torch.device("cpu"), torch.float32)
    params = [p for p in m.parameters() if p.requires_grad]
    groups = OA.optimizer_groups([(n, p) for n, p in m.named_parameters() if p.requires_grad])
    named = dict(m.named_parameters())
    opt = torch.optim.AdamW([{"params": [named[n] for n in groups[0]], "weight_decay": 0.0},
                             {"params": [named[n] for n in groups[1]], "weight_decay": 5e-4}], lr=1e-4)
    batch = synthetic_batch(B_cpu, 4, torch.device("cpu"), 123)
    cfg = OA.default_cfg(E=60, levels=3, ncam=4, bounds=PERACT_BOUNDS)
    np.random.seed(0)

    def step():
        opt.zero_grad()
        feats = [f.with_bias() for f in m.compute_visual_tokens(batch["rgbs"])]
        pcds = [torch.from_numpy(OS.pcd_downsample(batch["pcds"].numpy(), 8 if i == 0 else 2)) for i in range(3)]
        P = m.state_dict(keep_vars=True)
        out = OA.act3d_forward(P, cfg, feats, pcds, batch["curr_gripper"], None, gt_action=batch["action"], num_ghost_points=333)
        loss = sum(OA.keypose_loss(out, batch["action"]).values())
        loss.backward()
        opt.step()

    # median of >= 5 timed steps after 2 warm-ups (the first warm-up also bounds the leg: a host on
    # which one step takes longer than 15 s reports that single step)
    t0 = time.perf_counter()
    step()
    first = time.perf_counter() - t0
    if first > 15.0:
        dt, steps, how = first, 1, "one step (host too slow for repeats)"
    else:
        step()
        times = []
        for _ in range(steps):
            t0 = time.perf_counter()
            step()
            times.append(time.perf_counter() - t0)
        dt = sorted(times)[len(times) // 2]
        how = f"median of {steps} timed steps after 2 warm-ups"
    return {"value": B_cpu / dt, "unit": "samples/s", "cores": ncores, "kind": "port",
            "sample": f"{how}, {B_cpu} keyframes per step (same 4-cam 256x256 / 3-level / Ng=333 shapes, fp32 torch-CPU "
                      f"backbone+FPN + oracle hot path + AdamW), {dt:.2f} s/step"}


def time_kernel(fn, iters=20):
    """Average duration (ms) of `fn` (which enqueues on the current stream) with events on that stream."""
    for _ in range(3):
        fn()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters


def kernel_rooflines(a3d, device, B):
    """Live timing of the dominant hand-written kernels at the workload's shapes (ghost attention: Lq=333, S=4097,
    E=60, H=4) against their rooflines.  Algorithmic FLOPs per launch: forward 4*Lq*S*E*B (QK^T + PV), backward
    10*Lq*S*E*B (five contractions); the fused k,v in-projection + RoPE + operand-format kernel is HBM-bound:
    algorithmic bytes = the fp32 input rows + the 16-bit operand tensors it writes.  See DESIGN.md, kernels."""
    O = a3d.ops
    H, E, Lq, S = 4, 60, 333, 4097
    f16 = O.ATTN_MODE == "f16"
    g = torch.Generator().manual_seed(1)
    q_pre = torch.randn(B * Lq, E, generator=g).to(device)
    kv_pre = torch.randn(B * S, 2 * E, generator=g).to(device)
    q_xyz = torch.rand(B, Lq, 3, generator=g).to(device)
    k_xyz = torch.rand(B, S, 3, generator=g).to(device)
    operands = O.attn_operands16 if f16 else O.attn_operands
    Qs, Ks, Vt, Lqp, Sp, scale, freq, extra = operands(q_pre.data_ptr(), E, kv_pre.data_ptr(), 2 * E, kv_pre.data_ptr() + E * 4, 2 * E,
                                                       q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd=True)
    ns = O.pick_nsplit(B, H, Lqp, Sp)
    Oo, LSE = O.attn_core_fwd(Qs, Ks, Vt, None, B, H, Lq, Lqp, S, Sp, ns)
    dO = torch.randn_like(Oo)
    t_fwd = time_kernel(lambda: O.attn_core_fwd(Qs, Ks, Vt, None, B, H, Lq, Lqp, S, Sp, ns))
    t_bwd = time_kernel(lambda: O.attn_core_bwd(Qs, Ks, Vt, None, Oo, dO, LSE, B, H, Lq, Lqp, S, Sp, ns, extra=extra))
    f_fwd = 4.0 * Lq * S * E * B
    f_bwd = 10.0 * Lq * S * E * B
    x = torch.randn(B, S, E, generator=g).to(device)
    w = torch.randn(3 * E, E, generator=g).to(device)
    bb = torch.zeros(3 * E, device=device)
    Spad = (S + 63) // 64 * 64
    if f16:
        hf = torch.float16
        Kr = torch.empty((B, H, Spad, 32), device=device, dtype=hf)
        Vr = torch.empty((B, H, Spad, 32), device=device, dtype=hf)
        rows_only = O._rows_only()
        Kp = None if rows_only else torch.empty((B, H, 2, 16, Spad), device=device, dtype=hf)
        Vp = None if rows_only else torch.empty((B, H, 2, 16, Spad), device=device, dtype=hf)
        nz = lambda t_: None if t_ is None else t_.data_ptr()
        # the call ops.attn_operands_fused16 makes: rows-only operand set since round 6 (K rows + V rows with the ones channel);
        # A3D_ATTN_ROWS_ONLY=0: rows + planes of both, the round-5 set
        t_proj = time_kernel(lambda: O.L.call(
            "a3d_proj_rope_split16", x.data_ptr(), E, w.data_ptr() + E * E * 4, E, bb.data_ptr() + E * 4, E,
            k_xyz.data_ptr(), 1.0, Kr.data_ptr(), nz(Kp), 2, None, 1.0, Vr.data_ptr(), nz(Vp), O.V_ROWS if rows_only else O.V_PLANES,
            freq.data_ptr(), B, S, Spad, E, H, O.L.stream()))
        bytes_proj = B * (S * E * 4.0 + H * Spad * 2.0 * (32 + 32) * (1 if rows_only else 2))      # x rows + K, V rows (+ planes)
        # v_mfma_f32_16x16x32_{f16,bf16} = 16384 FLOP each; per (64 keys x 16 queries) the forward issues 8 score + 6 PV,
        # dQ 8 score + 8 dP + 6 dQ, dK/dV 8 score + 8 dP + 6 dV + 6 dK (two-part operands, d 15 -> 16)
        per_fwd, per_bwd, dt = 14, 22 + 28, "fp16 / bf16 MFMA on two-part operands (x = hi + lo; fp32 accumulate)"
    else:
        bf = torch.bfloat16
        Kr = torch.empty((B, H, Spad, O.QKW), device=device, dtype=bf)
        Kp = torch.empty((B, H, 2, 16, Spad), device=device, dtype=bf)
        Vr = torch.empty((B, H, Spad, 32), device=device, dtype=bf)
        Vp = torch.empty((B, H, 2, 16, Spad), device=device, dtype=bf)
        t_proj = time_kernel(lambda: O.L.call(
            "a3d_proj_rope_split", x.data_ptr(), E, w.data_ptr() + E * E * 4, E, bb.data_ptr() + E * 4, E,
            k_xyz.data_ptr(), 1.0, Kr.data_ptr(), O.QKW, Kp.data_ptr(), None, 1.0, Vr.data_ptr(), 32, Vp.data_ptr(),
            freq.data_ptr(), B, S, Spad, E, H, O.L.stream()))
        bytes_proj = B * (S * E * 4.0 + H * Spad * 2.0 * (O.QKW + 32 + 32 + 32))
        per_fwd, per_bwd, dt = 18, 26 + 32, "bf16 MFMA on split operands (q,k = hi+lo+lo2, p,v = hi+lo)"
    alt = {}
    if f16:
        # the split-bf16 family (attention.hip / attention_bwd.hip) at the same shape: it stays in the library as the backward of query
        # sets longer than the split-fp16 prep kernel's row sort serves (ops.ATTN16_BWD_MAX_LQP) and as A3D_ATTN_MODE=bf16x3; this entry
        # is the measurement that keeps it off the default path
        try:
            Qb, Kb, Vb, Lqp_b, Sp_b, _, _, extra_b = O.attn_operands(q_pre.data_ptr(), E, kv_pre.data_ptr(), 2 * E, kv_pre.data_ptr() + E * 4, 2 * E,
                                                                   q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd=True)
            nsb = O.pick_nsplit(B, H, Lqp_b, Sp_b)
            Ob, LSEb = O.attn_core_fwd(Qb, Kb, Vb, None, B, H, Lq, Lqp_b, S, Sp_b, nsb)
            tb_f = time_kernel(lambda: O.attn_core_fwd(Qb, Kb, Vb, None, B, H, Lq, Lqp_b, S, Sp_b, nsb))
            tb_b = time_kernel(lambda: O.attn_core_bwd(Qb, Kb, Vb, None, Ob, dO, LSEb, B, H, Lq, Lqp_b, S, Sp_b, nsb, extra=extra_b))
            alt = {"attn_bf16x3_family": {"fwd_ms": tb_f, "bwd_ms": tb_b, "fwd_vs_default": tb_f / t_fwd, "bwd_vs_default": tb_b / t_bwd,
                                          "note": "attention.hip / attention_bwd.hip (three-part bf16 q, k): the fallback backward for Lq > "
                                                  "ops.ATTN16_BWD_MAX_LQP and the A3D_ATTN_MODE=bf16x3 A/B family; not on the default path"}}
            del Qb, Kb, Vb, Ob, LSEb, extra_b
        except Exception as e:
            alt = {"attn_bf16x3_family": {"error": repr(e)[:200]}}
    tiles = B * H * (Lqp // 16) * (Sp // 64)
    x_fwd = tiles * per_fwd * 16384.0
    x_bwd = tiles * per_bwd * 16384.0
    extra_k = {}
    try:
        extra_k = other_kernel_rooflines(a3d, device, B, x, k_xyz, w, bb, freq)
    except Exception as e:                                   # a missing entry must not take the bench line down
        extra_k = {"error": repr(e)[:200]}
    return {**extra_k, **alt, **{
        "attn_fwd": {"bound": "mfma", "achieved": f_fwd / (t_fwd * 1e-3) / 1e12, "peak": 2500.0, "unit": "TFLOP/s",
                     "ms": t_fwd, "nsplit": ns, "launches_per_step": 6, "dtype": dt, "family": O.ATTN_MODE,
                     "executed_tflops": x_fwd / (t_fwd * 1e-3) / 1e12, "mfma_util_executed": x_fwd / (t_fwd * 1e-3) / 2.5e15},
        "attn_bwd": {"bound": "mfma", "achieved": f_bwd / (t_bwd * 1e-3) / 1e12, "peak": 2500.0,
                     "unit": "TFLOP/s", "ms": t_bwd, "launches_per_step": 6, "dtype": dt, "family": O.ATTN_MODE,
                     "executed_tflops": x_bwd / (t_bwd * 1e-3) / 1e12, "mfma_util_executed": x_bwd / (t_bwd * 1e-3) / 2.5e15},
        # achieved / frac: SURVEY 8(d)'s ALGORITHMIC bytes -- the fp32 context rows in + ONE 16-bit K and ONE 16-bit V out
        # (B S (4 E + 2 * 2 E)); stored_*: what the kernel really writes (two two-part operand tensors since round 6, four before), the figure rounds 1 - 4
        # reported as "achieved" (flattering: the review's recomputation gave 0.11 where the bench line said 0.30)
        "kv_proj_rope": {"bound": "hbm", "achieved": B * S * E * 8.0 / (t_proj * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s",
                         "algorithmic_bytes": B * S * E * 8.0, "stored_bytes": bytes_proj,
                         "stored_achieved": bytes_proj / (t_proj * 1e-3) / 1e9, "stored_frac": bytes_proj / (t_proj * 1e-3) / 1e9 / 8000.0,
                         "ms": t_proj, "launches_per_step": 6},
    }}


def other_kernel_rooflines(a3d, device, B, x, k_xyz, w, bb, freq):
    """HBM rooflines of the other hand-written hot-path kernels the round-3 review named, timed live at the workload's shapes
    (algorithmic bytes per launch):
      sq_fwd / sq_bwd   single-query attention over the S = 4097 context rows: forward reads X (4 S E B) + xyz (12 S B);
                        the backward reads them again and writes dX (4 S E B)
      knn_topk          12 N B bytes of points (N = 65 536), k = 4096 sorted indices out (8 k B)
      bn_stats          one read of a bf16 activation (the layer-1 map: 256 images x 64 x 64 x 256 channels)"""
    O, Lb = a3d.ops, a3d.ops.L
    lib = Lb.load()
    E, H = 60, 4
    S = x.shape[1]
    f4 = 4
    out = {}
    qrot = torch.randn(B, H, 1, 16, device=device)
    nsplit = O.sq_nsplit(B, S)
    ws = torch.empty((lib.a3d_sq_fwd_ws_floats(B, H, E, nsplit),), device=device)
    xbar, lse = torch.empty((B, H, E), device=device), torch.empty((B, H), device=device)
    wp, bp = w.data_ptr(), bb.data_ptr()

    def sq_fwd():
        Lb.call("a3d_sq_attn_fwd", x.data_ptr(), k_xyz.data_ptr(), wp + E * E * f4, E, bp + E * f4, None, E, None, qrot.data_ptr(),
                freq.data_ptr(), ws.data_ptr(), xbar.data_ptr(), lse.data_ptr(), None, B, S, E, H, nsplit, Lb.stream())
    t = time_kernel(sq_fwd)
    by = B * S * (E * 4.0 + 12.0)
    out["sq_fwd"] = {"bound": "hbm", "achieved": by / (t * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s", "ms": t,
                     "frac": by / (t * 1e-3) / 8e12, "launches_per_step": 6, "note": "keys + combine (2 launches)"}
    wsb = torch.zeros((lib.a3d_sq_bwd_ws_floats(B, H, E, nsplit),), device=device)
    dX = torch.empty((B, S, E), device=device)
    dqp = torch.empty((nsplit, B, H, 1, 16), device=device)
    gW, gb = torch.zeros(3 * E, E, device=device), torch.zeros(3 * E, device=device)

    def sq_bwd():
        Lb.call("a3d_sq_attn_bwd", x.data_ptr(), k_xyz.data_ptr(), wp + E * E * f4, E, bp + E * f4, None, E, qrot.data_ptr(),
                freq.data_ptr(), xbar.data_ptr(), lse.data_ptr(), None, wsb.data_ptr(), dX.data_ptr(), dqp.data_ptr(),
                gW.data_ptr() + E * E * f4, E, gb.data_ptr() + E * f4, None, E, None, B, S, E, H, nsplit, Lb.stream())
    t = time_kernel(sq_bwd)
    by = B * S * (2 * E * 4.0 + 12.0)
    out["sq_bwd"] = {"bound": "hbm", "achieved": by / (t * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s", "ms": t,
                     "frac": by / (t * 1e-3) / 8e12, "launches_per_step": 6, "note": "keys + weight-gradient reduce (2 launches)"}
    N, k = 65536, 4096
    g = torch.Generator().manual_seed(2)
    pts = torch.rand(B, N, 3, generator=g).to(device)
    pos = torch.rand(B, 3, generator=g).to(device)
    t = time_kernel(lambda: O.knn_topk(pos, pts, k))
    by = B * (N * 12.0 + k * 8.0)
    out["knn_topk"] = {"bound": "hbm", "achieved": by / (t * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s", "ms": t,
                       "frac": by / (t * 1e-3) / 8e12, "launches_per_step": 2, "note": "latency / sort bound: 2 launches (distances + histogram | select + sort)"}
    rows, C = 4 * B * 64 * 64, 256
    act = torch.randn(rows, C, device=device).to(torch.bfloat16)
    nslab = lib.a3d_bn_nslab(rows, C)
    partial = torch.empty((nslab, 2, C), device=device)
    t = time_kernel(lambda: Lb.call("a3d_bn_stats", act.data_ptr(), partial.data_ptr(), rows, C, nslab, Lb.stream()))
    by = rows * C * 2.0
    out["bn_stats"] = {"bound": "hbm", "achieved": by / (t * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s", "ms": t,
                       "frac": by / (t * 1e-3) / 8e12, "launches_per_step": 55, "note": "layer-1 map (537 MB); 55 launches of 17 - 537 MB per step"}
    del act
    # the backbone's own convolutions (bf16 MFMA implicit GEMMs with BatchNorm folded in): algorithmic bytes = one read of the
    # input map + one write of the output map; flops = 2 x pixels x taps x Cin x Cout, against the dense bf16 MFMA peak
    nimg = 4 * B
    for name, (cin, cout, hw, k, per_step) in {"conv3x3_64_64": (64, 64, 64, 3, 3), "conv3x3_32_64": (32, 64, 128, 3, 1),
                                               "conv1x1_64_256": (64, 256, 64, 1, 4)}.items():
        xin = torch.randn(nimg, cin, hw, hw, device=device).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2, bias=False).to(device).to(torch.bfloat16)
        conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
        scale = torch.stack([1.0 + 0.1 * torch.randn(cin), 0.1 * torch.randn(cin)]).to(device).contiguous()
        fn = a3d.nn.conv3x3_bn if k == 3 else a3d.nn.conv1x1_bn
        with torch.no_grad():
            t = time_kernel(lambda: fn(xin, conv, in_scale=scale, in_relu=True, want_stats=True))
        px = nimg * hw * hw
        by, fl = px * (cin + cout) * 2.0, 2.0 * px * k * k * cin * cout
        out[name] = {"bound": "hbm", "achieved": by / (t * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s", "ms": t,
                     "frac": by / (t * 1e-3) / 8e12, "mfma_TFLOPs": fl / (t * 1e-3) / 1e12, "mfma_frac": fl / (t * 1e-3) / 2.5e15,
                     "launches_per_step": per_step,
                     "note": f"{cin} -> {cout} channels, {nimg} maps of {hw} x {hw}; BatchNorm-apply of the producer and statistics of the output folded in"}
        del xin
    # the FPN's fine-level lateral convolution with bias + top-down add in the epilogue (a3d_conv1x1_topdown_fwd): algorithmic
    # bytes = one read of the backbone map and of the coarser FPN map + one write of the level's inner map
    hw, cin, cout = 128, 64, 64
    xin = torch.randn(nimg, cin, hw, hw, device=device).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    top = torch.randn(nimg, cout, hw // 2, hw // 2, device=device).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wlat, blat = torch.randn(cout, cin, 1, 1, device=device) * cin ** -0.5, torch.randn(60, device=device)
    with torch.no_grad():
        t = time_kernel(lambda: a3d.nn._LateralTopDownFn.apply(xin, wlat, blat, top))
    by = (xin.numel() + top.numel() + nimg * cout * hw * hw) * 2.0
    out["fpn_lateral_topdown"] = {"bound": "hbm", "achieved": by / (t * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s", "ms": t,
                                  "frac": by / (t * 1e-3) / 8e12, "launches_per_step": 1,
                                  "note": f"{cin} -> {cout} channels + bias + 2x-upsampled coarser map, {nimg} maps of {hw} x {hw}, one rounding (incl. the bf16 cast of the weight)"}
    del xin, top
    return out


def pmc_record(B):
    """HBM traffic / MFMA utilisation of the same kernels from the committed rocprofv3 --pmc passes (profiles/run_pmc.sh;
    counters cannot be read from inside this process).  None when no record exists for this batch size."""
    here = os.path.dirname(os.path.abspath(__file__))
    for rnd in ("r06", "r05", "r04"):                       # the newest committed counter record for this batch size
        path = os.path.join(here, "profiles", f"{rnd}_pmc_B{B}.json")
        try:
            with open(path) as fh:
                rec = json.load(fh)["kernels"]
            pmc_record.source = f"profiles/{rnd}_pmc_B{B}.json"
            return rec
        except Exception:
            continue
    return None


def _cfg5_traffic():
    """HBM bytes per launch of the fp8 attention forward (amax + pack + attn8_fwd) from the committed counter record of
    `bench.py --only-cfg5` (profiles/r06_campaign.sh pmc5), averaged over the run's launches; None without a record."""
    try:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r06_pmc_cfg5.json")) as fh:
            k = json.load(fh)["kernels"]["attn8_fwd"]
        return {"traffic": k["hbm_bytes"], "pmc": k.get("pmc"),
                "traffic_source": "profiles/r06_pmc_cfg5.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE; amax + pack + attn8_fwd, mean over the launches of bench.py --only-cfg5)"}
    except Exception:
        return {"traffic": None}


def cfg5_fp8_bench(a3d, device, B=16, steps=10, warmup=3):
    """BASELINE configs[4] (74 HiveFormer tasks, fp8 MFMA attention, 4 ghost-point levels at 10 000 points): the Act3D keypose
    EVALUATION forward at those token counts (3 cameras, 4 levels x 2500 ghost points, B keyframes per GPU; backbone + FPN +
    hot path), hipGraph-replayed, with the OPT-IN fp8 attention forward (A3D_ATTN_MODE=fp8, csrc/attention8.hip; e4m3
    tolerance, tests/test_attn8_gpu.py) and with the default split-fp16 attention.  The fp8 mode serves gradient-free
    forwards only (ops.ATTN_MODE), so the training step at these shapes -- the third number -- runs the default kernels."""
    E, O = a3d.engine, a3d.ops
    crit = a3d.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    batch = synthetic_batch(B, 3, device, seed=55)
    res = {}
    old = O.ATTN_MODE
    try:
        model = build_model(a3d, device, torch.bfloat16, levels=4, ghost_points=10000)
        model.eval()

        def forward():
            with torch.no_grad():
                return model(batch["rgbs"], batch["pcds"], batch["instr"], batch["curr_gripper"], gt_action=None)

        for mode in ("f16", "fp8"):
            O.ATTN_MODE = mode
            for _ in range(2):
                out = forward()
            torch.cuda.synchronize()
            graph = None
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    forward()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = forward()
                graph = g
            except Exception as e:                       # capture can fail (library versions): time the eager forward
                res[mode + "_graph_error"] = repr(e)[:200]
                torch.cuda.synchronize()
            run = graph.replay if graph is not None else forward
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            assert torch.isfinite(out["position"]).all()
            res[mode] = {"samples_per_s": B / dt, "ms_per_forward": dt * 1e3, "hipgraph": graph is not None}
            del graph
        O.ATTN_MODE = "f16"
        model.train()

        def fwd_bwd(sample, on_hot_done=None):
            return E.fwd_bwd_keypose(model, crit, sample, True, on_hot_done)

        flat, opt = E.get_optimizer(model, lr=1e-4, active_names=E.discover_active_parameters(model, lambda: fwd_bwd(batch)))
        step = E.GraphedStep(fwd_bwd, opt, batch, warmup=2)
        for _ in range(warmup):
            loss = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        res["train_default_mode"] = {"samples_per_s": B / dt, "ms_per_step": dt * 1e3, "final_loss": float(loss.item())}
        del step, model, flat, opt
        torch.cuda.empty_cache()
        # the ghost attention of one level at these shapes, forward only, both families (events on the launch stream)
        Lq, S, H, Ed = 2500, 3 * 32 * 32 + 1, 4, 60
        g = torch.Generator().manual_seed(3)
        qc = torch.randn(B * Lq, Ed, generator=g).to(device)
        kc = torch.randn(B * S, Ed, generator=g).to(device)
        vc = torch.randn(B * S, Ed, generator=g).to(device)
        O.ATTN_MODE = "fp8"           # both timings on the fp8 mode's operand set (value planes; the default set is rows-only)
        Qs, Ks, Vt, Lqp, Sp = O.attn_operands16(qc.data_ptr(), Ed, kc.data_ptr(), Ed, vc.data_ptr(), Ed, None, None, B, Lq, S, Ed, H,
                                                device, need_bwd=False)[:5]
        ns = O.pick_nsplit(B, H, Lqp, Sp)
        t = {}
        for mode in ("f16", "fp8"):
            O.ATTN_MODE = mode
            t[mode] = time_kernel(lambda: O.attn_core_fwd(Qs, Ks, Vt, None, B, H, Lq, Lqp, S, Sp, ns))
        flops = 4.0 * Lq * S * Ed * B
    finally:
        O.ATTN_MODE = old
    return {"metric": "keyposes/sec (Act3D evaluation forward, configs[4] token counts, fp8 attention)",
            "value": res["fp8"]["samples_per_s"], "unit": "samples/s", "n_gpus": 1, "ms_per_step": res["fp8"]["ms_per_forward"],
            "steps": steps, "warmup": warmup, "higher_is_better": True, "data": "synthetic",
            "dtype": "fp8 e4m3 attention forward (opt-in, e4m3 tolerance); bf16 backbone / FPN; fp32 elsewhere",
            "fp8_mode": res["fp8"], "default_mode_split_fp16": res["f16"], "train_step_default_mode": res["train_default_mode"],
            **{k: v for k, v in res.items() if k.endswith("_graph_error")},
            "config": {"workload": f"BASELINE configs[4] token counts: B={B} keyframes per GPU, 3 cameras 256x256, 4 levels x 2500 ghost "
                                   "points (num_ghost_points_val=10000), E=60, H=4; backbone + FPN + hot path, no gradient",
                       "attention_mode": "A3D_ATTN_MODE=fp8"},
            "roofline": {"bound": "mfma", "kernel": "attn8_fwd (+ amax + pack), ghost attention of one level: Lq=2500, S=3073",
                         "achieved": flops / (t["fp8"] * 1e-3) / 1e12, "peak": 5000.0, "unit": "TFLOP/s",
                         "frac": flops / (t["fp8"] * 1e-3) / 5.0e15, "ms": t["fp8"], "split_fp16_ms": t["f16"],
                         "split_fp16_frac": flops / (t["f16"] * 1e-3) / 2.5e15, **_cfg5_traffic(),
                         "dtype": "e4m3 MFMA 16x16x32 (fp32 accumulate); priced at the dense fp8 peak (5 PFLOP/s), the split-fp16 "
                                  "comparison at the fp16 / bf16 peak (2.5 PFLOP/s)"}}


def joint_step_bench(a3d, device, B=16, steps=10, warmup=3, world=1, rank=0):
    """BASELINE configs[3] (joint Act3D + trajectory-diffusion training, DP batch 128 over 8 GPUs = 16 per GPU): one joint
    iteration = one Act3D keypose training step AND one trajectory-diffusion training step on B samples each per rank (two
    models, two optimizers, as the reference trains them: main_keypose.py / main_trajectory.py), both data-parallel over the
    same ranks, hipGraph replays (engine.GraphedJointStep: the keypose all-reduces are hidden behind the trajectory step).
    Timed like the main line: barrier + synchronize on both sides, max over ranks."""
    import torch.distributed as dist
    import bench_denoise as BD
    E = a3d.engine
    model = build_model(a3d, device, torch.bfloat16)
    crit = a3d.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    kb = synthetic_batch(B, 4, device, seed=77 + rank)

    def kp_fwd_bwd(sample, on_hot_done=None):
        return E.fwd_bwd_keypose(model, crit, sample, True, on_hot_done)

    kflat, kopt = E.get_optimizer(model, lr=1e-4, active_names=E.discover_active_parameters(model, lambda: kp_fwd_bwd(kb)))
    planner = BD.build_planner(a3d, device, train=True)
    tb = BD.synthetic_inputs(B, 50, 3, device, seed=1 + rank)
    tcrit = a3d.TrajectoryCriterion()

    def tr_fwd_bwd(sample, on_hot_done=None):
        return E.fwd_bwd_trajectory(planner, tcrit, sample, on_hot_done)

    tflat, topt = E.get_optimizer(planner, lr=1e-4, active_names=E.discover_active_parameters(planner, lambda: tr_fwd_bwd(tb)))
    kddp = tddp = None
    if world > 1:
        overlap = os.environ.get("A3D_DP_OVERLAP", "1") == "1"
        kddp = E.FlatDataParallel(kflat, overlap=overlap, model=model)
        tddp = E.FlatDataParallel(tflat, overlap=overlap, model=planner)
        kddp.broadcast_parameters()
        tddp.broadcast_parameters()
    step = E.GraphedJointStep(E.GraphedStep(kp_fwd_bwd, kopt, kb, ddp=kddp, warmup=2, prefetch=model.backbone_maps if PREFETCH_BACKBONE else None),
                              E.GraphedStep(tr_fwd_bwd, topt, tb, ddp=tddp, warmup=2,
                                            prefetch=planner.prediction_head.backbone_maps if PREFETCH_BACKBONE else None))
    for _ in range(warmup):
        lk, lt = step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        lk, lt = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = tt.item()
    dt /= steps
    assert torch.isfinite(lk).all() and torch.isfinite(lt).all()
    return {"metric": "train samples/sec (keypose+diffusion fwd+bwd, joint iteration)", "value": world * B / dt, "unit": "samples/s",
            "n_gpus": world, "ms_per_step": dt * 1e3, "steps": steps, "warmup": warmup, "higher_is_better": True, "scaling": "weak",
            "data": "synthetic",
            "config": {"workload": f"BASELINE configs[3]: Act3D keypose step (B={B} keyframes per GPU, 4 cameras, 3 levels) + "
                                   f"DiffusionPlanner step (B={B} trajectories per GPU, horizon 50, 3 cameras, dropout 0.1), both with "
                                   "backbone + FPN + AdamW; hipGraph replays, joint iteration = engine.GraphedJointStep",
                       "global_batch": world * B, "parallelism": f"dp{world}", "hipgraph": True, "backbone_prefetch": PREFETCH_BACKBONE,
                       "allreduce": None if world == 1 else "RCCL all-reduce of both models' flat gradient buffers per iteration; hot-path "
                                    "segments start during the FPN backward, the keypose reductions complete behind the trajectory step",
                       "final_losses": [float(lk.item()), float(lt.item())]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64,
                    help="keyframe rows per GPU; 64 = the reference's default step: batch_size 16 episodes "
                         "(main_keypose.py:49) x ~4 keyframes per episode (<= 5, datasets/dataset_engine.py chunking)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--backbone-dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--full", action="store_true",
                    help="after the headline step also run every other leg: the sequential (no prefetch) step, the hot path alone, "
                         "the kernel rooflines, the `secondary` workloads (diffusion training / sampling, joint step, fp8 attention; "
                         "the joint step under data parallelism for --gpus N) and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed to DIR/<name>.npy (float32): its loss and "
                         "the flat parameter buffer after its AdamW update")
    ap.add_argument("--skip-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--kernels-only", action="store_true",
                    help="only the dominant-kernel micro-benchmarks (used for the rocprofv3 --pmc passes)")
    ap.add_argument("--skip-secondary", action="store_true",
                    help="with --full: skip the ChainedDiffuser entries (diffusion training step, 100-step sampling) of `secondary`")
    ap.add_argument("--only-cfg5", action="store_true", help="run only the configs[4] / fp8-attention secondary entry and print it")
    ap.add_argument("--cpu-batch", type=int, default=2)
    ap.add_argument("--cpu-steps", type=int, default=5)
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch.distributed as dist
    if world > 1:
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl", init_method="env://")
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    prepare_convolution_search()
    if os.environ.get("A3D_CUDNN_BENCHMARK", "1") == "1":
        torch.backends.cudnn.benchmark = True        # MIOpen find mode for the frozen backbone / FPN convolutions
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    a3d.lib.load()                                    # fails loudly if the HIP library is missing
    E = a3d.engine

    B = args.batch
    if args.kernels_only:
        print(json.dumps({"kernels": kernel_rooflines(a3d, device, B), "per_gpu_batch_keyframes": B}))
        return
    if args.only_cfg5:
        print(json.dumps(cfg5_fp8_bench(a3d, device, 16)))
        return
    model = build_model(a3d, device, torch.bfloat16 if args.backbone_dtype == "bf16" else torch.float32)
    crit = a3d.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    batch = synthetic_batch(B, 4, device, seed=1000 + rank)

    def fwd_bwd(sample, on_hot_done=None):
        # backward split at the FPN tokens: the hot-path gradient segments start their all-reduce (on_hot_done) while the
        # FPN / convolution backward is still to run (engine.fwd_bwd_keypose)
        return E.fwd_bwd_keypose(model, crit, sample, True, on_hot_done)

    active = E.discover_active_parameters(model, lambda: fwd_bwd(batch))
    flat, opt = E.get_optimizer(model, lr=1e-4, active_names=active)
    ddp = None
    if world > 1:
        ddp = E.FlatDataParallel(flat, overlap=os.environ.get("A3D_DP_OVERLAP", "1") == "1", model=model)
        ddp.broadcast_parameters()

    graphed = None
    graph_err = None
    if not args.no_graph:
        try:
            graphed = E.GraphedStep(fwd_bwd, opt, batch, ddp=ddp, warmup=2, prefetch=model.backbone_maps if PREFETCH_BACKBONE else None)
        except Exception as e:                         # capture can fail (e.g. library versions); fall back to eager
            graph_err = repr(e)[:200]
            graphed = None
            torch.cuda.synchronize()
            flat.rebind_grads()

    def step():
        if graphed is not None:
            return graphed()
        opt.zero_grad()
        loss = fwd_bwd(batch, None if ddp is None else ddp.hot_path_done)
        scale = ddp.sync_gradients() if ddp is not None else 1.0
        opt.step(grad_scale=scale)
        return loss

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    loss_val = float(loss.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": loss, "parameters": flat.flat})

    was_graphed = graphed is not None
    joint_dp = None
    if args.full and world > 1 and not args.skip_secondary and os.environ.get("A3D_BENCH_JOINT_DP", "1") == "1":
        # BASELINE configs[3] under data parallelism: every rank takes part (collectives), rank 0 reports it in `secondary`
        # (--full only; A3D_BENCH_JOINT_DP=0 or --skip-secondary leave it out)
        del graphed
        torch.cuda.empty_cache()
        try:
            joint_dp = joint_step_bench(a3d, device, 16, steps=max(3, args.steps // 2), warmup=2, world=world, rank=rank)
        except Exception as e:
            joint_dp = {"error": repr(e)[:300]}
        joint_dp["name"] = "joint_keypose_diffusion_cfg4"
        graphed = None

    if rank == 0:
        ms = elapsed / args.steps * 1e3
        res = {
            "metric": "train samples/sec (Act3D keypose fwd+bwd+AdamW step)", "value": world * B * args.steps / elapsed,
            "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("fp16 / bf16 MFMA on two-part operands (x = hi + lo; fp32 accumulate) in attention; " if a3d.ops.ATTN_MODE == "f16"
                      else "bf16 MFMA on split operands (q,k = hi+lo+lo2, p,v = hi+lo; fp32 accumulate) in attention; ") +
                     "fp32-accurate linears (f32 MFMA; bf16x3 MFMA from 4096 rows); " + ("bf16 frozen backbone + FPN" if args.backbone_dtype == "bf16" else "fp32 backbone + FPN"),
            "data": "synthetic",
            "config": {"workload": "Act3D keypose training step, 18-PerAct-task shapes: 4 cameras 256x256, 3 ghost-point "
                                   "levels, 1000 ghost points (333/level), E=60, frozen synthetic CLIP-RN50-shaped backbone "
                                   "+ trainable FPN included in the step",
                       "per_gpu_batch_keyframes": B, "global_batch": world * B, "parallelism": f"dp{world}",
                       "batch_note": "keyframe rows; reference default = 16 episodes x <=5 keyframes per step",
                       "hipgraph": was_graphed, "final_loss": loss_val, "backbone_prefetch": bool(was_graphed and PREFETCH_BACKBONE),
                       "allreduce": None if ddp is None else ("hot-path segments overlapped with the FPN backward" if ddp.overlap
                                                              else "one all-reduce after backward")},
        }
        if graph_err:
            res["config"]["graph_capture_error"] = graph_err
    if rank == 0 and args.full:
        if was_graphed and PREFETCH_BACKBONE and world == 1 and not args.skip_secondary:
            # the same step without the cross-step overlap: backbone -> FPN -> hot path -> backward -> AdamW strictly in order
            try:
                seq = E.GraphedStep(fwd_bwd, opt, batch, warmup=1)
                for _ in range(args.warmup):
                    seq()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    seq()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t1
                res["sequential_step"] = {"samples_per_s": B * args.steps / dt, "ms_per_step": dt / args.steps * 1e3,
                                          "note": "one graph per step, the frozen backbone inside its own step (no prefetch of the next batch's maps)"}
                del seq
            except Exception as e:
                res["sequential_step"] = {"error": repr(e)[:200]}
        # hot-path-only throughput (pre-computed visual tokens): informational
        try:
            with torch.no_grad():
                toks = model.compute_visual_tokens(batch["rgbs"])
                feats = [f.detach() for f in toks]                 # ops.TokenMap pairs: the owed FPN output bias travels along

            def hot_only():
                opt.zero_grad()
                out = model(None, batch["pcds"], batch["instr"], batch["curr_gripper"], gt_action=batch["action"],
                            visual_features=feats)
                sum(crit.compute_loss(out, batch).values()).backward()
            for _ in range(3):
                hot_only()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(10):
                hot_only()
            torch.cuda.synchronize()
            res["hot_path_only"] = {"samples_per_s": B * 10 / (time.perf_counter() - t1), "mode": "eager, fwd+bwd of everything "
                                    "after the FPN (pre-computed visual tokens), no optimizer"}
        except Exception as e:
            res["hot_path_only"] = {"error": repr(e)[:200]}
        try:
            ks = kernel_rooflines(a3d, device, B)
            if "error" in ks:
                res["kernels_error"] = ks.pop("error")
            alt_family = ks.pop("attn_bf16x3_family", None)       # the A/B family's timings: reported, never the dominant-kernel roofline
            # dominant hand-written kernel by (duration x launches per step) among the kernels whose launches all have the
            # timed shape (bn_stats' 55 launches per step range from 17 to 537 MB: its entry is the largest one)
            dom = max((k for k in ks if k != "bn_stats"), key=lambda k: ks[k]["ms"] * ks[k]["launches_per_step"])
            r = dict(ks[dom])
            r["kernel"] = dom
            r["frac"] = r["achieved"] / r["peak"]
            pmc = pmc_record(B) or {}
            r["traffic"] = pmc.get(dom, {}).get("hbm_bytes")
            if dom in pmc:
                r["traffic_source"] = f"{getattr(pmc_record, 'source', '?')} (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE per launch)"
                r["pmc"] = pmc[dom].get("pmc")
            res["roofline"] = r
            res["kernels"] = {k: {"ms": v["ms"], "achieved": v["achieved"], "unit": v["unit"], "frac": v["achieved"] / v["peak"],
                                  "launches_per_step": v.get("launches_per_step"),
                                  **({"mfma_util_executed": v["mfma_util_executed"]} if "mfma_util_executed" in v else {}),
                                  **{f: v[f] for f in ("mfma_TFLOPs", "mfma_frac", "note", "algorithmic_bytes", "stored_bytes", "stored_achieved",
                                                       "stored_frac") if f in v},
                                  **({"traffic": pmc[k]["hbm_bytes"]} if k in pmc else {}),
                                  **({"pmc": pmc[k]["pmc"]} if k in pmc and pmc[k].get("pmc") else {})}
                              for k, v in ks.items()}
            if alt_family is not None:
                res["kernels"]["attn_bf16x3_family"] = alt_family
        except Exception as e:
            res["roofline"] = {"error": repr(e)[:300]}
        if world == 1 and not args.skip_secondary:
            # the diffusion half of the metric and BASELINE configs[2], timed by this same driver-run process (N = 1 only:
            # the scaling runs stay short).  Each entry carries its own roofline.
            del graphed, model, flat, opt
            torch.cuda.empty_cache()
            import bench_denoise as BD
            res["secondary"] = []
            for name, fn in (("diffusion_train_script_shape", lambda: BD.training_bench(a3d, device, 22, 50, 3, steps=10, warmup=3)),
                             ("diffusion_train_cfg3_shape", lambda: BD.training_bench(a3d, device, 64, 16, 3, steps=10, warmup=3)),
                             ("diffusion_sampling_cfg3", lambda: BD.sampling_bench(a3d, device, 64, 16, 3, reps=3)),
                             # the horizon the reference deploys (interpolation_length 50); 24 trajectories = 192 sample-role workgroups
                             ("diffusion_sampling_script_shape", lambda: BD.sampling_bench(a3d, device, 24, 50, 3, reps=3)),
                             ("joint_keypose_diffusion_cfg4", lambda: joint_step_bench(a3d, device, 16)),
                             ("keypose_cfg5_fp8_attention", lambda: cfg5_fp8_bench(a3d, device, 16))):
                try:
                    r = fn()
                except Exception as e:
                    r = {"error": repr(e)[:300]}
                r["name"] = name
                res["secondary"].append(r)
                torch.cuda.empty_cache()
        if joint_dp is not None:
            res["secondary"] = [joint_dp]
        if world == 1 and not args.skip_cpu_baseline:
            try:
                res["cpu_baseline"] = cpu_baseline(a3d, args.cpu_batch, args.cpu_steps)
            except Exception as e:
                res["cpu_baseline"] = {"error": repr(e)[:300]}
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
