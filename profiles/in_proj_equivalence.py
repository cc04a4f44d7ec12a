"""Equivalence record of the packed in-projection refactor (ops.InProj, ops.ctx_kv_cache16, ops.sq_keys_fwd / sq_keys_bwd): for every
site that now takes its pointers from the one addressing, the entry names recorded at lib.call and the SHA-256 digests of every output
and gradient, on this tree and on the tree before it.  In the manner of profiles/attn_block_plan_equivalence.py, whose helpers it uses:

    python profiles/in_proj_equivalence.py --out this.json                                 # this tree
    python profiles/in_proj_equivalence.py --root PARENT_CHECKOUT --out parent.json
    python profiles/in_proj_equivalence.py --compare parent.json this.json --again parent2.json [--bench bench.json] \
        --out profiles/in_proj_equivalence.json

--root names the checkout whose package is imported (cases and runner are always this tree's).  Every case runs in a fresh child
process with fixed seeds, one at a time, each under its own time limit; the first case that exits with a fault, an abort or at its
limit ends the run and nothing more is started.  --compare passes when every launch list equals the parent's in order and every
digest equals the parent's; a tensor whose digest differs passes only if its largest difference from the parent is no larger than
the parent's own difference between its two runs (--again).

Shapes: B = 2, S = 70 (one full and one partial 64-key tile), E / H = 60 / 4 unless the case says otherwise.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from attn_block_plan_equivalence import digest, save, spread  # noqa: E402

CASE_SECONDS = 180                 # one case: a fresh process, the library load, at most one small planner and a few launches
B, S, E, H = 2, 70, 60, 4


def _rnd(dev, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g).to(dev), lambda *s: (torch.rand(*s, generator=g) * 2 - 0.5).to(dev)


def _grads(named):
    return {"g_" + n: p.grad for n, p in named if p.grad is not None}


def single_query_block(a3d, dev, AC, xyz):
    O = a3d.ops
    mha, norm = AC.modules(dev, E, H)
    rnd, pos = _rnd(dev, 21)
    q, kv, resid = (rnd(B, n, E).requires_grad_() for n in (1, S, 1))
    q_xyz, k_xyz = (pos(B, 1, 3), pos(B, S, 3)) if xyz else (None, None)
    dy = rnd(B, 1, E)
    fwd, y = AC.recorded(a3d, lambda: O.attn_block(q, kv, kv, resid, q_xyz, k_xyz, None, mha, norm, H))
    bwd, _ = AC.recorded(a3d, lambda: y.backward(dy))
    assert "a3d_sq_attn_fwd" in fwd and "a3d_sq_attn_bwd" in bwd, (fwd, bwd)
    named = list(mha.named_parameters(prefix="mha")) + list(norm.named_parameters(prefix="norm"))
    return fwd + bwd, dict(y=y.detach(), d_q=q.grad, d_kv=kv.grad, d_resid=resid.grad, **_grads(named))


def _query_layer(a3d, dev, AC, seed):
    """-> (apply(x, ctx, q_xyz, k_xyz, sink), named parameters) of one query-stream layer with non-trivial parameters"""
    import torch
    mha, n1 = AC.modules(dev, E, H, seed=seed)
    torch.manual_seed(seed + 100)
    l1, l2, n2 = torch.nn.Linear(E, E).to(dev), torch.nn.Linear(E, E).to(dev), torch.nn.LayerNorm(E).to(dev)
    torch.nn.init.normal_(n2.weight, mean=1.0, std=0.5), torch.nn.init.normal_(n2.bias, std=0.5)
    named = [(k + "." + n, p) for k, m in (("mha", mha), ("n1", n1), ("l1", l1), ("l2", l2), ("n2", n2)) for n, p in m.named_parameters()]
    apply = lambda x, ctx, q_xyz, k_xyz, sink=None: a3d.ops.QueryLayerFn.apply(
        x, ctx, q_xyz, k_xyz, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, n1.weight, n1.bias,
        l1.weight, l1.bias, l2.weight, l2.bias, n2.weight, n2.bias, H, sink)
    return apply, named


def query_layer(a3d, dev, AC):
    apply, named = _query_layer(a3d, dev, AC, 4)
    rnd, pos = _rnd(dev, 22)
    x, kv = rnd(B, 1, E).requires_grad_(), rnd(B, S, E).requires_grad_()
    q_xyz, k_xyz, dy = pos(B, 1, 3), pos(B, S, 3), rnd(B, 1, E)
    fwd, y = AC.recorded(a3d, lambda: apply(x, kv, q_xyz, k_xyz))
    bwd, _ = AC.recorded(a3d, lambda: y.backward(dy))
    assert "a3d_sq_attn_fwd" in fwd and "a3d_sq_attn_bwd_acc" in bwd, (fwd, bwd)
    return fwd + bwd, dict(y=y.detach(), d_x=x.grad, d_kv=kv.grad, **_grads(named))


def query_layer_behind_sink(a3d, dev, AC, defer):
    """the context of one pyramid level: two ghost-stream blocks (packed k | v projection, rows from ctx_kv_operands16) and one
    query-stream layer read it behind attach_grad_sink; CTX_DEFER parks the blocks' rows for the gate or adds them into the sink"""
    import torch
    O = a3d.ops
    O.CTX_DEFER = defer
    O.ReduceQueue.current = None
    Lq = 37
    blocks = [AC.modules(dev, E, H, seed=s) for s in (0, 1)]
    apply, named = _query_layer(a3d, dev, AC, 2)
    rnd, pos = _rnd(dev, 23)
    leaf, q, x = rnd(B, S, E).requires_grad_(), rnd(B, Lq, E).requires_grad_(), rnd(B, 1, E).requires_grad_()
    q_xyz, k_xyz, x_xyz = pos(B, Lq, 3), pos(B, S, 3), pos(B, 1, 3)
    dys = [rnd(B, Lq, E), rnd(B, Lq, E), rnd(B, 1, E)]

    def forward():
        ctx = O.attach_grad_sink(leaf * 1.0, [])
        sink = ctx._a3d_sink
        assert O.ctx_kv_applicable(ctx, k_xyz, [m for m, _ in blocks], H, Lq)
        with torch.no_grad():
            pairs = O.ctx_kv_operands16(ctx, k_xyz, [m for m, _ in blocks], H)
        ys = [O.attn_block(q, ctx, ctx, q, q_xyz, k_xyz, None, m, n, H, sink=sink, kv_pair=p) for (m, n), p in zip(blocks, pairs)]
        return ys + [apply(x, ctx, x_xyz, k_xyz, sink)]

    fwd, ys = AC.recorded(a3d, forward)
    bwd, _ = AC.recorded(a3d, lambda: torch.autograd.backward(ys, dys))
    assert "a3d_sq_attn_bwd_acc" in bwd and "a3d_ctx_kv_proj16" in fwd, (fwd, bwd)
    for i, (m, n) in enumerate(blocks):
        named += list(m.named_parameters(prefix="block%d.mha" % i)) + list(n.named_parameters(prefix="block%d.norm" % i))
    out = {"y%d" % i: y.detach() for i, y in enumerate(ys)}
    return fwd + bwd, dict(out, d_ctx=leaf.grad, d_q=q.grad, d_x=x.grad, **_grads(named))


def ctx_kv_operands(a3d, dev, AC, layers):
    O = a3d.ops
    mhas = [AC.modules(dev, E, H, seed=5 + j)[0] for j in range(layers)]
    rnd, pos = _rnd(dev, 24)
    ctx, xyz = rnd(B, S, E), pos(B, S, 3)
    assert O.ctx_kv_applicable(ctx, xyz, mhas, H)
    seen, pairs = AC.recorded(a3d, lambda: O.ctx_kv_operands16(ctx, xyz, mhas, H))
    return seen, {"%s%d" % (n, j): t for j, p in enumerate(pairs) for n, t in zip(("Kr", "Vr"), p)}


def _planner(a3d, dev, e, h):
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    import common as C
    torch.manual_seed(1000 + e)
    m = a3d.DiffusionPlanner(embedding_dim=e, num_attn_heads=h, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=100)
    with torch.no_grad():
        for n, p in m.named_parameters():                  # AdaLN modulations start at zero: give the tables something to hold
            if ".modulation." in n:
                p.normal_(std=0.1)
    return m.to(dev).eval(), C


def build_fused(a3d, dev, AC, e, h):
    """the sampler cache of a randomly initialised head: Ln = 5, four time rows, seven instruction tokens"""
    m, _ = _planner(a3d, dev, e, h)
    head = m.prediction_head
    rnd, pos = _rnd(dev, 25)
    ctx, xyz, instr, time_sin = rnd(B, S, e), pos(B, S, 3), rnd(B, 7, e), rnd(4, e)
    seen, st = AC.recorded(a3d, lambda: head.build_fused(ctx, xyz, instr, None, time_sin, 5))
    tensors = {"lang_kv": st["lang_kv"]}
    for i, rec in enumerate(st["layers"]):
        tensors.update({"Kf%d" % i: rec["Kf"], "Vt%d" % i: rec["Vt"]}, **{"mod%d_%d" % (i, k): t for k, t in enumerate(rec["mods"])})
    return seen, tensors


def trajectory(a3d, dev, AC, persist):
    """compute_trajectory, four steps, on the persistent sampler / on the per-phase launches"""
    import torch
    m, C = _planner(a3d, dev, E, H)
    a3d.diffusion.DN_PERSIST = persist
    inp = C.trajectory_inputs(95, B, 16, 2, E, pad_last=3)
    tokens = C.tokens_from_maps(inp["fmap"]).to(dev)
    d = {k: v.to(dev) for k, v in inp.items()}
    seen, out = AC.recorded(a3d, lambda: m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"],
                                                              init_noise=d["init_noise"], step_noise=d["step_noise"], visual_tokens=tokens,
                                                              n_steps=4))
    torch.cuda.synchronize()
    assert ("a3d_dn_persist" in seen) == persist and torch.isfinite(out).all(), seen
    return seen, {"trajectory": out}


CASES = {
    "single-query block, xyz": lambda *a: single_query_block(*a, True),
    "single-query block, no xyz": lambda *a: single_query_block(*a, False),
    "query layer": query_layer,
    "query layer behind a sink, deferred": lambda *a: query_layer_behind_sink(*a, True),
    "query layer behind a sink, undeferred": lambda *a: query_layer_behind_sink(*a, False),
    "ctx_kv_operands16, one layer": lambda *a: ctx_kv_operands(*a, 1),
    "ctx_kv_operands16, two layers": lambda *a: ctx_kv_operands(*a, 2),
    "build_fused E=60 H=4": lambda *a: build_fused(*a, 60, 4),
    "build_fused E=30 H=2": lambda *a: build_fused(*a, 30, 2),
    "trajectory, persistent": lambda *a: trajectory(*a, True),
    "trajectory, per phase": lambda *a: trajectory(*a, False),
}


def run_one(root, name, tensors_dir=None):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, root)
    import torch
    import attn_block_cases as AC
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(a3d.__file__))) == root, a3d.__file__
    launches, tensors = CASES[name](a3d, torch.device("cuda:0"), AC)
    torch.cuda.synchronize()
    save(tensors_dir, name, tensors)
    return dict(launches=launches, digests={k: digest(v) for k, v in tensors.items()})


def run_all(root, tensors_dir):
    results = {}
    for n in CASES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--case", n, "--tensors", tensors_dir],
                               stdout=subprocess.PIPE, text=True, timeout=CASE_SECONDS)
            status = p.returncode and "exit status %d" % p.returncode
        except subprocess.TimeoutExpired:                          # run() has ended the child
            status = "no result within %d s" % CASE_SECONDS
        if status:
            raise SystemExit("case %r: %s; nothing more is started" % (n, status))
        results[n] = json.loads(p.stdout.strip().splitlines()[-1])
        print(n, len(results[n]["launches"]), "launches", flush=True)
    return results


def compare(parent, this, again, dirs):
    """dirs: the tensor directories of parent, this, again"""
    report = {}
    for name, p in parent.items():
        t = this[name]
        differing = sorted(k for k in p["digests"] if p["digests"][k] != t["digests"].get(k))
        entry = dict(launches_identical=p["launches"] == t["launches"], parent=p, this=t,
                     digests_identical=not differing and set(p["digests"]) == set(t["digests"]))
        if again is not None:
            entry["parent_unstable"] = sorted(k for k in p["digests"] if again[name]["digests"][k] != p["digests"][k])
        if differing:
            entry["differing"] = {}
            for k in differing:
                own, ours = spread(dirs[0], dirs[2], name, k), spread(dirs[0], dirs[1], name, k)
                entry["differing"][k] = dict(max_abs_parent_vs_parent_again=own, max_abs_parent_vs_this=ours,
                                             within_parent_spread=own is not None and ours is not None and ours <= own)
        entry["passes"] = bool(entry["launches_identical"] and set(p["digests"]) == set(t["digests"]) and
                               all(d["within_parent_spread"] for d in entry.get("differing", {}).values()))
        report[name] = entry
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=REPO)
    ap.add_argument("--case")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--again", help="a second run of the parent: its own run-to-run spread")
    ap.add_argument("--bench", help="JSON file with the bench.py lines of the parent (twice) and of this tree")
    ap.add_argument("--tensors", help="(with --case) directory that receives the case's tensors")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.case:
        print(json.dumps(run_one(root, args.case, args.tensors)))
        return
    load = lambda f: json.load(open(f))
    if args.compare:
        files = args.compare + ([args.again] if args.again else [None])
        cases = compare(load(files[0]), load(files[1]), load(files[2]) if files[2] else None, [f and f + ".tensors" for f in files])
        result = dict(cases=cases, all_launch_lists_identical=all(e["launches_identical"] for e in cases.values()),
                      all_digests_identical=all(e["digests_identical"] for e in cases.values()),
                      passes=all(e["passes"] for e in cases.values()))
        if args.bench:
            result["bench"] = load(args.bench)
    else:
        result = run_all(root, args.out + ".tensors")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    if args.compare:
        print(json.dumps({k: v for k, v in result.items() if k not in ("cases", "bench")}))
        for n, e in result["cases"].items():
            if not e["passes"] or not e["digests_identical"]:
                print(n, "launches identical:", e["launches_identical"], e.get("differing"))
        sys.exit(0 if result["passes"] else 1)


if __name__ == "__main__":
    main()
