"""Equivalence record of the sampling refactor (one layer walk, one head iteration, one argument check, one graph cache,
compute_trajectory in phases): for every case below the launch list recorded at lib.call -- entry name, every non-pointer argument
(the c_int / c_uint / c_size_t / c_ulonglong / c_float positions of lib.SIGNATURES) and the integer fields of the Dn*Params blocks
passed by reference; pointers are not compared -- and the SHA-256 digests of every result tensor.  Run on each tree and compare:

    python profiles/sampling_refactor_equivalence.py --dry --root PARENT_CHECKOUT --out parent.dry.json
    python profiles/sampling_refactor_equivalence.py --dry --out this.dry.json
    python profiles/sampling_refactor_equivalence.py --same-launches parent.dry.json this.dry.json      # exit status 1 unless identical
    python profiles/sampling_refactor_equivalence.py --root PARENT_CHECKOUT --out parent.json           # live, only after the above
    python profiles/sampling_refactor_equivalence.py --out this.json
    python profiles/sampling_refactor_equivalence.py --compare parent.json this.json [--again parent2.json ...] \
        [--dry-pair parent.dry.json this.dry.json] [--bench bench.json] --out profiles/sampling_refactor_equivalence.json
    python profiles/sampling_refactor_equivalence.py --into RECORD.json --bench bench.json --out RECORD.json    # timings added later

--dry: lib.call is replaced by a recorder that does not call through (and torch.empty / empty_like hand out zeroed memory, so what a
skipped kernel would have written -- indices included -- is defined).  No path here reads a device value on the host, so the dry
lists are complete; the live pass is meant to run only when the two trees' dry lists are identical, so that no launch with other
arguments reaches the device.  --time measures the host-bound sampling paths of one tree (see time_one).

--root names the checkout whose package (and bench_denoise.py) is imported; the cases, the fixtures (tests/) and the runner are
always this tree's.  Every case runs in a fresh child process with fixed seeds and a time limit, at most --jobs (<= 4) at a time;
after a case that exits with an error or runs out of time its siblings are ended and nothing more is started.  Each live run leaves
its tensors next to its JSON (FILE.tensors/<case>.npz, not kept): for a tensor whose digests differ --compare records the largest
absolute difference between the parent's runs (--again) and between the trees.
"""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.append(REPO)                # the fixtures import the oracle package from the repository root
CASE_SECONDS = 240                  # one case: a fresh process, the library load, the model and a few dozen small calls
SCHEDULES = {"chain n_steps=2": dict(n_steps=2),
             "ddim K=4": dict(num_inference_steps=4, scheduler="ddim", eta=0.0),
             "ddpm K=4": dict(num_inference_steps=4, scheduler="ddpm")}
KEYWORD_ROWS = ("persistent", "op-by-op")
ACTIONER_CASES = ("actioner, shared backbone pass", "actioner, two backbone passes", "actioner, num_samples=2 select=goal")


def case_names():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import test_sampler_schedule_gpu as TS
    return (["sampling: " + c[0] for c in TS.CENSUS] + ["keywords: " + r for r in KEYWORD_ROWS] +
            ["multi-round head", "training: eval", "training: dropout"] + list(ACTIONER_CASES))


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def fname(name):
    return "".join(ch if ch.isalnum() else "_" for ch in name) + ".npz"


# ------------------------------------------------------------------------------------------------ the recorder
class Recorder:
    """Wraps lib.call of the imported package: every call is appended to self.seen as [entry, value, ...]."""

    def __init__(self, a3d, dry):
        self.lib, self.dry, self.seen, self.inner = a3d.lib, dry, [], a3d.lib.call
        scalar = (ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_ulonglong, ctypes.c_float)
        self.scalar = {n: [(i, t is ctypes.c_float) for i, t in enumerate(sig[1]) if t in scalar]
                       for n, sig in a3d.lib.SIGNATURES.items()}
        a3d.lib.call = self

    def __call__(self, entry, *args):
        rec = [entry]
        for i, is_float in self.scalar[entry]:
            rec.append(repr(float(args[i])) if is_float else int(args[i]))
        for a in args:
            block = getattr(a, "_obj", None)                          # ctypes.byref(structure)
            if isinstance(block, ctypes.Structure):
                rec.append({f: int(getattr(block, f)) for f, t in block._fields_ if t is ctypes.c_int})
        self.seen.append(rec)
        if not self.dry:
            return self.inner(entry, *args)

    def take(self):
        out, self.seen = self.seen, []
        return out


def zeroed_empty(torch):
    """torch.empty / empty_like hand out zeroed memory: the dry pass launches none of the kernels that would have written it"""
    empty, empty_like = torch.empty, torch.empty_like
    torch.empty = lambda *a, **k: empty(*a, **k).zero_()
    torch.empty_like = lambda *a, **k: empty_like(*a, **k).zero_()


class Case:
    def __init__(self, rec):
        self.rec, self.launches, self.tensors = rec, {}, {}

    def run(self, variant, fn):
        """fn() -> {name: tensor}; its launches and tensors are filed under `variant`"""
        import torch
        torch.manual_seed(0)
        self.rec.take()
        out = fn()
        torch.cuda.synchronize()
        self.launches[variant] = self.rec.take()
        for k, v in out.items():
            if v is not None:
                self.tensors["%s | %s" % (variant, k)] = v.detach().clone()


def ranking_tensors(pl):
    import torch
    out = {}
    if pl.last_ranking is not None:
        out.update({"last_ranking." + f: v for f, v in zip(pl.last_ranking._fields, pl.last_ranking) if torch.is_tensor(v)})
    if pl.last_guidance is not None:
        out["last_guidance.nearest"] = pl.last_guidance.nearest
    return out


def grads(m, loss):
    out = {"loss": loss}
    out.update({"grad " + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
    return out


# ------------------------------------------------------------------------------------------------ the cases
def sampling_model(a3d, dev, TS, C, **kw):
    from test_oracle_golden import _diffusion_params, load
    m = a3d.DiffusionPlanner(embedding_dim=TS.E, output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, weight_tying=True,
                             gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D", diffusion_timesteps=TS.T, **kw)
    m.load_state_dict(_diffusion_params(load("diffusion.pt")), strict=False)
    return m.to(dev).eval()


def sampling_inputs(torch, TS, C, dev, seed, B, Ln, G):
    inp = C.trajectory_inputs(seed, B, Ln, TS.NCAM, TS.E, pad_last=2)
    d = {k: v.to(dev) for k, v in inp.items()}
    d["tokens"] = C.tokens_from_maps(inp["fmap"]).to(dev)
    if G is not None:                                                 # per-candidate draws
        g = torch.Generator().manual_seed(seed + 1)
        d["init_noise"] = torch.randn(B, G, Ln, 9, generator=g).to(dev)
        d["step_noise"] = torch.randn(TS.T, B, G, Ln, 9, generator=g).to(dev)
    g = torch.Generator().manual_seed(seed + 2)
    d["scene_mask"] = (torch.rand(B, TS.NCAM, 256, 256, generator=g) < 0.1).to(dev)
    return d


def sample(m, d, sched, **kw):
    noise = None if sched.get("scheduler") == "ddim" else \
        d["step_noise"][:sched["num_inference_steps"]].contiguous() if "num_inference_steps" in sched else d["step_noise"]
    return m.compute_trajectory(d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], init_noise=d["init_noise"],
                                step_noise=noise, visual_tokens=d["tokens"], **sched, **kw)


def census_row(TS, name):
    import torch
    row = next(c for c in TS.CENSUS if c[0] == name)
    _, Ln, G, persist, fused, path = row
    B = 2
    if "too many" in name:                                            # 2 * B * ceil(L / 16) + 16 one above the CU count
        B = (torch.cuda.get_device_properties(0).multi_processor_count - 16) // 4 + 1
    return B, Ln, G, persist, fused, path


def run_sampling(case, a3d, dev, TS, C, name):
    import torch
    B, Ln, G, persist, fused, path = census_row(TS, name)
    a3d.diffusion.DN_PERSIST = persist
    m = sampling_model(a3d, dev, TS, C)
    d, d2 = (sampling_inputs(torch, TS, C, dev, seed, B, Ln, G) for seed in (99, 100))
    kw = dict(fused=fused, num_samples=G)
    for tag, sched in SCHEDULES.items():
        case.run(tag + ", eager", lambda: {"final": sample(m, d, sched, **kw)})
        assert m.last_sampler_path.split(" (")[0] == path.split(" (")[0], (m.last_sampler_path, path)

        def traced():
            final, trace = sample(m, d, sched, return_trace=True, **kw)
            return dict({"final": final}, **{"trace %d" % i: x for i, x in enumerate(trace)})
        case.run(tag + ", trace", traced)
        m._graph = None
        # capture, replay, replay with new inputs
        case.run(tag + ", graph x3", lambda: {"call %d" % i: sample(m, x, sched, use_graph=True, **kw).clone()
                                              for i, x in enumerate((d, d, d2))})
        m._graph = None


def run_keywords(case, a3d, dev, TS, C, name):
    B, Ln, _, persist, fused, _ = census_row(TS, name)
    a3d.diffusion.DN_PERSIST = persist
    m = sampling_model(a3d, dev, TS, C)
    import torch
    d = sampling_inputs(torch, TS, C, dev, 99, B, Ln, 2)
    sched = SCHEDULES["ddpm K=4"]
    variants = {"num_samples=2": {},
                "select=consensus": dict(select="consensus"),
                "select clearance rule": dict(select={"goal": 1.0, "clearance": 0.5}, scene_mask=d["scene_mask"]),
                "fused_conditioning": dict(fused_conditioning=True),
                "guide": dict(guide={"push": 1.0, "smooth": 0.5, "start": 0.5}, scene_mask=d["scene_mask"])}
    for tag, extra in variants.items():
        m.last_ranking = m.last_guidance = None
        case.run(tag, lambda: dict({"final": sample(m, d, sched, fused=fused, num_samples=2, **extra)}, **ranking_tensors(m)))


def run_multi_round(case, a3d, dev, TS, C):
    from test_oracle_golden import load, multi_head_inputs
    r = load("diffusion_multi.pt")
    inp, feats, xyz, P, bounds = multi_head_inputs(r)
    m = a3d.DiffusionPlanner(embedding_dim=r["cfg"]["E"], output_dim=7, num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6,
                             use_instruction=True, use_goal=True, use_goal_at_test=True, feat_scales_to_use=2, attn_rounds=2,
                             weight_tying=False, gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D",
                             diffusion_timesteps=100, dropout=0.0)
    m.load_state_dict(P, strict=False)
    m.to(dev).eval()
    d = {k: v.to(dev) for k, v in inp.items()}
    toks = [f.to(dev) for f in feats]
    args = (d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"])

    def two_steps():
        final, trace = m.compute_trajectory(*args, init_noise=d["init_noise"], step_noise=d["step_noise"], visual_tokens=toks, n_steps=2,
                                            return_trace=True)
        return {"final": final, "trace 0": trace[0], "trace 1": trace[1]}
    case.run("two sampling steps", two_steps)
    m.train()
    case.run("training forward + backward", lambda: grads(m, backward(m(
        d["trajectory"], d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], noise=d["noise"],
        timesteps=d["timesteps"], visual_tokens=toks))))


def backward(loss):
    loss.backward()
    return loss


def run_training(case, a3d, dev, TS, C, dropout):
    m = sampling_model(a3d, dev, TS, C, dropout=0.1, dropout_seed=7)
    m.train(dropout)
    import torch
    d = sampling_inputs(torch, TS, C, dev, 99, 2, 8, None)
    for i in range(2 if dropout else 1):                               # with dropout: two passes, the generator state advances
        m.zero_grad(set_to_none=True)
        case.run("forward + backward %d" % i, lambda: grads(m, backward(m(
            d["trajectory"], d["mask"], None, d["pcd"], d["instr"], d["curr_gripper"], d["goal_gripper"], noise=d["noise"],
            timesteps=d["timesteps"], visual_tokens=d["tokens"]))))


def run_actioner(case, a3d, dev, name):
    import torch
    import test_actioner_gpu as TA
    torch.backends.cudnn.deterministic = True
    kp = TA.make_keypose(a3d, dev)
    pl = TA.make_planner(a3d, dev, backbone_of=kp)
    instr = torch.randn(1, 53, 512, generator=torch.Generator().manual_seed(77)).to(dev)
    share = name == ACTIONER_CASES[0] or name == ACTIONER_CASES[2]
    act = a3d.Actioner(kp, pl, predict_keypose=True, predict_trajectory=True, share_backbone=share)
    act.set_instruction(instr)
    B, Ln, G = 2, 16, 2
    obs = [TA.observation(dev, seed, B, Ln) for seed in (1, 2)]
    kw = [dict(n_steps=2, init_noise=o["init_noise"], step_noise=o["step_noise"]) for o in obs]
    if name == ACTIONER_CASES[2]:
        for o, k in zip(obs, kw):
            k["init_noise"], k["step_noise"] = TA.candidate_noise(dev, B, G, Ln, 100, seed=9)
            k.update(num_samples=G, select="goal")

    def predict(i, use_graph):
        TA.set_rng(kp)
        o = obs[i]
        out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], use_graph=use_graph, **kw[i])
        assert act.last_backbone_passes == (1 if share else 2)
        return {"action": out["action"].clone(), "trajectory": out["trajectory"].clone()}

    for i in range(2):                                                # settle: the convolution library may change its algorithm
        predict(0, False)
    case.run("eager", lambda: dict(predict(0, False), **ranking_tensors(pl)))
    case.run("graph x3", lambda: {"call %d %s" % (j, k): v for j, i in enumerate((0, 0, 1)) for k, v in predict(i, True).items()})


def run_one(root, name, dry, tensors_dir):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    sys.path.insert(0, root)
    import torch
    import common as C
    import test_sampler_schedule_gpu as TS
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(a3d.__file__))) == root
    a3d.lib.load()
    dev = torch.device("cuda:0")
    case = Case(Recorder(a3d, dry))
    if dry:
        zeroed_empty(torch)
    kind, _, rest = name.partition(": ")
    if kind == "sampling":
        run_sampling(case, a3d, dev, TS, C, rest)
    elif kind == "keywords":
        run_keywords(case, a3d, dev, TS, C, rest)
    elif name == "multi-round head":
        run_multi_round(case, a3d, dev, TS, C)
    elif kind == "training":
        run_training(case, a3d, dev, TS, C, rest == "dropout")
    else:
        run_actioner(case, a3d, dev, name)
    if tensors_dir and not dry:
        import numpy as np
        os.makedirs(tensors_dir, exist_ok=True)
        np.savez(os.path.join(tensors_dir, fname(name)), **{k: v.cpu().numpy() for k, v in case.tensors.items()})
    return dict(launches=case.launches, digests={} if dry else {k: digest(v) for k, v in case.tensors.items()})


def run_all(root, jobs, dry, tensors_dir):
    results, pending, running = {}, case_names(), []
    while pending or running:
        while pending and len(running) < min(jobs, 4):
            n = pending.pop(0)
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--case", n, "--tensors", tensors_dir] + (["--dry"] if dry else [])
            running.append((n, subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)))
        n, p = running.pop(0)
        try:
            stdout, _ = p.communicate(timeout=CASE_SECONDS)
            status = p.returncode and "exit status %d" % p.returncode
        except subprocess.TimeoutExpired:
            status = "no result within %d s" % CASE_SECONDS
        if status:                                                     # nothing more is started, nothing is left running
            for _, q in [(n, p)] + running:
                q.kill()
                q.wait()
            raise SystemExit("case %r: %s; its siblings were ended and nothing more is started" % (n, status))
        results[n] = json.loads(stdout.strip().splitlines()[-1])
        print("done: %s (%d variants)" % (n, len(results[n]["launches"])), flush=True)
    return results


# ------------------------------------------------------------------------------------------------ comparing two runs
def launch_report(p, t):
    """per variant: the number of launches, the digest of the parent's list and whether this tree's list is the same"""
    out = {}
    for v in sorted(set(p) | set(t)):
        a, b = p.get(v), t.get(v)
        e = dict(launches=None if a is None else len(a), sha256=hashlib.sha256(json.dumps(a).encode()).hexdigest(),
                 same="identical" if a == b else "DIFFERENT")
        if a != b and a is not None and b is not None:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            e["first_difference"] = dict(index=i, parent=a[i] if i < len(a) else None, this=b[i] if i < len(b) else None)
        out[v] = e
    return out


def spread(dir_a, dir_b, name, key):
    """largest |a - b| of one tensor between two runs (None when a run kept no tensors)"""
    import numpy as np
    fa, fb = os.path.join(dir_a, fname(name)), os.path.join(dir_b, fname(name))
    if not (os.path.exists(fa) and os.path.exists(fb)):
        return None
    return float(np.abs(np.load(fa)[key].astype(np.float64) - np.load(fb)[key]).max())


def compare(parent, this, again, dirs, dry):
    report = {}
    for name, p in parent.items():
        t = this[name]
        entry = dict(launches=launch_report(p["launches"], t["launches"]), tensors=len(p["digests"]))
        if dry:
            entry["dry_launches_identical"] = dry[0][name]["launches"] == dry[1][name]["launches"]
            entry["dry_equals_live"] = dry[1][name]["launches"] == t["launches"]
        differing = sorted(k for k in set(p["digests"]) | set(t["digests"]) if p["digests"].get(k) != t["digests"].get(k))
        unstable = sorted(k for k in p["digests"] if any(a[name]["digests"][k] != p["digests"][k] for a in again))
        entry["digests_identical"] = not differing
        entry["parent_unstable"] = unstable
        entry["differs_on_a_parent_stable_tensor"] = sorted(set(differing) - set(unstable)) if again else sorted(differing)
        worst = lambda pairs, k: max((x for x in (spread(a, b, name, k) for a, b in pairs) if x is not None), default=None)
        entry["spreads"] = {k: dict(max_abs_parent_vs_parent_again=worst([(dirs[0], d) for d in dirs[2:]], k),
                                    max_abs_parent_vs_this=spread(dirs[0], dirs[1], name, k),
                                    digest_identical_to_parent=k not in differing) for k in sorted(set(unstable) | set(differing))}
        report[name] = entry
    return report


# ------------------------------------------------------------------------------------------------ host time of the sampling paths
def time_one(root):
    """One tree, one process: the two graphed sampling entries of bench.py --full's `secondary` (bench_denoise.sampling_bench at
    B = 64 / L = 16 and B = 24 / L = 50) and the eager op-by-op path (fused=False, n_steps=10: 189 launches per step, the path most
    sensitive to host overhead) on the equivalence model; every timed window ends with a device synchronise."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    sys.path.insert(0, root)
    import torch
    import common as C
    import test_sampler_schedule_gpu as TS
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    BD = importlib.import_module("bench_denoise")
    assert os.path.dirname(os.path.abspath(BD.__file__)) == root
    dev = torch.device("cuda:0")
    out = {}
    for key, (B, Ln) in (("graphed_B64_L16_ms_per_100_steps", (64, 16)), ("graphed_B24_L50_ms_per_100_steps", (24, 50))):
        out[key] = BD.sampling_bench(a3d, dev, B, Ln, 3, reps=3)["ms_per_100_step_batch"]
    m = sampling_model(a3d, dev, TS, C)
    d = sampling_inputs(torch, TS, C, dev, 99, 2, 8, None)
    run = lambda: sample(m, d, dict(n_steps=10), fused=False)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    out["eager_op_by_op_ms_per_10_steps"] = (time.perf_counter() - t0) / 5 * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=REPO)
    ap.add_argument("--case")
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out")
    ap.add_argument("--same-launches", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--again", nargs="*", default=[], help="further runs of the parent: its own run-to-run spread")
    ap.add_argument("--dry-pair", nargs=2, metavar=("PARENT_DRY", "THIS_DRY"))
    ap.add_argument("--bench", help="timings (the lines of --time, collected by the caller) for the record's \"bench\" entry")
    ap.add_argument("--into", help="an existing record: --bench is added to it and the result written to --out")
    ap.add_argument("--time", action="store_true", help="print the timings of --root as one JSON line")
    ap.add_argument("--tensors", help="(with --case) directory that receives the case's tensors")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    load = lambda f: json.load(open(f))
    if args.case:
        print(json.dumps(run_one(root, args.case, args.dry, args.tensors)))
        return
    if args.time:
        print(json.dumps(time_one(root)))
        return
    if args.same_launches:
        a, b = (load(f) for f in args.same_launches)
        bad = [(n, v) for n in a for v in sorted(set(a[n]["launches"]) | set(b[n]["launches"]))
               if a[n]["launches"].get(v) != b[n]["launches"].get(v)]
        for n, v in bad:
            print("DIFFERENT: %s | %s" % (n, v), launch_report(a[n]["launches"], b[n]["launches"])[v].get("first_difference"))
        print("%d cases, %d launch lists, %d launches: %s" % (
            len(a), sum(len(c["launches"]) for c in a.values()), sum(len(v) for c in a.values() for v in c["launches"].values()),
            "DIFFERENT" if bad or set(a) != set(b) else "identical"))
        raise SystemExit(1 if bad or set(a) != set(b) else 0)
    if args.into:
        result = dict(load(args.into), bench=load(args.bench))
    elif args.compare:
        dirs = [f + ".tensors" for f in args.compare + args.again]
        cases = compare(load(args.compare[0]), load(args.compare[1]), [load(f) for f in args.again], dirs,
                        [load(f) for f in args.dry_pair] if args.dry_pair else None)
        result = dict(cases=cases,
                      all_launch_lists_identical=all(v["same"] == "identical" for e in cases.values() for v in e["launches"].values()),
                      all_digests_identical=all(e["digests_identical"] for e in cases.values()),
                      no_difference_on_a_parent_stable_tensor=not any(e["differs_on_a_parent_stable_tensor"] for e in cases.values()),
                      parent_runs=1 + len(args.again))
        if args.bench:
            result["bench"] = load(args.bench)
    else:
        result = run_all(root, args.jobs, args.dry, args.out + ".tensors")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    if args.compare:
        print(json.dumps({k: v for k, v in result.items() if k not in ("cases", "bench")}))
        for n, e in result["cases"].items():
            if not e["digests_identical"] or any(v["same"] != "identical" for v in e["launches"].values()):
                sp = e["spreads"].values()
                print("%s: launch lists that differ %s; %d tensors differ, %d of them on a tensor the parent reproduces; largest "
                      "|parent - parent again| %s, largest |parent - this| %s" % (
                          n, [k for k, v in e["launches"].items() if v["same"] != "identical"], len(e["spreads"]),
                          len(e["differs_on_a_parent_stable_tensor"]),
                          max((x["max_abs_parent_vs_parent_again"] or 0.0 for x in sp), default=None),
                          max((x["max_abs_parent_vs_this"] or 0.0 for x in sp), default=None)))


if __name__ == "__main__":
    main()
