"""Equivalence record of the attention-block refactor: for every case of tests/attn_block_cases.py (and the cached inference pair,
fused and unfused) the entry names recorded at lib.call and the SHA-256 digests of y, every input gradient and the in_proj / out_proj /
LayerNorm gradients.  Run once on each tree and compare:

    python profiles/attn_block_plan_equivalence.py --out this.json                     # this tree
    python profiles/attn_block_plan_equivalence.py --root PARENT_CHECKOUT --out parent.json
    python profiles/attn_block_plan_equivalence.py --compare parent.json this.json [--again parent2.json ...] [--bench bench.json] \
        --out profiles/attn_block_plan_equivalence.json

Each run also leaves the tensors themselves next to its JSON (FILE.tensors/<case>.npz, not kept): for a tensor whose digests differ
--compare reads them and records the largest absolute difference between the parent's runs and between the trees.

--root names the checkout whose package is imported (the cases and the runner are always this tree's).  Every case runs in a fresh
child process with fixed seeds (at most --jobs at a time).  --compare: launch lists must be equal up to the a3d_rope_split_qk /
a3d_split_vt wrapper names and, in the "qk" / "none" backward, up to order; a digest that differs is reported with the parent's own
run-to-run result from --again.
"""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASE_SECONDS = 120                 # one case: a fresh process, the library load and a few small launches
WRAPPERS = {"a3d_rope_split_qk": "a3d_rope_split", "a3d_split_vt": "a3d_rope_split"}


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def save(tensors_dir, name, tensors):
    import numpy as np
    if tensors_dir:
        os.makedirs(tensors_dir, exist_ok=True)
        np.savez(os.path.join(tensors_dir, name.replace(" ", "_").replace(",", "") + ".npz"),
                 **{k: v.detach().cpu().numpy() for k, v in tensors.items()})


def spread(dir_a, dir_b, name, key):
    """largest |a - b| of one tensor between two runs (None when a run kept no tensors)"""
    import numpy as np
    f = name.replace(" ", "_").replace(",", "") + ".npz"
    if not (dir_a and dir_b and os.path.exists(os.path.join(dir_a, f)) and os.path.exists(os.path.join(dir_b, f))):
        return None
    return float(np.abs(np.load(os.path.join(dir_a, f))[key].astype(np.float64) - np.load(os.path.join(dir_b, f))[key]).max())


def run_one(root, name, tensors_dir=None):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, root)
    import torch
    import attn_block_cases as AC
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    if name.startswith("cached "):
        a3d.ops.FUSED_PROJ = name == "cached fused"
        build, block, y = AC.run_cached(a3d, dev)
        save(tensors_dir, name, {"y": y})
        return dict(fwd=build + block, bwd=None, digests={"y": digest(y)})
    c = next(c for c in AC.CASES if c["name"] == name)
    for k, v in c["switches"].items():
        assert hasattr(a3d.ops, k), k
        setattr(a3d.ops, k, v)
    r = AC.run_case(a3d, dev, c)
    save(tensors_dir, name, r["tensors"])
    out = dict(fwd=r["fwd"], bwd=r["bwd"], digests={k: digest(v) for k, v in r["tensors"].items()})
    if hasattr(a3d.ops, "attn_block_plan"):
        route = a3d.ops.attn_block_plan(**r["plan"])
        out["route"] = dict(family=route.family, operands=route.operands, projection=route.projection, core_fwd=route.core_fwd,
                            core_bwd=route.core_bwd, nsplit=route.nsplit)
    return out


def run_all(root, jobs, tensors_dir):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import attn_block_cases as AC
    names = [c["name"] for c in AC.CASES] + ["cached fused", "cached unfused"]
    results, pending = {}, list(names)
    running = []
    while pending or running:
        while pending and len(running) < jobs:
            n = pending.pop(0)
            running.append((n, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--root", root, "--case", n, "--tensors", tensors_dir],
                                                stdout=subprocess.PIPE, text=True)))
        n, p = running.pop(0)
        try:
            stdout, _ = p.communicate(timeout=CASE_SECONDS)
            status = p.returncode and "exit status %d" % p.returncode
        except subprocess.TimeoutExpired:
            status = "no result within %d s" % CASE_SECONDS
        if status:                                                 # nothing more is started, nothing is left running
            for _, q in [(n, p)] + running:
                q.kill()
                q.wait()
            raise SystemExit("case %r: %s; its siblings were ended and nothing more is started" % (n, status))
        results[n] = json.loads(stdout.strip().splitlines()[-1])
    return results


def compare(parent, this, again, dirs):
    report = {}
    for name, p in parent.items():
        t = this[name]
        mode = name.split()[0]
        same = {}
        for leg in ("fwd", "bwd"):
            a = None if p[leg] is None else [WRAPPERS.get(e, e) for e in p[leg]]
            b = t[leg]
            if a == b:
                same[leg] = "identical" if p[leg] == t[leg] else "identical up to wrapper names"
            elif leg == "bwd" and mode in ("qk", "none") and sorted(a) == sorted(b):
                same[leg] = "permuted"
            else:
                same[leg] = "DIFFERENT"
        differing = sorted(k for k in p["digests"] if p["digests"][k] != t["digests"].get(k))
        entry = dict(launches=same, digests_identical=not differing and set(p["digests"]) == set(t["digests"]), parent=p, this=t)
        if differing:
            worst = lambda pairs, k: max((x for x in (spread(a, b, name, k) for a, b in pairs) if x is not None), default=None)
            entry["differing"] = {k: dict(stable_on_parent=all(a[name]["digests"][k] == p["digests"][k] for a in again) if again else None,
                                          max_abs_parent_vs_parent_again=worst([(dirs[0], d) for d in dirs[2:]], k),
                                          max_abs_parent_vs_this=spread(dirs[0], dirs[1], name, k),
                                          max_abs_parent_again_vs_this=worst([(d, dirs[1]) for d in dirs[2:]], k)) for k in differing}
        if again:
            entry["parent_unstable"] = sorted(k for k in p["digests"] if any(a[name]["digests"][k] != p["digests"][k] for a in again))
        report[name] = entry
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=REPO)
    ap.add_argument("--case")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--again", nargs="*", default=[], help="further runs of the parent: its own run-to-run spread")
    ap.add_argument("--bench")
    ap.add_argument("--tensors", help="(with --case) directory that receives the case's tensors")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.case:
        print(json.dumps(run_one(root, args.case, args.tensors)))
        return
    load = lambda f: json.load(open(f))
    if args.compare:
        dirs = [f + ".tensors" for f in args.compare + args.again]
        cases = compare(load(args.compare[0]), load(args.compare[1]), [load(f) for f in args.again], dirs)
        result = dict(cases=cases,
                      all_launch_lists_equivalent=all("DIFFERENT" not in e["launches"].values() for e in cases.values()),
                      all_digests_identical=all(e["digests_identical"] for e in cases.values()))
        import numpy as np
        cached = {}
        for tree, d in zip(("parent", "this"), dirs):                  # the cached pair's own relation: fused against unfused output
            f, u = (os.path.join(d, "cached_%s.npz" % n) for n in ("fused", "unfused"))
            if os.path.exists(f) and os.path.exists(u):
                yf, yu = np.load(f)["y"].astype(np.float64), np.load(u)["y"].astype(np.float64)
                cached[tree] = dict(max_abs_fused_vs_unfused=float(np.abs(yf - yu).max()), max_abs_y=float(np.abs(yu).max()),
                                    fraction_of_elements_differing=float((yf != yu).mean()))
        result["cached_pair_fused_vs_unfused"] = cached
        if args.bench:
            result["bench"] = load(args.bench)
    else:
        result = run_all(root, args.jobs, args.out + ".tensors")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    if args.compare:
        print(json.dumps({k: v for k, v in result.items() if k != "cases"}))
        for n, e in result["cases"].items():
            if not e["digests_identical"] or "DIFFERENT" in e["launches"].values():
                print(n, e["launches"], e.get("differing"))


if __name__ == "__main__":
    main()
