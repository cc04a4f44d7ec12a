#!/usr/bin/env python3
"""One a3d_ctx_kv_proj16(nl = 2) launch against the two a3d_proj_rope_split16 k | v launches it replaces, at the keypose step's shape
(B = 64, S = 4097, E = 60, H = 4), events on the launch stream as bench.time_kernel.  Prints one JSON line.

usage: python profiles/ctx_kv_proj_probe.py [--iters 50] [--only both|new|old] [--B 64] [--S 4097] [--splits 0]
Under `rocprofv3 --kernel-trace --pmc ...` (profiles/pmc_json_cmd.sh) use --iters 3: the counters are per launch.
Floors of the new launch (derived in DESIGN section 4): HBM 63 MB of X + 272 MB of rows = 335 MB -> 42 us at 8 TB/s; f32 MFMA issue
4 x 60 v_mfma_f32_16x16x4 (8 passes = 32 cycles each) per 16 keys on 1024 SIMDs -> 51 us at 2.4 GHz, 62 us at 2.0 GHz.
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_kernel(fn, iters):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default="both", choices=("both", "new", "old"))
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--S", type=int, default=4097)
    ap.add_argument("--splits", type=int, default=0)
    a = ap.parse_args()
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    O, L = a3d.ops, a3d.lib
    dev = torch.device("cuda:0")
    B, S, E, H = a.B, a.S, 60, 4
    Sp = (S + 63) // 64 * 64
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, E, generator=g).to(dev)
    xyz = torch.rand(B, S, 3, generator=g).to(dev)
    w = [(torch.randn(3 * E, E, generator=g) * E ** -0.5).to(dev) for _ in range(2)]
    bb = [torch.randn(3 * E, generator=g).to(dev) for _ in range(2)]
    freq = O.rope_freq(E, dev)
    rows = lambda: torch.empty((B, H, Sp, 32), device=dev, dtype=torch.float16)
    new_o = [(rows(), rows()) for _ in range(2)]
    old_o = [(rows(), rows()) for _ in range(2)]
    st = L.stream()

    def new():
        args = []
        for l in range(2):
            args += [w[l].data_ptr() + E * E * 4, bb[l].data_ptr() + E * 4, new_o[l][0].data_ptr(), new_o[l][1].data_ptr()]
        L.call("a3d_ctx_kv_proj16", x.data_ptr(), E, xyz.data_ptr(), *args, E, freq.data_ptr(), 2, B, S, Sp, E, H, a.splits, st)

    def old():
        for l in range(2):
            L.call("a3d_proj_rope_split16", x.data_ptr(), E, w[l].data_ptr() + E * E * 4, E, bb[l].data_ptr() + E * 4, E,
                   xyz.data_ptr(), 1.0, old_o[l][0].data_ptr(), None, 2, None, 1.0, old_o[l][1].data_ptr(), None, O.V_ROWS,
                   freq.data_ptr(), B, S, Sp, E, H, st)

    out = {"probe": "ctx_kv_proj", "B": B, "S": S, "E": E, "H": H, "iters": a.iters,
           "splits": a.splits or L.load().a3d_ctx_kv_proj16_splits(B, Sp), "device": torch.cuda.get_device_name(0)}
    if a.only in ("both", "old"):
        out["old_two_launches_us"] = 1e3 * time_kernel(old, a.iters)
    if a.only in ("both", "new"):
        out["new_one_launch_us"] = 1e3 * time_kernel(new, a.iters)
    if a.only == "both":
        # a second pair in the other order: the two figures must not depend on which ran first (clocks, cache state)
        out["new_one_launch_us_2"] = 1e3 * time_kernel(new, a.iters)
        out["old_two_launches_us_2"] = 1e3 * time_kernel(old, a.iters)
        differ = sum(int((n.view(torch.int16) != o.view(torch.int16)).sum()) for np_, op in zip(new_o, old_o) for n, o in zip(np_, op))
        out["elements_differing_in_bits"] = differ
        out["elements"] = 4 * new_o[0][0].numel()
        err = max(float((n.float().view(B, H, Sp, 2, 16).sum(3) - o.float().view(B, H, Sp, 2, 16).sum(3)).abs().max())
                  for np_, op in zip(new_o, old_o) for n, o in zip(np_, op))
        out["max_abs_diff_of_carried_values"] = err
    bytes_new = B * (S * E * 4.0 + 4 * H * Sp * 32 * 2.0)
    out["needed_MB_new"] = bytes_new / 1e6
    out["floors_us"] = {"hbm_8TBs": bytes_new / 8e12 * 1e6, "mfma_f32_issue_2.4GHz": B * ((S + 15) // 16) * 240 * 32 / 1024 / 2.4e3,
                        "mfma_f32_issue_2.0GHz": B * ((S + 15) // 16) * 240 * 32 / 1024 / 2.0e3}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
