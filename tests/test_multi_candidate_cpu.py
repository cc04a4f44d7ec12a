"""Several candidate trajectories per scene (compute_trajectory(num_samples=G), a3d_dn_persist_group) on the host: the new C-ABI
entry (export, ctypes signature, header arity, argument validation without a GPU), the argument errors of the public interface, and
the group / chunk index algebra of the persistent sampler's two roles against a brute-force enumeration."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_pkg

T = 100
SHAPES = [(1, 16), (4, 16), (5, 16), (3, 20), (2, 50), (3, 64)]          # (G, L)


def test_group_entry_is_exported_with_a_signature_of_the_header_arity():
    a3d = load_pkg()
    lib = a3d.lib.load()
    header = open(os.path.join(ROOT, "include", "act3d_hip.h")).read()
    for name in ("a3d_dn_persist_group", "a3d_dn_persist_group_of"):
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, "%s is not declared in include/act3d_hip.h" % name
        n_header = len([p for p in m.group(1).split(",") if p.strip()])
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_header, (name, len(fn.argtypes or ()), n_header)
    # the arguments of a3d_dn_persist_sched plus n_cand
    assert len(lib.a3d_dn_persist_group.argtypes) == len(lib.a3d_dn_persist_sched.argtypes) + 1


def test_group_c_abi_argument_validation_without_gpu():
    """a3d_dn_persist_group rejects bad arguments on the host before any launch, with -22 and its own name in
    a3d_last_error_string: the candidate count, and everything a3d_dn_persist_sched rejects; the two older entries still answer
    under their own names."""
    a3d = load_pkg()
    lib = a3d.lib.load()
    L = a3d.lib
    d = ctypes.c_void_p(64)                                                          # aligned, never dereferenced
    hp = L.DnHeadParams(enc_w0=64, enc_w1=64)
    tp = L.DnTailParams(pos_w0=64, rot_w0=64, coef_pos=64, coef_rot=64)

    def group(B=4, Ln=16, D=9, E=120, H=8, S=100, Sp=128, nsplit=2, row_first=0, nsteps=10, n_rows=10, last=1, n_cand=2, head=hp, tail=tp,
              kvx=None, sync=d, stacks=(4, 2, 2)):
        return lib.a3d_dn_persist_group(d, stacks[0], stacks[1], stacks[2], ctypes.byref(head), ctypes.byref(tail), d, d, d, kvx, d, sync,
                                        B, Ln, D, E, H, S, Sp, nsplit, row_first, nsteps, n_rows, last, n_cand, None)

    def refused(rc, name="a3d_dn_persist_group", also=b""):
        assert rc == -22, name
        msg = lib.a3d_last_error_string()
        assert (name + ":").encode() in msg and also in msg, msg

    refused(group(n_cand=0), also=b"n_cand=0")
    refused(group(n_cand=-2), also=b"n_cand=-2")
    refused(group(B=4, n_cand=3), also=b"n_cand=3")                                  # B % n_cand != 0
    refused(group(B=2, n_cand=4), also=b"n_cand=4")
    refused(group(Ln=65))                                                            # L > 64
    refused(group(E=121))                                                            # E != 15 H
    refused(group(B=0))
    refused(group(nsteps=0))
    refused(group(nsteps=11))                                                        # more steps than table rows
    refused(group(row_first=1))
    refused(group(row_first=-1))
    refused(group(n_rows=0, nsteps=1))
    refused(group(last=2))
    refused(group(last=-1))
    refused(group(Sp=100))                                                           # Sp % 64
    refused(group(nsplit=0))
    refused(group(D=17))
    refused(group(Ln=50))                                                            # four row tiles need the kvx exchange buffer
    refused(group(sync=None))
    refused(group(stacks=(4, 0, 2)))
    refused(group(tail=L.DnTailParams(pos_w0=64, rot_w0=64, coef_pos=64)))           # no rotation table
    refused(group(tail=L.DnTailParams(pos_w0=64, rot_w0=64, coef_pos=64, coef_rot=64, cond_mask=64)))
    # the older entries keep their names
    rc = lib.a3d_dn_persist_sched(d, 4, 2, 2, ctypes.byref(hp), ctypes.byref(tp), d, d, d, None, d, d, 2, 16, 9, 120, 8, 100, 128, 2, 0, 11,
                                  10, 1, None)
    assert rc == -22 and b"a3d_dn_persist_sched:" in lib.a3d_last_error_string()
    rc = lib.a3d_dn_persist(d, 4, 2, 2, ctypes.byref(hp), ctypes.byref(tp), d, d, d, None, d, d, 2, 16, 9, 120, 8, 100, 128, 2, 3, 10, None)
    assert rc == -22 and b"a3d_dn_persist:" in lib.a3d_last_error_string() and b"from t=3" in lib.a3d_last_error_string()
    out = (ctypes.c_int * 5)()
    assert lib.a3d_dn_persist_group_of(6, 16, 4, 0, out) == -22 and b"a3d_dn_persist_group_of:" in lib.a3d_last_error_string()
    assert lib.a3d_dn_persist_group_of(6, 16, 3, 6, out) == -22
    assert lib.a3d_dn_persist_group_of(6, 16, 3, 0, None) == -22


@pytest.mark.parametrize("G,Ln", SHAPES)
def test_workspace_sizes_follow_the_trajectory_count(G, Ln):
    """Every workspace of the persistent sampler is per trajectory: its size for B = scenes x n_cand is what the single-candidate
    call of B trajectories asks for (the group entry adds no query), linear in B where it is linear at all."""
    lib = load_pkg().lib.load()
    scenes, E, H, n_layers = 3, 120, 8, 8
    B = scenes * G
    NT = -(-Ln // 16)
    assert lib.a3d_dn_persist_xbuf_floats(B, Ln) == G * lib.a3d_dn_persist_xbuf_floats(scenes, Ln) == B * NT * 2 * 16 * 128
    assert lib.a3d_dn_persist_kvx_floats(B, Ln, E) == G * lib.a3d_dn_persist_kvx_floats(scenes, Ln, E)
    assert (lib.a3d_dn_persist_kvx_floats(B, Ln, E) == 0) == (NT == 1)
    nse = lib.a3d_dn_persist_splits(H, 2)
    assert lib.a3d_dn_cross_ws_floats(2 * B * NT, H, nse) == G * lib.a3d_dn_cross_ws_floats(2 * scenes * NT, H, nse)
    n10, n100 = lib.a3d_dn_persist_sync_ints(B, Ln, n_layers, 10), lib.a3d_dn_persist_sync_ints(B, Ln, n_layers, 100)
    # the ready queue holds one slot per (step, layer, group); groups <= trajectories x tiles, which is what it is sized for
    out = (ctypes.c_int * 5)()
    assert lib.a3d_dn_persist_group_of(B, Ln, G, 0, out) == 0
    groups = out[0]
    assert groups <= B * NT and 0 < n10 < n100 and n100 - n10 >= 90 * n_layers * groups


def test_compute_trajectory_num_samples_raises_before_any_launch():
    """num_samples and the shapes of the injected noise are checked on the host: on CPU tensors the bad calls raise ValueError
    (a good call would go on to the kernels, which need the GPU)."""
    a3d = load_pkg()
    m = a3d.DiffusionPlanner(embedding_dim=60, num_attn_heads=4, num_query_cross_attn_layers=6, use_instruction=True, use_goal=True,
                             gripper_loc_bounds=[[-1, -1, -1], [1, 1, 1]], rotation_parametrization="6D", diffusion_timesteps=T)
    B, Ln, G, D = 2, 8, 3, 10                                   # 8 pose channels -> D = 10 signal channels
    mask = torch.zeros(B, Ln, dtype=torch.bool)
    args = (mask, None, torch.zeros(B, 1, 3, 16, 16), torch.zeros(B, 53, 512), torch.zeros(B, 8), torch.zeros(B, 8))
    z = torch.zeros
    bad = [dict(num_samples=0), dict(num_samples=-1), dict(num_samples=2.5), dict(num_samples="4"), dict(num_samples=True),
           dict(num_samples=G, init_noise=z(B * G, Ln, D)),                              # rank
           dict(num_samples=G, init_noise=z(B, G + 1, Ln, D)),
           dict(num_samples=G, init_noise=z(G, B, Ln, D)),                               # candidate-major
           dict(num_samples=G, init_noise=z(B, G, Ln, D - 1)),
           dict(num_samples=G, step_noise=z(T, B * G, Ln, D)),                           # rank
           dict(num_samples=G, step_noise=z(T, B, G, Ln + 1, D)),
           dict(num_samples=G, step_noise=z(T - 1, B, G, Ln, D)),                        # one row per step of the full chain
           dict(num_samples=G, num_inference_steps=10, step_noise=z(T, B, G, Ln, D)),    # ... or of the schedule
           dict(num_samples=G, num_inference_steps=10, step_noise=z(10, B, Ln, D)),
           dict(num_samples=G, num_inference_steps=0), dict(num_samples=G, scheduler="euler"), dict(num_samples=1, eta=0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            m.compute_trajectory(*args, **kw)
        with pytest.raises(ValueError):                       # and through forward(run_inference=True, ...)
            m(None, *args, run_inference=True, **kw)
    D_ = a3d.diffusion
    assert D_.check_num_samples(1) == 1 and D_.check_num_samples(7) == 7
    D_.check_candidate_noise(z(B, G, Ln, D), z(T, B, G, Ln, D), B, G, Ln, D, T)
    D_.check_candidate_noise(None, None, B, G, Ln, D, T)


# ---- the index algebra of the two roles (csrc/denoise.hip: dnp_chunk / dnp_nchunk / dnp_group_tiles), restated in numpy
def model(scenes, G, Ln):
    """Closed forms: per trajectory j -> (scene, chunk, group id within a role, first unit, tile count); units u = j NT + tile."""
    NT = -(-Ln // 16)
    cs = max(1, 4 // NT)
    nch = -(-G // cs)
    j = np.arange(scenes * G)
    scene, cand = j // G, j % G
    chunk = cand // cs
    grp = scene * nch + chunk
    first = (scene * G + chunk * cs) * NT
    tiles = np.minimum(cs, G - chunk * cs) * NT
    return dict(NT=NT, cs=cs, nch=nch, groups=scenes * nch, scene=scene, chunk=chunk, grp=grp, first=first, tiles=tiles)


def brute_force(scenes, G, Ln):
    """The grouping by enumeration: walk the scenes, cut each scene's candidates into runs of at most max(1, 4 // NT), give every
    run the next group id and list its (trajectory, tile) units in order."""
    NT = len(range(0, Ln, 16))
    per_chunk = 1
    while (per_chunk + 1) * NT <= 4:
        per_chunk += 1
    groups, j = [], 0
    for s in range(scenes):
        left = G
        while left > 0:
            n = min(per_chunk, left)
            groups.append({"scene": s, "units": [(jj, t) for jj in range(j, j + n) for t in range(NT)]})
            j += n
            left -= n
    assert j == scenes * G
    return NT, groups


@pytest.mark.parametrize("G,Ln", SHAPES)
def test_group_and_chunk_index_algebra(G, Ln):
    lib = load_pkg().lib.load()
    scenes = 3
    B = scenes * G
    mo = model(scenes, G, Ln)
    NT, groups = brute_force(scenes, G, Ln)
    assert mo["NT"] == NT and mo["groups"] == len(groups)
    assert mo["cs"] == {1: 4, 2: 2, 3: 1, 4: 1}[NT]
    covered = set()
    for gid, g in enumerate(groups):
        units = g["units"]
        assert 1 <= len(units) <= 4, "a group exceeds the four tiles the streaming item is instantiated for"
        flat = [jj * NT + t for jj, t in units]
        assert flat == list(range(flat[0], flat[0] + len(flat))), "a group's units are consecutive"
        for jj, t in units:
            # trajectory -> scene, candidate -> chunk, tiles per group, unit <-> (trajectory, tile)
            assert mo["scene"][jj] == g["scene"] == jj // G
            assert mo["grp"][jj] == gid and mo["first"][jj] == flat[0] and mo["tiles"][jj] == len(units)
            u = jj * NT + t
            assert (u // NT, u % NT) == (jj, t) and u not in covered
            covered.add(u)
            assert 16 * t < Ln                                    # the tile's row offset lies within its OWN trajectory
    assert covered == set(range(B * NT))
    # the library's host mirror evaluates the device functions themselves
    out = (ctypes.c_int * 5)()
    for jj in range(B):
        assert lib.a3d_dn_persist_group_of(B, Ln, G, jj, out) == 0
        assert list(out) == [mo["groups"], mo["grp"][jj], mo["first"][jj], mo["tiles"][jj], mo["scene"][jj]], (jj, list(out))
    # the queue code 1 + layer * 2 groups + role * groups + group decodes uniquely
    codes = {1 + l * 2 * mo["groups"] + role * mo["groups"] + gid for l in range(8) for role in range(2) for gid in range(mo["groups"])}
    assert len(codes) == 8 * 2 * mo["groups"] and min(codes) == 1
    # the stated cases
    if (G, Ln) == (4, 16):
        assert mo["nch"] == 1 and set(mo["tiles"]) == {4}                     # one K / V pass serves all four candidates
    if (G, Ln) == (2, 50):
        assert mo["nch"] == 2 and set(mo["tiles"]) == {4}                     # every candidate has its own items
    if (G, Ln) == (3, 20):
        assert [len(g["units"]) for g in groups[:2]] == [4, 2]                # chunks of 2 and 1 candidates
    if (G, Ln) == (5, 16):
        assert [len(g["units"]) for g in groups[:2]] == [4, 1]
    if G == 1:
        assert (mo["grp"] == np.arange(B)).all() and set(mo["tiles"]) == {NT}   # a group is a trajectory: the single-candidate kernel
