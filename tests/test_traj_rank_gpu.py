"""GPU tests of the candidate ranking: the kernel (a3d_traj_rank) against the float64 restatement of tests/traj_rank_ref.py, ties,
non-finite candidates, the mechanics of the entry point (guard bands, NULL outputs, determinism, the goal read in place, graph
capture) and the integration into compute_trajectory(select=...) and Actioner.predict(select=...).

Bars.  `terms` and `scores`: 5e-5 of the largest magnitude of that term (of the scores) in the call, the bar of the fp32 reductions in
tests/test_multi_candidate_gpu.py.  `best` and `order`: EXACTLY the restatement's, under a condition that is asserted on the
restatement first: every adjacent gap of a scene's sorted float64 scores is at least 1e-3 of the scene's largest score (20 times the
bar above, so no fp32 evaluation within the bar can swap two neighbours).  The seeds below were chosen on the CPU so that the
condition holds (traj_rank_ref.find_seed); no scene is skipped.  One case admits no such seed: with G = 2 the consensus term is the
same number for both candidates (d is symmetric), so there the restatement must tie exactly and the kernel's two scores must be
bit-equal -- the index decides in both (traj_rank_ref.structural_tie).

Shapes: the six of the issue, (1, 64, 64, 7) = the largest staged layout (130 KB of LDS, above the 64 KB a launch gets without asking)
and (1, 64, 100, 7), where the candidates no longer fit and are read through L2."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import traj_rank_ref as R  # noqa: E402
from test_actioner_gpu import (candidate_noise, deterministic_convolutions, make_keypose, make_planner, observation,  # noqa: E402,F401
                               set_rng, by_hand)

pytestmark = pytest.mark.gpu
TOL = 5e-5
GUARD = 64

# (B, G, L, Dp) -> mask kind -> one seed per entry of traj_rank_ref.SELECTS (consensus, goal, smooth, shortest, mixed); 0 where not
# listed.  A seed of None: the case is not run (only for the two shapes this file adds, which are there for the two memory layouts:
# every call computes and compares all five terms whatever the rule).
SEEDS = {
    (3, 5, 17, 8): {"none": (0, 0, 26, 0, 0), "suffix": (0, 0, 16, 1, 2), "scattered": (0, 0, 4, 0, 1), "padded_scene": (0, 1, 9, 0, 0)},
    (2, 8, 50, 8): {"none": (0, 0, 0, 4, 0), "suffix": (1, 2, 0, 1, 0), "scattered": (0, 0, 2, 0, 1), "padded_scene": (0, 0, 2, 0, 1)},
    (1, 64, 16, 7): {"none": (8093, 2455, 0, 0, 6994), "suffix": (25696, 138, 0, 0, 9056), "scattered": (999, 664, 0, 0, 2103),
                     "padded_scene": (0, 0, 0, 0, 0)},
    (1, 64, 64, 7): {"none": (None, 11, None, 0, None), "scattered": (None, 238, None, 0, None)},
    (1, 64, 100, 7): {"none": (None, 121, None, 0, None), "scattered": (None, 6342, None, 0, None)},
}
SHAPES = [(1, 1, 1, 7), (2, 2, 3, 7), (3, 5, 17, 8), (2, 8, 50, 8), (1, 64, 16, 7), (2, 3, 300, 8), (1, 64, 64, 7), (1, 64, 100, 7)]
CASES = [(s, m) for s in SHAPES for m in R.MASKS if s not in SEEDS or m in SEEDS[s]]


def seeds_of(shape, mask_kind):
    return SEEDS.get(shape, {}).get(mask_kind, (0,) * 5)


# ------------------------------------------------------------------------------------------------ calling the entry point
def guarded(n, dtype, dev):
    """a buffer of n elements with a poisoned band of GUARD elements on either side: (whole, view of the n elements)"""
    whole = torch.full((n + 2 * GUARD,), -7 if dtype == torch.int32 else -12345.5, device=dev, dtype=dtype)
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    want = -7 if whole.dtype == torch.int32 else -12345.5
    return bool((whole[:GUARD] == want).all()) and bool((whole[GUARD + n:] == want).all())


def raw_rank(a3d, P, mask_u8, goal, ldg, bounds, w, rw, outputs=("order", "scores", "terms", "selected")):
    """a3d_traj_rank on guarded output buffers -> dict of views (absent optional outputs are passed as NULL) + "_whole" """
    B, G, L, Dp = P.shape
    dev = P.device
    sizes = {"best": (B, torch.int32), "order": (B * G, torch.int32), "scores": (B * G, torch.float32),
             "terms": (B * G * 5, torch.float32), "selected": (B * L * Dp, torch.float32)}
    buf = {k: guarded(n, dt, dev) for k, (n, dt) in sizes.items() if k == "best" or k in outputs}
    p = lambda k: buf[k][1].data_ptr() if k in buf else None
    a3d.lib.call("a3d_traj_rank", P.data_ptr(), mask_u8.data_ptr(), None if goal is None else goal.data_ptr(), ldg,
                 None if bounds is None else bounds.data_ptr(), float(w[0]), float(w[1]), float(w[2]), float(w[3]), float(w[4]),
                 float(rw), p("best"), p("order"), p("scores"), p("terms"), p("selected"), B, G, L, Dp, a3d.lib.stream())
    torch.cuda.synchronize()
    shapes = {"best": (B,), "order": (B, G), "scores": (B, G), "terms": (B, G, 5), "selected": (B, L, Dp)}
    out = {k: v[1].view(shapes[k]) for k, v in buf.items()}
    out["_whole"] = {k: (v[0], sizes[k][0]) for k, v in buf.items()}
    return out


def to_dev(dev, P, mask, goal, bounds):
    return (torch.from_numpy(P).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev), torch.from_numpy(goal).to(dev),
            torch.from_numpy(bounds).to(dev))


# ------------------------------------------------------------------------------------------------ 1: against the restatement
@pytest.mark.parametrize("shape,mask_kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_kernel_vs_float64_restatement(a3d, dev, shape, mask_kind):
    B, G, L, Dp = shape
    ran = 0
    for si, (select, seed) in enumerate(zip(R.SELECTS, seeds_of(shape, mask_kind))):
        if seed is None:
            continue
        ran += 1
        rw = 1.0                                                   # the weight the seeds were chosen for
        P, mask, goal, bounds = R.make_case(seed, B, G, L, Dp, mask_kind)
        ref = R.rank_ref(P, mask, goal, bounds, select, rot_weight=rw)
        tie = R.structural_tie(G, select)
        # the condition for exact ranks, on the restatement, every scene
        assert R.gaps_ok(ref["scores"], exact_ties=tie), (shape, mask_kind, si, seed)
        Pd, md, gd, bd = to_dev(dev, P, mask, goal, bounds)
        got = raw_rank(a3d, Pd, md, gd, 8, bd, R.weights_of(select), rw)
        name = "traj_rank %s %s %s" % ("x".join(map(str, shape)), mask_kind, select if isinstance(select, str) else "mixed")
        terms = got["terms"].cpu().numpy().astype(np.float64)
        worst = []
        for k, term in enumerate(R.TERMS):
            scale = np.abs(ref["terms"][..., k]).max()
            err = np.abs(terms[..., k] - ref["terms"][..., k]).max()
            worst.append("%s %.2e/%.2e" % (term, err, scale))
            assert err <= TOL * scale, "%s: %s max err %.3e > %g * %.3e" % (name, term, err, TOL, scale)
        scores = got["scores"].cpu().numpy().astype(np.float64)
        s_scale, s_err = np.abs(ref["scores"]).max(), np.abs(scores - ref["scores"]).max()
        print("[parity] %s: max_abs_err/ref_absmax %s; scores %.2e/%.2e" % (name, ", ".join(worst), s_err, s_scale))
        assert s_err <= TOL * s_scale, "%s: scores max err %.3e > %g * %.3e" % (name, s_err, TOL, s_scale)
        if tie:
            assert np.array_equal(ref["scores"][:, 0], ref["scores"][:, 1]) and torch.equal(got["scores"][:, 0], got["scores"][:, 1])
        assert np.array_equal(got["best"].cpu().numpy(), ref["best"]), name
        assert np.array_equal(got["order"].cpu().numpy(), ref["order"]), name
        assert torch.equal(got["selected"], Pd[torch.arange(B, device=dev), got["best"].long()]), name
        assert np.array_equal(got["selected"].cpu().numpy(), ref["selected"]), name
        for k, (whole, n) in got["_whole"].items():
            assert guards_intact(whole, n), (name, k)
    assert ran > 0


# ------------------------------------------------------------------------------------------------ 2: ties
@pytest.mark.parametrize("G,L", [(4, 16), (7, 50), (64, 16)])
def test_identical_candidates_tie_to_the_lowest_index(a3d, dev, G, L):
    P, mask, goal, bounds = R.make_case(1, 2, G, L, 8, "scattered")
    P[:] = P[:, :1]
    Pd, md, gd, bd = to_dev(dev, P, mask, goal, bounds)
    got = raw_rank(a3d, Pd, md, gd, 8, bd, R.weights_of(R.MIXED), 1.0)
    assert (got["best"] == 0).all() and torch.equal(got["order"], torch.arange(G, device=dev, dtype=torch.int32).expand(2, G))
    assert torch.equal(got["scores"], got["scores"][:, :1].expand(2, G)) and torch.isfinite(got["scores"]).all()
    assert (got["terms"][..., 0] == 0).all()                      # every pair distance is an exact 0, rotation part included


def test_a_duplicated_medoid_wins_at_its_first_index(a3d, dev):
    """candidates 1 and 3 are the same trajectory, the one in the middle of the others: both score alike, bit for bit, below the
    rest, and the lower index is selected"""
    B, G, L = 2, 5, 17
    P, mask, goal, bounds = R.make_case(2, B, G, L, 8, "suffix")
    far = np.array([[0.2, 0, 0], [0, 0, 0], [-0.2, 0, 0], [0, 0, 0], [0, 0.3, 0]], dtype=np.float32).reshape(1, G, 1, 3)
    P[:] = P[:, 1:2]                                              # everyone is candidate 1 ...
    P[..., :3] += far                                             # ... shifted: 0 and 2 to either side, 4 further away; 3 stays put
    Pd, md, gd, bd = to_dev(dev, P, mask, goal, bounds)
    ref = R.rank_ref(P, mask, goal, bounds, "consensus")
    assert (ref["best"] == 1).all() and (ref["order"][:, 1] == 3).all()
    got = raw_rank(a3d, Pd, md, gd, 8, bd, R.weights_of("consensus"), 1.0)
    assert (got["best"] == 1).all() and (got["order"][:, 0] == 1).all() and (got["order"][:, 1] == 3).all()
    assert torch.equal(got["scores"][:, 1], got["scores"][:, 3])
    assert torch.equal(got["selected"], Pd[:, 1])


# ------------------------------------------------------------------------------------------------ 3: non-finite candidates
@pytest.mark.parametrize("select", ["consensus", "shortest", R.MIXED], ids=["consensus", "shortest", "mixed"])
def test_a_nan_candidate_is_ranked_last_and_never_selected(a3d, dev, select):
    B, G, L = 3, 4, 16
    P, mask, goal, bounds = R.make_case(3, B, G, L, 8, "suffix")
    for b in range(B):
        P[b, b % G] = np.nan                                      # candidate 0 of scene 0 included: the index tie-break must not pick it
    ref = R.rank_ref(P, mask, goal, bounds, select)
    Pd, md, gd, bd = to_dev(dev, P, mask, goal, bounds)
    got = raw_rank(a3d, Pd, md, gd, 8, bd, R.weights_of(select), 1.0)
    bad = torch.arange(B, device=dev) % G
    assert torch.equal(got["order"][:, -1].long(), bad) and (got["best"].long() != bad).all()
    assert torch.isinf(got["scores"][torch.arange(B, device=dev), bad]).all() and torch.isfinite(got["selected"]).all()
    fin = np.isfinite(ref["scores"])
    assert fin.sum() == B * (G - 1)                               # the others keep finite scores, in the restatement and here
    np.testing.assert_allclose(got["scores"].cpu().numpy()[fin], ref["scores"][fin], rtol=0, atol=TOL * np.abs(ref["scores"][fin]).max())
    assert np.array_equal(got["best"].cpu().numpy(), ref["best"])


def test_all_nan_selects_candidate_zero_and_keeps_the_nans_visible(a3d, dev):
    B, G, L = 2, 3, 16
    P, mask, goal, bounds = R.make_case(4, B, G, L, 7, "none")
    P[1] = np.nan
    Pd, md, gd, bd = to_dev(dev, P, mask, goal, bounds)
    got = raw_rank(a3d, Pd, md, gd, 8, bd, R.weights_of("consensus"), 1.0)
    assert int(got["best"][1]) == 0 and got["order"][1].tolist() == [0, 1, 2] and torch.isinf(got["scores"][1]).all()
    assert torch.isnan(got["selected"][1]).all() and torch.isfinite(got["selected"][0]).all() and torch.isfinite(got["scores"][0]).all()


# ------------------------------------------------------------------------------------------------ 4: mechanics
def test_null_outputs_determinism_and_the_goal_read_in_place(a3d, dev):
    B, G, L, Dp = 3, 5, 17, 8
    P, mask, goal, bounds = R.make_case(7, B, G, L, Dp, "scattered")
    Pd, md, gd, bd = to_dev(dev, P, mask, goal, bounds)
    w = R.weights_of(R.MIXED)
    full = raw_rank(a3d, Pd, md, gd, 8, bd, w, 1.0)
    again = raw_rank(a3d, Pd, md, gd, 8, bd, w, 1.0)
    for k in ("best", "order", "scores", "terms", "selected"):
        assert torch.equal(full[k], again[k]), k                  # a second launch: the same bits
    for outs in ((), ("order",), ("scores", "selected"), ("terms",)):
        part = raw_rank(a3d, Pd, md, gd, 8, bd, w, 1.0, outputs=outs)
        assert set(part) == set(outs) | {"best", "_whole"}
        for k in ("best",) + outs:
            assert torch.equal(part[k], full[k]), (outs, k)
        for k, (whole, n) in part["_whole"].items():
            assert guards_intact(whole, n), (outs, k)
    # the goal as the first 7 channels of (B, 8) rows, leading dimension 8, against a packed (B, 7) copy at leading dimension 7
    packed = gd[:, :7].contiguous()
    assert torch.equal(raw_rank(a3d, Pd, md, packed, 7, bd, w, 1.0)["terms"], full["terms"])
    wide = torch.full((B, 12), float("nan"), device=dev)
    wide[:, :7] = gd[:, :7]
    assert torch.equal(raw_rank(a3d, Pd, md, wide, 12, bd, w, 1.0)["terms"], full["terms"])
    # no goal, no bounds: those terms are 0 and the rest is unchanged
    w0 = R.weights_of({"consensus": 1.0, "smooth": 20.0, "length": 0.3})
    bare = raw_rank(a3d, Pd, md, None, 0, None, w0, 1.0)
    assert (bare["terms"][..., [1, 4]] == 0).all() and torch.equal(bare["terms"][..., [0, 2, 3]], full["terms"][..., [0, 2, 3]])
    # the public function: the same launch, the goal row slice read in place
    rk = a3d.rank_trajectories(Pd, md.bool(), goal=gd[:, :7], bounds=bd, select=R.MIXED)
    for k in ("best", "order", "scores", "terms", "selected"):
        assert torch.equal(getattr(rk, k), full[k]), k
    # the staged and the L2 layout compute the same bits: L = 100 rows of which only the first 17 are valid
    big = np.zeros((1, 64, 100, 7), dtype=np.float32)
    big[..., 3] = 1.0
    small, _, goal1, _ = R.make_case(8, 1, 64, 17, 7, "none")
    big[:, :, :17] = small
    m_big = np.ones((1, 100), dtype=np.uint8)
    m_big[:, :17] = 0
    a = raw_rank(a3d, torch.from_numpy(big).to(dev), torch.from_numpy(m_big).to(dev), torch.from_numpy(goal1).to(dev), 8, bd, w, 1.0)
    b = raw_rank(a3d, torch.from_numpy(small).to(dev), torch.zeros(1, 17, dtype=torch.uint8, device=dev),
                 torch.from_numpy(goal1).to(dev), 8, bd, w, 1.0)
    assert torch.equal(a["terms"], b["terms"]) and torch.equal(a["order"], b["order"])


def test_one_call_captured_in_a_graph_and_replayed_with_changed_inputs(a3d, dev):
    B, G, L, Dp = 2, 8, 50, 8
    P, mask, goal, bounds = R.make_case(0, B, G, L, Dp, "suffix")
    Pd, md, gd, bd = to_dev(dev, P, mask, goal, bounds)
    sP, sm, sg = Pd.clone(), md.bool().clone(), gd.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a3d.rank_trajectories(sP, sm, goal=sg, bounds=bd, select=R.MIXED)                 # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = a3d.rank_trajectories(sP, sm, goal=sg, bounds=bd, select=R.MIXED)
    for seed, kind in ((0, "suffix"), (3, "scattered"), (1, "none")):
        P2, mask2, goal2, _ = R.make_case(seed, B, G, L, Dp, kind)
        P2d, m2d, g2d, _ = to_dev(dev, P2, mask2, goal2, bounds)
        sP.copy_(P2d), sm.copy_(m2d.bool()), sg.copy_(g2d)
        g.replay()
        eager = a3d.rank_trajectories(P2d, m2d.bool(), goal=g2d, bounds=bd, select=R.MIXED)
        for k in eager._fields:
            assert torch.equal(getattr(out, k), getattr(eager, k)), (seed, k)


# ------------------------------------------------------------------------------------------------ 5: integration
@pytest.fixture(scope="module")
def models(a3d, dev):
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        kp = make_keypose(a3d, dev)
        pl = make_planner(a3d, dev, backbone_of=kp)
        instr = torch.randn(1, 53, 512, generator=torch.Generator().manual_seed(77)).to(dev)
        o = observation(dev, 1, 2, 16)
        for _ in range(2):                       # settle the convolution library's algorithm choice
            by_hand(kp, pl, instr, o, n_steps=1)
        return kp, pl, instr
    finally:
        torch.backends.cudnn.deterministic = old


KW = dict(num_inference_steps=4, scheduler="ddim")


def hand_written(cands, mask, goal, bounds, select, rot_weight=1.0):
    """what a user writes without the option: rank the (B, G, L, Dp) candidates, index with best"""
    ref = R.rank_ref(cands.cpu().numpy(), mask.cpu().numpy(), goal.cpu().numpy(), bounds.cpu().numpy(), select, rot_weight)
    assert R.gaps_ok(ref["scores"]), ref["scores"]
    best = torch.from_numpy(ref["best"]).to(cands.device)
    return cands[torch.arange(cands.shape[0], device=cands.device), best], ref


def test_compute_trajectory_select(a3d, models, dev):
    kp, pl, instr = models
    B, G, Ln = 2, 3, 16
    o = observation(dev, 51, B, Ln)
    init, _ = candidate_noise(dev, B, G, Ln, 4)
    goal = o["gt_action"][:, -1, :7]
    args = (o["mask"], o["rgbs"][:, -1] / 2 + 0.5, o["pcds"][:, -1], instr.expand(B, -1, -1).contiguous(), o["gripper"][:, -1, :7], goal)
    kw = dict(KW, num_samples=G, init_noise=init)
    cands = pl.compute_trajectory(*args, **kw)
    assert cands.shape == (B, G, Ln, 7)
    assert torch.equal(pl.compute_trajectory(*args, select=None, **kw), cands)            # None: today's call
    before = pl.last_ranking
    sel = pl.compute_trajectory(*args, select="consensus", **kw)
    rk = pl.last_ranking
    assert rk is not before and sel.shape == (B, Ln, 7)                                    # the single-trajectory shape
    assert torch.equal(rk.candidates, cands) and torch.equal(sel, rk.selected)
    assert torch.equal(sel, cands[torch.arange(B, device=dev), rk.best.long()])
    want, ref = hand_written(cands, o["mask"], goal, pl.gripper_loc_bounds, "consensus")
    assert np.array_equal(rk.best.cpu().numpy(), ref["best"]) and torch.equal(sel, want)
    assert rk.order.shape == (B, G) and rk.scores.shape == (B, G) and rk.terms.shape == (B, G, 5)
    # another rule and rotation weight reach the kernel
    sel2 = pl.compute_trajectory(*args, select={"goal": 1.0, "length": 0.25}, rot_weight=0.5, **kw)
    want2, ref2 = hand_written(cands, o["mask"], goal, pl.gripper_loc_bounds, {"goal": 1.0, "length": 0.25}, 0.5)
    assert torch.equal(sel2, want2)
    np.testing.assert_allclose(pl.last_ranking.scores.cpu().numpy(), ref2["scores"], rtol=0, atol=TOL * np.abs(ref2["scores"]).max())
    # through forward(run_inference=True), with the trace: entries stay per candidate
    out, trace = pl(None, *args, run_inference=True, select="consensus", return_trace=True, **kw)
    assert out.shape == (B, Ln, 7) and torch.equal(out, pl.last_ranking.selected)
    assert len(trace) == 4 and all(x.shape == (B, G, Ln, 9) for x in trace)
    # the captured loop, then the ranking launch after the replay
    for _ in range(2):
        assert torch.equal(pl.compute_trajectory(*args, select="consensus", use_graph=True, **kw), sel)
    assert torch.equal(pl.compute_trajectory(*args, use_graph=True, **kw), cands)
    pl._graph = None


def test_actioner_predict_select(a3d, models, dev):
    kp, pl, instr = models
    B, G, Ln = 2, 3, 16
    o = observation(dev, 52, B, Ln)
    init, _ = candidate_noise(dev, B, G, Ln, 4, seed=10)
    rule = {"consensus": 1, "smooth": 0.5}
    act = a3d.Actioner(kp, pl, predict_trajectory=True)
    act.set_instruction(instr)
    set_rng(kp)
    all_ = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], num_samples=G, init_noise=init, **KW)
    assert all_["trajectory"].shape == (B, G, Ln, 7) and act.last_ranking is None
    set_rng(kp)
    out = act.predict(o["rgbs"], o["pcds"], o["gripper"], None, o["mask"], num_samples=G, init_noise=init, select=rule, **KW)
    # (B, L, pose width): 7 for the 7-channel rows this planner is given (8 with action_dim = 8)
    assert out["trajectory"].shape == (B, Ln, 7) and torch.equal(out["action"], all_["action"])
    assert act.last_ranking is pl.last_ranking and torch.equal(act.last_ranking.candidates, all_["trajectory"])
    want, ref = hand_written(all_["trajectory"], o["mask"], out["action"][..., :7], pl.gripper_loc_bounds, rule)
    assert torch.equal(out["trajectory"], want) and np.array_equal(act.last_ranking.best.cpu().numpy(), ref["best"])
