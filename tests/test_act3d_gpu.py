"""End-to-end parity of the HIP Act3D path (forward, loss, backward) on the MI355X:
  (1) against the golden outputs of the REFERENCE itself (tests/golden/act3d.pt), ghost points injected;
  (2) against the CPU oracle at the full cfg-2 token counts (4 cameras, 4097 context tokens, Ng=333), teacher-forced
      per level (SURVEY §0 "chaotic argmax cascade").
Tolerances: indices / argmax positions bit-exact; logits, actions, losses 1e-3 (north_star); gradients 1e-3 relative.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import common as C  # noqa: E402
from oracle import act3d as OA  # noqa: E402
from oracle import sampling as OS  # noqa: E402
from test_oracle_golden import ACT3D_TAGS, _act3d_case, act3d_params, pcd_factor  # noqa: E402

pytestmark = pytest.mark.gpu


def rel_close(name, got, ref, atol, rtol):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs()
    print(f"[parity] {name}: max_abs_err={err.max().item():.3e} ref_absmax={ref.abs().max().item():.3e}")
    assert torch.isfinite(got).all(), name
    assert (err <= atol + rtol * ref.abs()).all(), f"{name}: max err {err.max().item():.3e}"


def scale_close(name, got, ref, tol=5e-4, floor=1.0):
    """|got - ref| <= tol * max(1, max|ref|): north_star's bar is 1e-3 absolute for O(1) tensors; the assert is HALF of it
    (2x the worst value observed on MI355X, 2.0e-4 -- profiles/r04_parity_report.txt -- so a regression cannot hide in the
    slack), relative to the tensor's scale for the deliberately large-logit fixtures (gain-3 weights, logits up to ~25)."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs().max().item()
    scale = max(floor, ref.abs().max().item())
    print(f"[parity] {name}: max_abs_err={err:.3e} ref_absmax={ref.abs().max().item():.3e} rel_to_scale={err / scale:.2e}")
    assert torch.isfinite(got).all(), name
    assert err <= tol * scale, f"{name}: max err {err:.3e} > {tol} * {scale:.3e}"


GRAD_TOL = 1e-3        # of the tensor's scale; 2x the worst keypose gradient observed on MI355X (4.9e-4, query_embed.weight)


def build_model(a3d, dev, cfg, P, Ng, train, bounds=C.PERACT_BOUNDS, **kw):
    image = cfg.get("image", 256)
    m = a3d.act3d.Act3D(image_size=(image, image), embedding_dim=cfg["E"], num_attn_heads=4, gripper_loc_bounds=bounds,
                        num_ghost_points=Ng * cfg["levels"], num_ghost_points_val=Ng * cfg["levels"],
                        num_sampling_level=cfg["levels"], use_instruction=cfg["use_instruction"], **kw)
    res = m.load_state_dict(P, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    missing = [k for k in res.missing_keys if not k.startswith("backbone") and "feature_pyramid" not in k]
    assert not missing, missing
    m.to(dev)
    m.train(train)
    return m


def _golden_inputs(r, cfg, dev):
    inp = C.keypose_inputs(r["seed"], cfg["B"], cfg["ncam"], cfg["E"], cfg["levels"], image=cfg["image"])
    fmaps = [f.to(dev).requires_grad_(cfg["train"]) for f in inp["feats"][:2]]
    maps = [fmaps[0]] + [fmaps[-1]] * (cfg["levels"] - 1)
    tok = {}
    feats = []
    for f in maps:
        if id(f) not in tok:
            tok[id(f)] = C.tokens_from_maps(f)
        feats.append(tok[id(f)])
    return inp, fmaps, feats


def _check_golden_forward(tag, r, cfg, out, pcd):
    for i in range(cfg["levels"]):
        if i > 0:
            # ghost-point context indices: bit-exact vs the reference, up to torch.topk's unspecified order among EXACTLY
            # tied distances (every differing position is proven to be a 0-ulp tie; all goldens together hold 2 of them)
            pcd_i = OS.pcd_downsample(pcd.cpu().numpy(), pcd_factor(cfg, i))
            nt = C.assert_topk_equal_up_to_exact_ties(out["topk_indices_pyramid"][i].cpu().numpy(), r["topk"][i].numpy(),
                                                      r["positions"][i - 1].numpy(), pcd_i, f"{tag} level {i}")
            assert nt <= 4, f"{tag} level {i}: {nt} tied positions differ"
        for l in range(2):
            scale_close(f"{tag} mask L{i} layer{l}", out["ghost_pcd_masks_pyramid"][i][l], r["masks"][i][l])
        assert torch.equal(out["position_pyramid"][i][:, 0].cpu(), r["positions"][i]), f"argmax position level {i}"
    rel_close("rotation", out["rotation"], r["rotation"], 1e-3, 0)
    rel_close("gripper", out["gripper"], r["gripper"], 1e-3, 0)
    scale_close("query", out["query_features"][0], r["query_features"])
    rel_close("position", out["position"], r["position"], 1e-3, 0)
    if "offsets" in r:                                  # regress_position_offset (act3d.py:323-327)
        scale_close("offsets", out["fine_ghost_pcd_offsets"], r["offsets"])


def _check_golden_grads(r, cfg, m, fmaps):
    named = dict(m.named_parameters())
    for n, gref in r["grads"].items():
        # gain-3 fixtures: sharply peaked softmax over ~1000-4000 keys, |logit| ~ 100: fp32-grade logits are needed for the
        # Lq=1 query stream's gradients (DESIGN.md "numerics")
        scale_close("grad " + n, named[n].grad, gref, GRAD_TOL)
    bad = []
    for n, nr in r["grad_norms"].items():
        if "feature_pyramid" in n or n not in named:
            continue
        g = named[n].grad
        assert g is not None, n
        got = g.norm().item()
        print(f"[parity] grad norm {n}: {got:.6e} vs {nr:.6e} rel={abs(got - nr) / (nr + 1e-30):.2e}")
        if abs(got - nr) > 3e-3 * nr + 2e-4:
            bad.append(f"{n}: {got} vs {nr}")
    assert not bad, "gradient norms off by more than 3e-3:\n  " + "\n  ".join(bad)
    for f, nr in zip(fmaps, r["feat_grad_norms"]):
        if nr is not None:
            print(f"[parity] feature grad norm: {f.grad.norm().item():.6e} vs {nr:.6e}")
            assert abs(f.grad.norm().item() - nr) <= 3e-3 * nr + 1e-5
    if "feat1_grad_sample" in r:
        rel_close("feat grad sample", C.tokens_from_maps(fmaps[1].grad)[:, ::517], r["feat1_grad_sample"], 1e-4, 3e-3)
    if "feat0_grad_sample" in r:
        rel_close("feat grad sample", C.tokens_from_maps(fmaps[0].grad)[:, ::37], r["feat0_grad_sample"], 1e-4, 3e-3)


@pytest.mark.parametrize("tag", ACT3D_TAGS)
def test_act3d_vs_reference_golden(a3d, dev, tag):
    """Ghost points injected from the reference's record.  The two *_128_* tags are BASELINE.json configs[0]:
    batch 1, one 128x128 camera, one ghost-point level (1000 points in training, 10000 at evaluation).

    Every tag's forward comparison runs twice: with autograd recording (the parameters require gradients, so the eval tags too take
    the both-parts-P attention forward) and once more under torch.no_grad() (the adaptive-P forward that evaluation and ghost-point
    sampling run in production), against the same record at the same tolerances."""
    r, cfg, names = _act3d_case(tag)
    P = act3d_params(cfg, r["seed"], r["gain"], names)
    m = build_model(a3d, dev, cfg, P, cfg["Ng"], cfg["train"], **r.get("model_kw", {}))
    inp, fmaps, feats = _golden_inputs(r, cfg, dev)

    def fwd():
        return m(None, inp["pcd"].to(dev), inp["instr"].to(dev), inp["curr_gripper"].to(dev),
                 gt_action=inp["action"].to(dev) if cfg["train"] else None,
                 ghost_points=[g.to(dev) for g in r["ghost"]], visual_features=feats)

    with torch.no_grad():
        out_ng = fwd()
    _check_golden_forward(tag + " (no_grad)", r, cfg, out_ng, inp["pcd"])
    del out_ng
    out = fwd()
    _check_golden_forward(tag, r, cfg, out, inp["pcd"])
    if not cfg["train"]:
        return
    sample = {"action": inp["action"].to(dev), "task": ["t"] * cfg["B"]}
    if "probe" in r:           # the 6D heads have no loss in the reference: a fixed linear functional of the outputs
        losses = {k: (out[k] * w.to(dev)).sum() for k, w in r["probe"].items()}
        crit = None
    else:
        lk = dict(position_loss="ce", ground_truth_gaussian_spread=0.01,
                  rotation_parametrization=r.get("model_kw", {}).get("rotation_parametrization", "quat_from_query"))
        lk.update(r.get("loss_kw", {}))
        crit = a3d.losses.LossAndMetrics(**lk)
        losses = crit.compute_loss(out, sample)
    for k, v in r["losses"].items():
        rel_close("loss " + k, losses[k], v, 1e-3, 1e-3)
    sum(losses.values()).backward()
    _check_golden_grads(r, cfg, m, fmaps)
    if crit is not None:
        met = crit.compute_metrics(out, sample)
        for k, v in r["metrics"].items():
            rel_close("metric " + k, met[k], v, 1e-3, 0)


@pytest.mark.parametrize("tag", ["train_L3_C1_N64", "eval_L3_C1_N128", "train_128_L1_C1_N1000", "eval_128_L1_C1_N10000"])
def test_act3d_free_running_numpy_sampler(a3d, dev, tag):
    """NO injection: ghost_sampler="numpy" consumes the global numpy RNG exactly like the reference (act3d.py:394-440),
    so with the reference's seed the whole free-running step -- ghost points, k-NN sets, argmax cascade, action, and for
    the training tags the engine.train_one_step loss / gradients -- reproduces the reference's record."""
    r, cfg, names = _act3d_case(tag)
    P = act3d_params(cfg, r["seed"], r["gain"], names)
    m = build_model(a3d, dev, cfg, P, cfg["Ng"], cfg["train"], ghost_sampler="numpy")
    inp, fmaps, feats = _golden_inputs(r, cfg, dev)
    m.compute_visual_tokens = lambda rgb: feats          # the reference's record was made on injected FPN outputs
    sample = {"rgbs": torch.zeros(cfg["B"], cfg["ncam"], 3, 8, 8, device=dev), "pcds": inp["pcd"].to(dev),
              "instr": inp["instr"].to(dev), "curr_gripper": inp["curr_gripper"].to(dev), "action": inp["action"].to(dev),
              "task": ["t"] * cfg["B"]}
    np.random.seed(r["seed"])
    if not cfg["train"]:
        with torch.no_grad():
            out = m(sample["rgbs"], sample["pcds"], sample["instr"], sample["curr_gripper"], gt_action=None)
    else:
        keep = {}
        fwd = m.forward
        m.forward = lambda *a, **k: keep.setdefault("out", fwd(*a, **k))
        hot = [n for n, _ in m.named_parameters() if not n.startswith("backbone") and "feature_pyramid" not in n]
        flat, opt = a3d.engine.get_optimizer(m, lr=1e-4, active_names=hot)
        crit = a3d.losses.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query",
                                         ground_truth_gaussian_spread=0.01)
        before = flat.flat.clone()
        loss = a3d.engine.train_one_step(m, crit, opt, 0, sample)
        out = keep["out"]
        rel_close("train_one_step loss", loss, sum(r["losses"].values()), 1e-3, 1e-3)
        assert not torch.equal(before, flat.flat), "the optimizer step did not move the parameters"
    for i in range(cfg["levels"]):
        assert torch.equal(out["ghost_pcd_pyramid"][i].transpose(1, 2).cpu(), r["ghost"][i]), f"ghost points level {i}"
    _check_golden_forward(tag, r, cfg, out, inp["pcd"])
    if cfg["train"]:
        _check_golden_grads(r, cfg, m, fmaps)           # flat.grad still holds this step's gradients


@pytest.mark.parametrize("name,B,ncam,levels,Ng,bounds,seed", [
    # BASELINE.json configs[1] token counts: 4 cameras at 256x256, 3 levels, 1000 ghost points (333 / level), S = 4097
    ("cfg2", 2, 4, 3, 333, C.PERACT_BOUNDS, 5),
    # configs[4] shapes: 74-task workspace, 4 levels at 10000 ghost points (2500 / level), 3 cameras, S = 3073
    ("cfg5", 2, 3, 4, 2500, C.HIVEFORMER_BOUNDS, 6),
    # configs[3] (joint keypose + trajectory training, DP batch 128 over 8 GPUs): the keypose half at its PER-GPU shape, 16 keyframes;
    # the trajectory half is tests/test_diffusion_gpu.py::test_cfg4_trajectory_half_per_gpu_shape_vs_oracle
    ("cfg4-keypose", 16, 4, 3, 333, C.PERACT_BOUNDS, 7),
])
def test_act3d_full_shapes_vs_oracle_teacher_forced(a3d, dev, name, B, ncam, levels, Ng, bounds, seed):
    """Full token counts of the training configurations -- HIP vs CPU oracle, per-level teacher forcing."""
    _full_shapes_case(a3d, dev, name, B, ncam, levels, Ng, bounds, seed)


# The opt-in fp8 attention forward (csrc/attention8.hip), which serves gradient-free forwards only (ops.ATTN_MODE).  Its stated
# tolerance grows with the logit range (tests/test_attn8_gpu.py:fp8_tolerance: relative L2 of one attention output =
# 2^-5 (1.5 + L / 8) at |log2-logit| <= L), so this fixture uses gain-1 parameters (the mild logits of a freshly initialised
# model, L ~ 10) where the default-mode test above uses gain 2 (L ~ 50, where e4m3 logits are meaningless: 25 % of the
# mask-logit scale, measured).  The mask logits average the attention outputs' independent errors once more (a ghost
# point's feature is LayerNorm(residual + attention)): bound 2^-6 of each tensor's scale, observed <= 5.1e-3.
FP8_FWD_TOL = 2.0 ** -6


def test_act3d_cfg5_shapes_fp8_attention_mode(a3d, dev):
    """BASELINE.json configs[4]: 4 levels at 10 000 ghost points, fp8 MFMA attention -- the opt-in A3D_ATTN_MODE=fp8, forward
    without gradient, against the fp32 oracle at e4m3's tolerance (the default mode's test above holds the same shapes, with
    gradients, to 1e-3).  The general attention cores must really have run on a3d_attn8_fwd."""
    old, seen, call = a3d.ops.ATTN_MODE, [], a3d.lib.call
    a3d.ops.ATTN_MODE = "fp8"
    a3d.ops.L.call = lambda name, *args: (seen.append(name), call(name, *args))[1]
    try:
        _full_shapes_case(a3d, dev, "cfg5-fp8", 2, 3, 4, 2500, C.HIVEFORMER_BOUNDS, 6, fwd_tol=FP8_FWD_TOL, gain=1.0,
                          forward_only=True)
    finally:
        a3d.ops.ATTN_MODE = old
        a3d.ops.L.call = call
    # 4 levels x 2 ghost-point attention layers (the query stream runs the single-query kernels)
    assert seen.count("a3d_attn8_fwd") == 8 and "a3d_attn16_fwd" not in seen and "a3d_attn_fwd" not in seen, \
        sorted(set(n for n in seen if "attn" in n))


def _full_shapes_case(a3d, dev, name, B, ncam, levels, Ng, bounds, seed, fwd_tol=1e-3, gain=2.0, forward_only=False):
    E = 60
    man = torch.load(os.path.join(HERE, "golden", "act3d_manifest.pt"), weights_only=False)
    cfg = dict(E=E, levels=levels, ncam=ncam, use_instruction=False)
    P = act3d_params(cfg, seed, gain, man["named_parameters"])
    leaf, Po = {}, {}
    for n, t in P.items():
        if id(t) not in leaf:
            leaf[id(t)] = t.clone().requires_grad_()
        Po[n] = leaf[id(t)]
    inp = C.keypose_inputs(seed, B, ncam, E, levels, bounds=bounds)
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    ghost = [torch.from_numpy(OS.ref_sample_ghost_points(bounds, B, Ng, 0))]
    teacher = []
    for i in range(levels):
        teacher.append(inp["action"][:, :3] + torch.from_numpy(rs.normal(0, 0.01, size=(B, 3)).astype(np.float32)))
        if i + 1 < levels:
            ghost.append(torch.from_numpy(OS.ref_sample_ghost_points(bounds, B, Ng, i + 1, inp["action"][:, :3].numpy(),
                                                                      OA.ball_diameters(0.16)[i + 1])))
    # oracle
    f0 = inp["feats"][0].clone().requires_grad_()
    f1 = inp["feats"][1].clone().requires_grad_()
    ofeats = [C.tokens_from_maps(f0)] + [C.tokens_from_maps(f1)] * (levels - 1)
    pcds = [torch.from_numpy(OS.pcd_downsample(inp["pcd"].numpy(), 8 if i == 0 else 2)) for i in range(levels)]
    ocfg = OA.default_cfg(E=E, levels=levels, ncam=ncam, bounds=bounds)
    oout = OA.act3d_forward(Po, ocfg, ofeats, pcds, inp["curr_gripper"], None, gt_action=inp["action"], ghost_points=ghost,
                            teacher_positions=teacher)
    olosses = OA.keypose_loss(oout, inp["action"])
    sum(olosses.values()).backward()
    # device
    m = build_model(a3d, dev, cfg, P, Ng, True, bounds=bounds)
    d0 = inp["feats"][0].to(dev).requires_grad_()
    d1 = inp["feats"][1].to(dev).requires_grad_()
    t1 = C.tokens_from_maps(d1)
    dfeats = [C.tokens_from_maps(d0)] + [t1] * (levels - 1)
    with torch.set_grad_enabled(not forward_only):
        out = m(None, inp["pcd"].to(dev), None, inp["curr_gripper"].to(dev), gt_action=inp["action"].to(dev),
                ghost_points=[g.to(dev) for g in ghost], teacher_positions=[t.to(dev) for t in teacher], visual_features=dfeats)
    for i in range(levels):
        if i > 0:
            assert torch.equal(out["topk_indices_pyramid"][i].cpu(), oout["topk_indices"][i]), f"top-k indices level {i}"
        for l in range(2):
            scale_close(f"{name} mask L{i} layer{l}", out["ghost_pcd_masks_pyramid"][i][l], oout["ghost_pcd_masks_pyramid"][i][l],
                        tol=fwd_tol)
        o_top = oout["ghost_pcd_masks_pyramid"][i][-1].max(-1).indices
        gap = oout["ghost_pcd_masks_pyramid"][i][-1].topk(2, -1).values
        safe = (gap[:, 0] - gap[:, 1]) > 2 * fwd_tol * max(1.0, oout["ghost_pcd_masks_pyramid"][i][-1].abs().max().item())
        d_top = out["ghost_pcd_masks_pyramid"][i][-1].max(-1).indices.cpu()
        assert torch.equal(d_top[safe], o_top[safe]), f"argmax level {i}"
    rel_close(f"{name} rotation", out["rotation"], oout["rotation"], fwd_tol, 0)
    crit = a3d.losses.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query",
                                     ground_truth_gaussian_spread=0.01)
    losses = crit.compute_loss(out, {"action": inp["action"].to(dev), "task": ["t"] * B})
    for k, v in olosses.items():
        rel_close(f"{name} loss " + k, losses[k], v, fwd_tol, fwd_tol)
    if forward_only:
        return
    sum(losses.values()).backward()
    named = dict(m.named_parameters())
    bad = []
    for n, p in Po.items():
        if n in named and p.grad is not None and not any(n.startswith(pre + f".{i}.") for pre in (
                "ghost_points_embed_pyramid", "ghost_point_cross_attn_pyramid", "query_cross_attn_pyramid") for i in (1, 2, 3)):
            g = named[n].grad
            ref = p.grad
            denom = ref.abs().max().item() + 1e-6
            err = (g.cpu() - ref).abs().max().item()
            l2 = ((g.cpu() - ref).norm() / (ref.norm() + 1e-12)).item()
            print(f"[parity] {name} grad {n}: max_abs_err={err:.3e} ref_absmax={denom:.3e} of_scale={err / denom:.2e} rel_l2={l2:.2e}")
            if err > GRAD_TOL * denom + 1e-4:
                bad.append(f"{n}: err {err:.3e} vs absmax {denom:.3e} ({err / denom:.2e} of scale)")
    assert not bad, "gradients outside %g of their scale:\n  %s" % (GRAD_TOL, "\n  ".join(bad))
    scale_close(f"{name} d feat level0", d0.grad, f0.grad, GRAD_TOL, floor=0.0)
    scale_close(f"{name} d feat fine", d1.grad, f1.grad, GRAD_TOL, floor=0.0)


def test_bf16_token_maps_gathered_in_place_equal_the_fp32_copy(a3d, dev):
    """The bf16 training path (bench.py: fpn_dtype = bf16) hands the FPN's channels-last bf16 map to the hot path as is.
    Feeding the same bf16 values as an fp32 copy must give the identical forward, and the bf16 gradient map (shared by
    the two fine levels, accumulated in place) must equal the rounded fp32 one."""
    r, cfg, names = _act3d_case("train_L3_C1_N64")
    P = act3d_params(cfg, r["seed"], r["gain"], names)
    inp, _, _ = _golden_inputs(r, cfg, dev)
    crit = a3d.losses.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    sample = {"action": inp["action"].to(dev), "task": ["t"] * cfg["B"]}
    res = {}
    for tag, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32), ("bf16pad", torch.bfloat16)):
        m = build_model(a3d, dev, cfg, P, cfg["Ng"], True)
        maps = [f.to(dev).to(torch.bfloat16).to(dt).requires_grad_() for f in inp["feats"][:2]]
        toks = [C.tokens_from_maps(f) for f in maps]
        if tag == "bf16pad":       # rows of 64 channels, the hot path reads the first 60 (channel-padded FPN, nn.py)
            toks = [torch.nn.functional.pad(t, (0, 4)).detach().requires_grad_() for t in toks]
            maps = toks
        feats = [toks[0]] + [toks[1]] * (cfg["levels"] - 1)
        out = m(None, inp["pcd"].to(dev), inp["instr"].to(dev), inp["curr_gripper"].to(dev), gt_action=inp["action"].to(dev),
                ghost_points=[g.to(dev) for g in r["ghost"]], visual_features=feats)
        loss = sum(crit.compute_loss(out, sample).values())
        loss.backward()
        res[tag] = (out, loss, maps, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    ob, lb, mb, gb = res["bf16"]
    of, lf, mf, gf = res["fp32"]
    op, lp, mp_, gp = res["bf16pad"]
    assert torch.equal(lb, lf) and torch.equal(lp, lf)
    for a, b in zip(mp_, mb):                    # padded rows: same gradient in the 60 real channels, pad channels untouched
        assert torch.equal(a.grad[..., :60], C.tokens_from_maps(b.grad)) and (a.grad[..., 60:] == 0).all()
    for i in range(cfg["levels"]):
        assert torch.equal(ob["ghost_pcd_masks_pyramid"][i][-1], of["ghost_pcd_masks_pyramid"][i][-1])
    gmax = max(g_.abs().max().item() for g_ in gf.values())
    for n in gf:      # same arithmetic; the small-M weight gradients accumulate with float atomics (order noise only, also
        #               on tensors whose gradient is mathematically zero -- hence the scale of ALL gradients in the bound)
        assert (gb[n] - gf[n]).abs().max().item() <= 1e-5 * max(1e-3 * gmax, gf[n].abs().max().item()), n
    for a, b in zip(mb, mf):
        assert a.grad.dtype == torch.bfloat16
        ref = b.grad
        err = (a.grad.float() - ref).abs().max().item()
        print(f"[parity] bf16 token-map gradient vs fp32: max abs err {err:.3e} (scale {ref.abs().max().item():.3e})")
        assert err <= 2 ** -7 * ref.abs().max().item(), err       # two bf16 roundings (one per fine level) at most
        same = ((a.grad == 0) == (ref == 0)).float().mean().item()
        assert same > 0.9999, same                                 # same sparsity: only gathered rows receive a gradient


def test_context_gradient_sink_equals_autograd_sum(a3d, dev):
    """ops.GradSink: the four consumers of a level's context tokens (two ghost-attention layers, two query-stream layers) sum its
    gradient in ONE buffer inside their kernels (first writes, the others += , a gate node hands the total to autograd) instead of
    returning four tensors for autograd to add.  Same model, same inputs, A3D_CTX_SINK on / off: every parameter gradient and the
    token-map gradients agree to fp32 re-association noise, and a second pass gives the same result (the sinks drain)."""
    r, cfg, names = _act3d_case("train_L3_C1_N64")
    P = act3d_params(cfg, r["seed"], r["gain"], names)
    inp, _, _ = _golden_inputs(r, cfg, dev)
    crit = a3d.losses.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    sample = {"action": inp["action"].to(dev), "task": ["t"] * cfg["B"]}
    keep = a3d.ops.CTX_GRAD_SINK
    res = {}
    try:
        for tag, flag in (("sink", True), ("plain", False), ("sink2", True)):
            a3d.ops.CTX_GRAD_SINK = flag
            m = build_model(a3d, dev, cfg, P, cfg["Ng"], True)
            maps = [f.to(dev).float().requires_grad_() for f in inp["feats"][:2]]
            toks = [C.tokens_from_maps(f) for f in maps]
            feats = [toks[0]] + [toks[1]] * (cfg["levels"] - 1)
            out = m(None, inp["pcd"].to(dev), inp["instr"].to(dev), inp["curr_gripper"].to(dev), gt_action=inp["action"].to(dev),
                    ghost_points=[g.to(dev) for g in r["ghost"]], visual_features=feats)
            loss = sum(crit.compute_loss(out, sample).values())
            loss.backward()
            if flag:
                assert all(sk.buf is None and sk.writers == 0 for sk in a3d.ops.GradSink.live) and len(a3d.ops.GradSink.live) == cfg["levels"]
            res[tag] = (loss.detach(), [f.grad.clone() for f in maps], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    finally:
        a3d.ops.CTX_GRAD_SINK = keep
    ls, ms, gs = res["sink"]
    lp, mp_, gp = res["plain"]
    assert torch.equal(ls, lp) and set(gs) == set(gp)
    gmax = max(g_.abs().max().item() for g_ in gp.values())
    worst = 0.0
    for n in gp:
        err = (gs[n] - gp[n]).abs().max().item()
        worst = max(worst, err / max(1e-3 * gmax, gp[n].abs().max().item()))
        assert err <= 1e-5 * max(1e-3 * gmax, gp[n].abs().max().item()), n
    for a, b in zip(ms, mp_):
        assert (a - b).abs().max().item() <= 1e-5 * max(b.abs().max().item(), 1e-12)
    print(f"[parity] context gradient sink vs autograd sum: worst relative parameter-gradient difference {worst:.3e}")
    for n in gs:                                   # the second pass with sinks reproduces the first
        assert (res["sink2"][2][n] - gs[n]).abs().max().item() <= 1e-5 * max(1e-3 * gmax, gs[n].abs().max().item()), n


def test_hot_path_forward_is_run_to_run_deterministic(a3d, dev):
    """Same visual tokens + same sampler state -> bit-identical free-running forward (ghost points, k-NN sets, mask logits,
    argmax cascade, action): no forward kernel depends on atomics or launch timing.  (The convolutions in front of the hot
    path are MIOpen's and may change algorithm between the first and later calls, which is why evaluation tests record the
    forwards instead of repeating them.)"""
    torch.manual_seed(0)
    m = a3d.Act3D(image_size=(128, 128), gripper_loc_bounds=C.PERACT_BOUNDS, num_ghost_points=300, num_ghost_points_val=600,
                  num_sampling_level=3, sampler_seed=5).to(dev).eval()
    inp = C.keypose_inputs(61, 3, 2, 60, 3, image=128)
    feats = [C.tokens_from_maps(f.to(dev)) for f in (inp["feats"][0], inp["feats"][1], inp["feats"][1])]
    outs = []
    with torch.no_grad():
        for _ in range(3):
            m._rng_state.copy_(torch.tensor([5, 0]))
            outs.append(m(None, inp["pcd"].to(dev), inp["instr"].to(dev), inp["curr_gripper"].to(dev), gt_action=None,
                          visual_features=feats))
    for o in outs[1:]:
        for i in range(3):
            assert torch.equal(o["ghost_pcd_pyramid"][i], outs[0]["ghost_pcd_pyramid"][i]), f"ghost points level {i}"
            assert torch.equal(o["ghost_pcd_masks_pyramid"][i][-1], outs[0]["ghost_pcd_masks_pyramid"][i][-1]), f"mask level {i}"
            assert torch.equal(o["position_pyramid"][i], outs[0]["position_pyramid"][i])
            if i > 0:
                assert torch.equal(o["topk_indices_pyramid"][i], outs[0]["topk_indices_pyramid"][i])
        assert torch.equal(o["rotation"], outs[0]["rotation"]) and torch.equal(o["gripper"], outs[0]["gripper"])


def test_bf16_fpn_deferred_output_bias_width_120(a3d, dev):
    """E = 120 / 8 heads with the bf16 FPN: the 3x3 output convolutions run bias-free and the bias is owed to the gathered rows
    (ops.TokenMap.row_bias); its gradient is a column sum over the gathered rows (a3d_colsum_rows, any width).  Same step with the
    bias materialised on the map (TokenMap.with_bias(), autograd sums the rows): same loss, same bias gradients."""
    torch.manual_seed(0)
    B, ncam, E, levels = 2, 1, 120, 2
    m = a3d.Act3D(embedding_dim=E, num_attn_heads=8, gripper_loc_bounds=C.PERACT_BOUNDS, num_ghost_points=64 * levels,
                  num_ghost_points_val=64 * levels, num_sampling_level=levels, sampler_seed=7).to(dev).train()
    m.backbone_dtype = m.fpn_dtype = torch.bfloat16
    inp = C.keypose_inputs(17, B, ncam, E, levels)
    rgb = torch.rand((B, ncam, 3, 256, 256), generator=torch.Generator().manual_seed(3)).to(dev)
    crit = a3d.losses.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query", ground_truth_gaussian_spread=0.01)
    sample = {"action": inp["action"].to(dev), "task": ["t"] * B}
    teacher = [inp["action"][:, :3].to(dev).contiguous()] * levels
    biases = {n: p for n, p in m.named_parameters() if "feature_pyramid.layer_blocks" in n and n.endswith("bias")}
    res = {}
    # ONE pass through the backbone / FPN (MIOpen may pick another convolution algorithm on a second call, and the untrained
    # model turns 1e-2 bf16 feature noise into a visibly different loss); the two runs differ only in where the bias is added
    toks = [t.detach() for t in m.compute_visual_tokens(rgb)]
    assert all(isinstance(t, a3d.ops.TokenMap) and t.row_bias is not None and t.tokens.dtype == torch.bfloat16 for t in toks)
    for tag in ("deferred", "materialised"):
        m.zero_grad(set_to_none=True)
        m._rng_state.copy_(torch.tensor([7, 0]))
        feats = toks if tag == "deferred" else [t.with_bias() for t in toks]
        out = m(None, inp["pcd"].to(dev), inp["instr"].to(dev), inp["curr_gripper"].to(dev), gt_action=inp["action"].to(dev),
                visual_features=feats, teacher_positions=teacher)
        loss = sum(crit.compute_loss(out, sample).values())
        loss.backward()
        res[tag] = (loss.detach().clone(), {n: p.grad.clone() for n, p in biases.items() if p.grad is not None})
    (la, ga), (lb, gb) = res["deferred"], res["materialised"]
    assert abs(la.item() - lb.item()) <= 1e-5 * max(1.0, abs(lb.item())), (la.item(), lb.item())
    used = [n for n in gb if gb[n].abs().max().item() > 0]
    assert used and set(used) <= set(ga), (sorted(ga), sorted(gb))
    for n in used:
        err, sc = (ga[n] - gb[n]).abs().max().item(), gb[n].abs().max().item()
        print(f"[parity] deferred FPN output bias gradient {n}: err {err:.3e} of scale {sc:.3e}")
        assert torch.isfinite(ga[n]).all() and err <= 1e-3 * sc, (n, err, sc)
