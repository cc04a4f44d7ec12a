"""Generates tests/golden/*.pt by running the REFERENCE (/root/reference, imported with stubs) on seeded inputs.

Run in the build container only:   python tests/golden/make_goldens.py
The fixtures hold seeds + the reference's outputs (small tensors); inputs/parameters are regenerated from the seeds
by tests/golden/common.py.  Nothing of the reference's source is stored.
"""
import os
import sys
from contextlib import contextmanager

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import common as C  # noqa: E402
from refimport import import_reference  # noqa: E402

torch.set_num_threads(8)
R = import_reference()


def save(name, obj):
    path = os.path.join(HERE, name)
    torch.save(obj, path)
    print("wrote", name, "%.1f KB" % (os.path.getsize(path) / 1024))


# ------------------------------------------------------------------------------------------------------ G1-G3: blocks
def golden_blocks():
    out = {}
    rs = np.random.RandomState(7)
    # G1: RoPE-3D code, rotary application, sinusoidal embedding
    for E in (60, 120):
        xyz = C.rs_tensor(rs, (2, 9, 3), scale=1.5)
        code = R.pe.RotaryPositionEncoding3D(E)(xyz)
        x = C.rs_tensor(rs, (2, 9, E))
        rot = R.pe.RotaryPositionEncoding.embed_rotary(x, code[..., 0], code[..., 1])
        out[f"rope_{E}"] = dict(xyz=xyz, code=code, x=x, rotated=rot)
    t = torch.tensor([0.0, 1.0, 17.0, 99.0])
    out["sinusoidal_120"] = dict(t=t, emb=R.pe.SinusoidalPosEmb(120)(t))
    # G2: MultiheadCustomAttention, the three projection paths, with / without RoPE and padding mask, fwd + grads
    for tag, (Lq, S, E, H, rope, masked, mode) in {
        "cross_rope": (37, 131, 60, 4, True, False, "kv"),
        "self_mask": (16, 16, 120, 8, True, True, "qk"),
        "cross_plain": (5, 53, 120, 8, False, False, "kv"),
    }.items():
        B = 2
        m = R.mha.MultiheadCustomAttention(E, H)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = C.seeded_state_dict(shapes, seed=11 + E + Lq, gain=2.0)
        m.load_state_dict(sd)
        q = C.rs_tensor(rs, (B, Lq, E)).requires_grad_()
        k = q if mode == "qk" else C.rs_tensor(rs, (B, S, E)).requires_grad_()
        v = k if mode == "kv" else C.rs_tensor(rs, (B, S, E)).requires_grad_()
        q_xyz = C.rs_tensor(rs, (B, Lq, 3)) if rope else None
        k_xyz = (q_xyz if mode == "qk" else C.rs_tensor(rs, (B, S, 3))) if rope else None
        kmask = None
        if masked:
            kmask = torch.zeros(B, S, dtype=torch.bool)
            kmask[1, -5:] = True
        pe = R.pe.RotaryPositionEncoding3D(E)
        kw = {}
        if rope:
            kw["rotary_pe"] = (pe(q_xyz), pe(k_xyz))
        if mode == "qk":
            vv = v
            o, w = m(query=q.transpose(0, 1), key=q.transpose(0, 1), value=vv.transpose(0, 1), key_padding_mask=kmask, **kw)
        else:
            o, w = m(query=q.transpose(0, 1), key=k.transpose(0, 1), value=v.transpose(0, 1), key_padding_mask=kmask, **kw)
        o = o.transpose(0, 1)
        dy = C.rs_tensor(rs, tuple(o.shape))
        o.backward(dy)
        out["mha_" + tag] = dict(cfg=(B, Lq, S, E, H, rope, masked, mode), seed=11 + E + Lq,
                                 q=q.detach(), k=k.detach(), v=v.detach(), q_xyz=q_xyz, k_xyz=k_xyz, kmask=kmask, dy=dy,
                                 out=o.detach(), weights_mean=w.detach().mean(1),
                                 dq=q.grad.clone(), dk=None if mode == "qk" else k.grad.clone(),
                                 dv=None if mode == "kv" else v.grad.clone(),
                                 d_in_w=m.in_proj_weight.grad.clone(), d_in_b=m.in_proj_bias.grad.clone(),
                                 d_out_w=m.out_proj.weight.grad.clone())
    # G3: RelativeCrossAttentionModule (list outputs) and ParallelAttentionLayer with NON-zero AdaLN, eval mode
    E, H, B, Lq, S = 60, 4, 2, 21, 77
    mod = R.layers.RelativeCrossAttentionModule(E, H, 2)
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict(C.seeded_state_dict(shapes, seed=31, gain=2.0))
    q, v = C.rs_tensor(rs, (B, Lq, E)), C.rs_tensor(rs, (B, S, E))
    q_xyz, v_xyz = C.rs_tensor(rs, (B, Lq, 3)), C.rs_tensor(rs, (B, S, 3))
    pe = R.pe.RotaryPositionEncoding3D(E)
    outs = mod(query=q.transpose(0, 1), value=v.transpose(0, 1), query_pos=pe(q_xyz), value_pos=pe(v_xyz))
    out["rel_cross_attn_module"] = dict(seed=31, q=q, v=v, q_xyz=q_xyz, v_xyz=v_xyz,
                                        outs=[o.detach().transpose(0, 1).contiguous() for o in outs])
    E, H, B, Ln, S = 120, 8, 2, 16, 70
    lay = R.layers.ParallelAttentionLayer(d_model=E, n_heads=H, self_attention1=True, self_attention2=False,
                                          cross_attention1=True, cross_attention2=False, rotary_pe=True, use_adaln=True)
    lay.eval()
    shapes = {k: tuple(v.shape) for k, v in lay.state_dict().items()}
    lay.load_state_dict(C.seeded_state_dict(shapes, seed=41, gain=1.5))
    s1, s2 = C.rs_tensor(rs, (B, Ln, E)), C.rs_tensor(rs, (B, S, E))
    x1, x2 = C.rs_tensor(rs, (B, Ln, 3)), C.rs_tensor(rs, (B, S, 3))
    sem = R.pe.SinusoidalPosEmb(E)(torch.arange(Ln))[None].repeat(B, 1, 1)
    ada = C.rs_tensor(rs, (B, E))
    mask = torch.zeros(B, Ln, dtype=torch.bool)
    mask[1, -4:] = True
    pe = R.pe.RotaryPositionEncoding3D(E)
    with torch.no_grad():
        y, _ = lay(seq1=s1, seq1_key_padding_mask=mask, seq2=s2, seq2_key_padding_mask=None, seq1_pos=pe(x1),
                   seq2_pos=pe(x2), seq1_sem_pos=sem, seq2_sem_pos=None, ada_sgnl=ada)
    out["parallel_attention_layer"] = dict(seed=41, s1=s1, s2=s2, x1=x1, x2=x2, ada=ada, mask=mask, out=y)
    # two files, each under the size limit for a committed file (tests/test_oracle_golden.py merges them)
    save("blocks_mha.pt", {k: out.pop(k) for k in ("mha_self_mask", "mha_cross_plain")})
    save("blocks.pt", out)


# ------------------------------------------------------------------------------------------------------ G4/G5: sampling
def golden_sampling():
    out = {}
    np.random.seed(123)
    b = C.PERACT_BOUNDS
    out["cube"] = dict(seed=123, pts=R.utils.sample_ghost_points_uniform_cube(b, 50))
    c = np.array([0.2, 0.0, 1.0])
    bb = np.stack([np.clip(c - 0.08, b[0], b[1]), np.clip(c + 0.08, b[0], b[1])])
    out["sphere"] = dict(center=c, radius=0.08, bounds=bb, pts=R.utils.sample_ghost_points_uniform_sphere(c, 0.08, bb, 50))
    c2 = np.array([0.64, 0.5, 1.5])        # near the workspace corner: clipped box
    bb2 = np.stack([np.clip(c2 - 0.02, b[0], b[1]), np.clip(c2 + 0.02, b[0], b[1])])
    out["sphere_clipped"] = dict(center=c2, radius=0.02, bounds=bb2,
                                 pts=R.utils.sample_ghost_points_uniform_sphere(c2, 0.02, bb2, 40))
    rs = np.random.RandomState(5)
    for f, H in ((2, 256), (8, 256), (4, 128), (2, 128)):
        pcd = C.rs_tensor(rs, (1, 2, 3, H, H), kind="uniform")
        ref = F.interpolate(pcd.view(2, 3, H, H), scale_factor=1.0 / f, mode="bilinear")
        h = H // f
        out[f"interp_{f}_{H}"] = dict(seed=5, sum=ref.double().sum().item(),
                                      sample=ref.view(1, 2, 3, h, h).permute(0, 1, 3, 4, 2).reshape(1, 2 * h * h, 3)[:, ::97].clone())
    save("sampling.pt", out)


# ------------------------------------------------------------------------------------------------------ G6/G7: Act3D
def build_ref_act3d(E, levels, ncam, Ng, use_instruction, seed, gain, image=256, Ng_val=None, model_kw=None):
    m = R.act3d.Act3D(backbone="clip", image_size=(image, image), embedding_dim=E, num_attn_heads=4,
                      gripper_loc_bounds=C.PERACT_BOUNDS, num_ghost_points=Ng * levels,
                      num_ghost_points_val=(Ng * 2 if Ng_val is None else Ng_val) * levels, num_sampling_level=levels,
                      weight_tying=True, gp_emb_tying=True, use_instruction=use_instruction, **(model_kw or {}))
    if image == 128:
        # the reference's constructor names the attribute `coarse_feature_map` for 128x128 images but forward reads
        # `feature_map_pyramid` (act3d.py:81 vs :378); patch the instance as SURVEY App. B-5 does
        m.feature_map_pyramid = m.coarse_feature_map
    shapes, alias = C.unique_param_shapes(m)
    sd = C.expand_aliases(C.seeded_state_dict(shapes, seed, gain), alias)
    missing = m.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    return m, sd


def inject_features(m, inp, ncam):
    """Replaces backbone+FPN by the seeded feature maps; everything downstream is the reference's own code."""
    def fake(visible_rgb, visible_pcd, num_cameras):
        import einops
        pcd = einops.rearrange(visible_pcd, "bt ncam c h w -> (bt ncam) c h w")
        feats, poss, pcds = [], [], []
        for i in range(m.num_sampling_level):
            p = F.interpolate(pcd, scale_factor=1. / m.downscaling_factor_pyramid[i], mode='bilinear')
            p = einops.rearrange(p, "(bt ncam) c h w -> bt (ncam h w) c", ncam=num_cameras)
            feats.append(inp["feats"][i])
            poss.append(m.relative_pe_layer(p))
            pcds.append(p)
        return feats, poss, pcds
    m._compute_visual_features = fake


def run_act3d_case(tag, E, levels, ncam, Ng, use_instruction, B, train, min_gap=1e-2, image=256, Ng_val=None,
                   model_kw=None, loss_kw=None, probe=False):
    """model_kw: non-default Act3D constructor options; loss_kw: LossAndMetrics options; probe=True replaces the loss by a
    fixed linear functional of (rotation, gripper, position) -- used for the 6D heads, for which the reference has no loss."""
    for attempt in range(80):
        seed, gain = 100 + attempt, 3.0
        m, sd = build_ref_act3d(E, levels, ncam, Ng, use_instruction, seed, gain, image=image, Ng_val=Ng_val,
                                model_kw=model_kw)
        inp = C.keypose_inputs(seed, B, ncam, E, levels, image=image)
        for f in inp["feats"]:
            f.requires_grad_(train)
        inject_features(m, inp, ncam)
        m.train(train)
        np.random.seed(seed)
        rgb = torch.zeros(B, ncam, 3, image, image)
        out = m(rgb, inp["pcd"], inp["instr"], inp["curr_gripper"], gt_action=inp["action"] if train else None)
        gaps = []
        for masks in out["ghost_pcd_masks_pyramid"]:
            top2 = masks[-1].topk(2, dim=-1).values
            gaps.append((top2[:, 0] - top2[:, 1]).min().item())
        if min(gaps) > min_gap:
            break
    else:
        raise RuntimeError("no seed with a safe top-2 logit gap")
    print(tag, "seed", seed, "min top-2 gaps per level", gaps)
    rec = dict(cfg=dict(E=E, levels=levels, ncam=ncam, Ng=out["ghost_pcd_pyramid"][0].shape[-1],
                        use_instruction=use_instruction, B=B, train=train, image=image),
               seed=seed, gain=gain, gaps=gaps,
               ghost=[g.detach().transpose(1, 2).contiguous() for g in out["ghost_pcd_pyramid"]],
               masks=[[mm.detach() for mm in ms] for ms in out["ghost_pcd_masks_pyramid"]],
               positions=[p.detach()[:, 0] for p in out["position_pyramid"]],
               position=out["position"].detach(), rotation=out["rotation"].detach(), gripper=out["gripper"].detach(),
               query_features=out["query_features"].detach()[0], model_kw=dict(model_kw or {}), loss_kw=dict(loss_kw or {}))
    if model_kw:
        rec["param_shapes"] = C.unique_param_shapes(m)[0]
    if out["fine_ghost_pcd_offsets"] is not None:
        rec["offsets"] = out["fine_ghost_pcd_offsets"].detach()
    idxs = [None]
    for i in range(1, levels):
        l2 = ((out["position_pyramid"][i - 1] - out["visible_pcd_pyramid"][i]) ** 2).sum(-1).sqrt()
        tk = l2.topk(k=32 * 32 * ncam, dim=-1, largest=False)
        idxs.append(tk.indices)
        rec.setdefault("topk_values", [None]).append(tk.values)
    rec["topk"] = idxs
    if train:
        lk = dict(position_loss="ce", rotation_parametrization=(model_kw or {}).get("rotation_parametrization", "quat_from_query"),
                  ground_truth_gaussian_spread=0.01)
        lk.update(loss_kw or {})
        crit = R.main_keypose.LossAndMetrics(**lk)
        sample = {"action": inp["action"], "task": ["t"] * B}
        if probe:
            g = torch.Generator().manual_seed(seed)
            rec["probe"] = dict(rotation=torch.randn(out["rotation"].shape, generator=g),
                                gripper=torch.randn(out["gripper"].shape, generator=g),
                                position=torch.randn(out["position"].shape, generator=g))
            losses = {k: (out[k] * w).sum() for k, w in rec["probe"].items()}
        else:
            losses = crit.compute_loss(out, sample)
        total = sum(losses.values())
        total.backward()
        rec["losses"] = {k: v.detach() for k, v in losses.items()}
        grads = {n: p.grad.clone() for n, p in m.named_parameters()
                 if p.grad is not None and not n.startswith("backbone") and "feature_pyramid" not in n}
        rec["grad_norms"] = {n: g.norm().item() for n, g in grads.items()}
        keep = ["query_embed.weight", "curr_gripper_embed.weight", "ghost_points_embed_pyramid.0.weight",
                "ghost_point_cross_attn_pyramid.0.attn_layers.0.multihead_attn.in_proj_weight",
                "query_cross_attn_pyramid.0.attn_layers.1.multihead_attn.out_proj.weight",
                "ghost_point_cross_attn_pyramid.0.ffw_layers.1.linear1.weight", "gripper_state_predictor.2.weight",
                "gripper_state_predictor.0.weight", "ghost_point_offset_predictor.0.weight", "ghost_point_offset_predictor.2.bias",
                "instr_position_embedding.weight", "instr_position_norm.weight", "instruction_encoder.weight"]
        rec["grads"] = {n: grads[n] for n in keep if n in grads}
        rec["feat_grad_norms"] = [None if f.grad is None else f.grad.norm().item() for f in inp["feats"][:2]]
        if levels == 1:
            rec["feat0_grad_sample"] = C.tokens_from_maps(inp["feats"][0].grad)[:, ::37].clone()
        fg = inp["feats"][1].grad if levels > 1 else None
        if fg is not None:
            rec["feat1_grad_sample"] = C.tokens_from_maps(fg)[:, ::517].clone()
        if not probe:
            rec["metrics"] = {k: v.detach() for k, v in crit.compute_metrics(out, sample).items()
                              if k.startswith("mean") or k == "gripper"}
    return rec


def golden_act3d():
    out = {
        "train_L3_C1_N64": run_act3d_case("train_L3_C1_N64", 60, 3, 1, 64, False, 2, True),
        "eval_L3_C1_N128": run_act3d_case("eval_L3_C1_N128", 60, 3, 1, 64, False, 2, False),
        "train_L2_C2_N64_instr": run_act3d_case("train_L2_C2_N64_instr", 60, 2, 2, 64, True, 2, True),
        "train_L4_C1_N32": run_act3d_case("train_L4_C1_N32", 60, 4, 1, 32, False, 1, True),      # default min_gap = 1e-2 (seed 175)
    }
    save("act3d.pt", out)
    # G12: parameter manifest of the default configuration
    m, _ = build_ref_act3d(60, 3, 1, 333, False, 1, 1.0)
    man = {n: tuple(p.shape) for n, p in m.named_parameters() if not n.startswith("backbone")}
    m2, _ = build_ref_act3d(60, 3, 1, 333, True, 1, 1.0)
    man2 = {n: tuple(p.shape) for n, p in m2.named_parameters() if not n.startswith("backbone")}
    sdk = [k for k in m.state_dict().keys() if not k.startswith("backbone")]
    save("act3d_manifest.pt", dict(named_parameters=man, named_parameters_instr=man2, state_dict_keys=sdk,
                                   n_trainable=sum(int(np.prod(s)) for s in man.values()),
                                   n_trainable_instr=sum(int(np.prod(s)) for s in man2.values())))


def golden_act3d_options():
    """The non-default Act3D options of act3d.py:30-39 (regress_position_offset, *_from_top_ghost, 6D_*, ins_pos_emb)."""
    out = {
        "offset_topghost_inspos": run_act3d_case(
            "offset_topghost_inspos", 60, 2, 1, 64, True, 2, True,
            model_kw=dict(regress_position_offset=True, rotation_parametrization="quat_from_top_ghost", ins_pos_emb=True),
            loss_kw=dict(position_loss="ce+mse")),
        "sixd_query": run_act3d_case("sixd_query", 60, 2, 1, 64, False, 2, True,
                                     model_kw=dict(rotation_parametrization="6D_from_query"), probe=True),
        "sixd_topghost_offset_eval": run_act3d_case(
            "sixd_topghost_offset_eval", 60, 2, 1, 64, False, 2, False,
            model_kw=dict(rotation_parametrization="6D_from_top_ghost", regress_position_offset=True)),
    }
    save("act3d_options.pt", out)


def golden_act3d_cfg1():
    """BASELINE.json configs[0]: single-task keypose, batch 1, one 128x128 camera, ONE ghost-point level
    (num_ghost_points 1000 in training, 10000 at evaluation).  Free-running (numpy-seeded ghost points)."""
    out = {
        "train_128_L1_C1_N1000": run_act3d_case("train_128_L1_C1_N1000", 60, 1, 1, 1000, False, 1, True, min_gap=2e-3,
                                                image=128, Ng_val=10000),
        "eval_128_L1_C1_N10000": run_act3d_case("eval_128_L1_C1_N10000", 60, 1, 1, 1000, False, 1, False, min_gap=2e-3,
                                                image=128, Ng_val=10000),
    }
    save("act3d_cfg1.pt", out)


# ------------------------------------------------------------------------------------------------------ G8/G9/G10: diffusion
@contextmanager
def patched_rng(randn_list, randint_value):
    orig_randn, orig_randint = torch.randn, torch.randint
    it = iter(randn_list)

    def fake_randn(*a, **k):
        return next(it).clone()

    def fake_randint(*a, **k):
        return randint_value.clone()

    torch.randn, torch.randint = fake_randn, fake_randint
    try:
        yield
    finally:
        torch.randn, torch.randint = orig_randn, orig_randint


def golden_diffusion():
    E, B, Ln, ncam = 120, 2, 8, 1
    m = R.dm.DiffusionPlanner(backbone="clip", image_size=(256, 256), embedding_dim=E, output_dim=7,
                              num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6, use_instruction=True,
                              use_goal=True, use_goal_at_test=True, feat_scales_to_use=1, attn_rounds=1,
                              weight_tying=True, gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D",
                              diffusion_timesteps=100)
    shapes, alias = C.unique_param_shapes(m)
    seed = 77
    sd = C.expand_aliases(C.seeded_state_dict(shapes, seed, gain=1.5), alias)
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    m.eval()                                   # dropout off (SURVEY §7 hard parts)
    inp = C.trajectory_inputs(seed, B, Ln, ncam, E, pad_last=2)
    head = m.prediction_head

    def fake_encode_images(rgb, pcd):
        import einops
        p = einops.rearrange(pcd, "bt ncam c h w -> (bt ncam) c h w")
        p = F.interpolate(p, scale_factor=1. / 8, mode='bilinear')
        p = einops.rearrange(p, "(bt ncam) c h w -> bt (ncam h w) c", ncam=ncam)
        return [inp["fmap"]], [p]
    head.encode_images = fake_encode_images
    rgb = torch.zeros(B, ncam, 3, 256, 256)
    rec = dict(cfg=dict(E=E, B=B, L=Ln, ncam=ncam, pad_last=2), seed=seed, gain=1.5)
    # G8: training loss with injected noise / timesteps (+ gradients)
    with patched_rng([inp["noise"]], inp["timesteps"]):
        loss = m(inp["trajectory"], inp["mask"], rgb, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"])
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None and "feature_pyramid" not in n}
    rec["train_loss"] = loss.detach()
    rec["grad_norms"] = {n: g.norm().item() for n, g in grads.items()}
    keep = ["prediction_head.traj_encoder.0.weight", "prediction_head.traj_attention.0.layers.0.adaln_12.modulation.1.weight",
            "prediction_head.traj_attention.0.layers.3.sa1.in_proj_weight", "prediction_head.pos_regressor.0.3.weight",
            "prediction_head.vl_attention.0.layers.1.cross_12.in_proj_weight", "prediction_head.goal_gripper_embed.weight"]
    rec["grads"] = {n: grads[n].clone() for n in keep}
    # head forward on a fixed noisy trajectory (eval)
    with torch.no_grad():
        tr9 = m.convert_rot(torch.cat([m.normalize_pos(inp["trajectory"][..., :3]), inp["trajectory"][..., 3:]], -1))
        pcdn = torch.permute(m.normalize_pos(torch.permute(inp["pcd"], [0, 1, 3, 4, 2])), [0, 1, 4, 2, 3])
        cg = inp["curr_gripper"].clone(); cg[:, :3] = m.normalize_pos(cg[:, :3]); cg = m.convert_rot(cg)
        gg = inp["goal_gripper"].clone(); gg[:, :3] = m.normalize_pos(gg[:, :3]); gg = m.convert_rot(gg)
        pred = head(tr9, inp["mask"], inp["timesteps"], rgb, pcdn, cg, gg, inp["instr"])[-1]
    rec["head_in"] = tr9
    rec["head_out"] = pred
    rec["conv"] = dict(curr9=cg, goal9=gg)
    # G9: the full 100-step sampling loop with injected noise
    sn = inp["step_noise"]
    m.position_noise_scheduler.injected_noise = {t: sn[t][..., :3] for t in range(100)}
    m.rotation_noise_scheduler.injected_noise = {t: sn[t][..., 3:] for t in range(100)}
    trace = {}
    orig = m.policy_forward_pass

    def spy(trajectory, timestep, fixed_inputs):
        t = int(timestep[0])
        if t in (99, 98, 60, 1, 0):
            trace[t] = trajectory.detach().clone()
        return orig(trajectory, timestep, fixed_inputs)
    m.policy_forward_pass = spy
    with torch.no_grad(), patched_rng([inp["init_noise"]], inp["timesteps"]):
        final = m(inp["trajectory"], inp["mask"], rgb, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"],
                  run_inference=True)
    rec["sample_trace_inputs"] = trace
    rec["sample_final"] = final
    # G10: rotation conversions
    rs = np.random.RandomState(3)
    q = C.rs_tensor(rs, (6, 4))
    qn = R.utils.normalise_quat(q)
    mat = R.p3d.quaternion_to_matrix(qn)
    o6 = R.utils.get_ortho6d_from_rotation_matrix(mat)
    rec["rot"] = dict(q=q, qn=qn, mat=mat, o6=o6, mat_back=R.utils.compute_rotation_matrix_from_ortho6d(o6 * 1.7),
                      q_back=R.p3d.matrix_to_quaternion(mat))
    man = {n: tuple(p.shape) for n, p in m.named_parameters() if not n.startswith("prediction_head.backbone")}
    rec["manifest"] = dict(named_parameters=man, n_trainable=sum(int(np.prod(s)) for s in man.values()),
                           with_grad=sorted(grads.keys()))
    save("diffusion.pt", rec)


def golden_diffusion_multi():
    """The multi-round / multi-scale head (diffusion_head.py:249-275): attn_rounds = 2, feat_scales_to_use = 2, untied
    module sets, goal-conditioned (so that scale 1 attends to the find_traj_nn neighbourhood of the previous prediction).
    Dropout is zeroed (p = 0 in every nn.Dropout / attention module) so that train-mode gradients are deterministic."""
    E, B, Ln, ncam = 120, 2, 8, 1
    m = R.dm.DiffusionPlanner(backbone="clip", image_size=(256, 256), embedding_dim=E, output_dim=7,
                              num_vis_ins_attn_layers=2, num_query_cross_attn_layers=6, use_instruction=True,
                              use_goal=True, use_goal_at_test=True, feat_scales_to_use=2, attn_rounds=2,
                              weight_tying=False, gripper_loc_bounds=C.DIFFUSION_BOUNDS, rotation_parametrization="6D",
                              diffusion_timesteps=100)
    shapes, alias = C.unique_param_shapes(m)
    seed = 91
    sd = C.expand_aliases(C.seeded_state_dict(shapes, seed, gain=1.5), alias)
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if hasattr(mod, "dropout") and isinstance(getattr(mod, "dropout"), float):
            mod.dropout = 0.0
    inp = C.trajectory_inputs(seed, B, Ln, ncam, E, pad_last=2)
    fine = C.fine_feature_map(seed, B, ncam, E)
    head = m.prediction_head

    def fake_encode_images(rgb, pcd):
        import einops
        out = []
        for f in (8, 2):
            p = einops.rearrange(pcd, "bt ncam c h w -> (bt ncam) c h w")
            p = F.interpolate(p, scale_factor=1. / f, mode='bilinear')
            out.append(einops.rearrange(p, "(bt ncam) c h w -> bt (ncam h w) c", ncam=ncam))
        return [inp["fmap"], fine], out
    head.encode_images = fake_encode_images
    rgb = torch.zeros(B, ncam, 3, 256, 256)
    rec = dict(cfg=dict(E=E, B=B, L=Ln, ncam=ncam, pad_last=2, attn_rounds=2, feat_scales=2), seed=seed, gain=1.5,
               param_shapes=shapes, alias=alias)
    m.train()
    with patched_rng([inp["noise"]], inp["timesteps"]):
        loss = m(inp["trajectory"], inp["mask"], rgb, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"])
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None and "feature_pyramid" not in n}
    rec["train_loss"] = loss.detach()
    rec["grad_norms"] = {n: g.norm().item() for n, g in grads.items()}
    keep = ["prediction_head.traj_encoder.0.weight", "prediction_head.traj_attention.3.layers.0.adaln_12.modulation.1.weight",
            "prediction_head.pos_attention.1.layers.1.sa1.in_proj_weight", "prediction_head.pos_regressor.2.3.weight",
            "prediction_head.vl_attention.1.layers.1.cross_12.in_proj_weight", "prediction_head.rot_regressor.3.0.weight"]
    rec["grads"] = {n: grads[n].clone() for n in keep}
    m.eval()
    spy = {}
    import model.trajectory_optimization.diffusion_head as dh
    orig_nn = dh.find_traj_nn

    def rec_nn(traj, pc, nn_=64):
        out = orig_nn(traj, pc, nn_)
        spy.setdefault("nn", []).append(out.clone())
        return out
    dh.find_traj_nn = rec_nn
    with torch.no_grad():
        tr9 = m.convert_rot(torch.cat([m.normalize_pos(inp["trajectory"][..., :3]), inp["trajectory"][..., 3:]], -1))
        pcdn = torch.permute(m.normalize_pos(torch.permute(inp["pcd"], [0, 1, 3, 4, 2])), [0, 1, 4, 2, 3])
        cg = inp["curr_gripper"].clone(); cg[:, :3] = m.normalize_pos(cg[:, :3]); cg = m.convert_rot(cg)
        gg = inp["goal_gripper"].clone(); gg[:, :3] = m.normalize_pos(gg[:, :3]); gg = m.convert_rot(gg)
        preds = head(tr9, inp["mask"], inp["timesteps"], rgb, pcdn, cg, gg, inp["instr"])
    dh.find_traj_nn = orig_nn
    rec["head_in"] = tr9
    rec["head_outs"] = [p.clone() for p in preds]
    rec["nn_indices"] = spy["nn"]
    rec["conv"] = dict(curr9=cg, goal9=gg)
    # a short sampling run (5 denoise steps) through the reference's own loop
    sn = inp["step_noise"]
    m.position_noise_scheduler.injected_noise = {t: sn[t][..., :3] for t in range(100)}
    m.rotation_noise_scheduler.injected_noise = {t: sn[t][..., 3:] for t in range(100)}
    trace = []
    orig = m.policy_forward_pass
    calls = {"n": 0}

    class Stop(Exception):
        pass

    def limited(trajectory, timestep, fixed_inputs):
        if calls["n"] == 5:
            trace.append(trajectory.detach().clone())
            raise Stop()
        calls["n"] += 1
        return orig(trajectory, timestep, fixed_inputs)
    m.policy_forward_pass = limited
    try:
        with torch.no_grad(), patched_rng([inp["init_noise"]], inp["timesteps"]):
            m(inp["trajectory"], inp["mask"], rgb, inp["pcd"], inp["instr"], inp["curr_gripper"], inp["goal_gripper"],
              run_inference=True)
    except Stop:
        pass
    rec["sample_state_after_5_steps"] = trace[0]
    save("diffusion_multi.pt", rec)


def golden_optimizer():
    """G11: which names land in which AdamW group + one AdamW step on a toy module (engine.py:89-102)."""
    import types
    rs = np.random.RandomState(9)
    mod = torch.nn.Sequential()
    mod.add_module("lin", torch.nn.Linear(6, 4))
    mod.add_module("norm", torch.nn.LayerNorm(4))
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(C.rs_tensor(rs, tuple(p.shape)))
    no_decay = ["bias", "LayerNorm.weight", "LayerNorm.bias"]
    groups = [{"params": [], "weight_decay": 0.0, "lr": 1e-4}, {"params": [], "weight_decay": 5e-4, "lr": 1e-4}]
    names = [[], []]
    for name, p in mod.named_parameters():
        gi = 0 if any(nd in name for nd in no_decay) else 1
        groups[gi]["params"].append(p)
        names[gi].append(name)
    opt = torch.optim.AdamW(groups)
    before = {n: p.detach().clone() for n, p in mod.named_parameters()}
    gr = {n: C.rs_tensor(rs, tuple(p.shape)) for n, p in mod.named_parameters()}
    for it in range(2):
        for n, p in mod.named_parameters():
            p.grad = gr[n].clone() * (it + 1)
        opt.step()
    save("optimizer.pt", dict(groups=names, before=before, grads=gr, after={n: p.detach().clone() for n, p in mod.named_parameters()}))


def golden_metrics():
    """G13: evaluation metrics (main_trajectory.py:306-343, main_keypose.py:431-482) and the non-default loss options
    (symmetric_rotation_loss, position_loss="mse") of main_keypose.py:368-386."""
    pred, gt, action, kp, tasks = C.metrics_inputs()
    out = {}
    r1, r2 = R.main_trajectory.TrajectoryCriterion.compute_metrics(pred, gt, torch.zeros(pred.shape[:2], dtype=torch.bool))
    out["traj"] = dict(summary={k: v.clone() for k, v in r1.items()}, per_traj={k: v.clone() for k, v in r2.items()})
    for sym in (False, True):
        crit = R.main_keypose.LossAndMetrics(position_loss="mse", rotation_parametrization="quat_from_query",
                                             ground_truth_gaussian_spread=0.01, symmetric_rotation_loss=sym)
        sample = {"action": action, "task": tasks}
        p = {k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in kp.items()}
        p["rotation"].requires_grad_()
        p["position"].requires_grad_()
        losses = crit.compute_loss(p, sample)
        sum(losses.values()).backward()
        met = crit.compute_metrics({k: (v.detach() if torch.is_tensor(v) else v) for k, v in p.items()}, sample)
        out[f"keypose_sym{int(sym)}"] = dict(losses={k: v.detach().clone() for k, v in losses.items()},
                                             d_rotation=p["rotation"].grad.clone(), d_position=p["position"].grad.clone(),
                                             metrics={k: v.clone() for k, v in met.items()})
    save("metrics.pt", out)


def _import_reference_datasets():
    """The reference's `datasets` package (datasets/dataset_engine.py, datasets/utils.py) under the alias `refdatasets` (the
    name `datasets` is taken by an unrelated installed package and by refimport's inert stub).  torchvision / blosc are not
    installed: `torchvision.transforms(.functional)` is stubbed by the torch operators torchvision 0.14 dispatches to for
    float tensors -- resize(NEAREST) = F.interpolate(mode="nearest"), pad(reflect) = F.pad(mode="reflect"), crop = slice,
    RandomCrop.get_params = two torch.randint draws unless the size already matches (third-party: parity unpinned there);
    everything else that runs is the reference's own code."""
    import importlib.util
    import types

    def resize(img, size, interpolation=None):
        return F.interpolate(img, size=list(size), mode="nearest")

    def pad(img, padding, padding_mode="constant"):
        left, top, right, bottom = padding
        return F.pad(img, [left, right, top, bottom], mode=padding_mode)

    def crop(img, i, j, h, w):
        return img[..., i:i + h, j:j + w]

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            h, w = img.shape[-2:]
            th, tw = output_size
            if h < th or w < tw:
                raise ValueError("Required crop size is larger than input image size")
            if w == tw and h == th:
                return 0, 0, h, w
            i = torch.randint(0, h - th + 1, size=(1,)).item()
            j = torch.randint(0, w - tw + 1, size=(1,)).item()
            return i, j, th, tw

    tvt = sys.modules["torchvision.transforms"]
    tvt.InterpolationMode = types.SimpleNamespace(NEAREST="nearest")
    tvt.RandomCrop = RandomCrop
    fmod = types.ModuleType("torchvision.transforms.functional")
    fmod.resize, fmod.pad, fmod.crop = resize, pad, crop
    sys.modules["torchvision.transforms.functional"] = fmod
    tvt.functional = fmod
    sys.modules.setdefault("blosc", types.ModuleType("blosc"))
    spec = importlib.util.spec_from_file_location("refdatasets", "/root/reference/datasets/__init__.py",
                                                  submodule_search_locations=["/root/reference/datasets"])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["refdatasets"] = pkg
    spec.loader.exec_module(pkg)
    import refdatasets.dataset_engine as de
    return de


def golden_dataset():
    """Data plane: items of the reference's RLBenchDataset (training: with the Resize augmentation; evaluation)
    on the synthetic episodes of common.write_synthetic_dataset, and the collated batches of the two main scripts."""
    import random
    import tempfile
    de = _import_reference_datasets()
    out = {}
    with tempfile.TemporaryDirectory() as root:
        instr = C.write_synthetic_dataset(root)
        for tag, training, traj in (("train_traj", True, True), ("eval_traj", False, True), ("train_keypose", True, False)):
            random.seed(5)
            np.random.seed(5)
            torch.manual_seed(5)
            ds = de.RLBenchDataset(root=root, instructions=instr, taskvar=C.DATASET_TASKVAR, max_episode_length=5, cache_size=0,
                                   max_episodes_per_task=100, cameras=C.DATASET_CAMERAS, training=training,
                                   gripper_loc_bounds=C.PERACT_BOUNDS, image_rescale=(0.75, 1.25),
                                   point_cloud_rotate_yaw_range=0.0, return_low_lvl_trajectory=traj, dense_interpolation=traj,
                                   interpolation_length=12, action_dim=8, predict_short=False)
            items = [ds[i] for i in range(5)]
            collate = R.main_trajectory.traj_collate_fn if traj else R.main_keypose.keypose_collate_fn
            batch = collate(items)
            rec = {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in batch.items()}
            rec["instr_sample"] = rec.pop("instr")[:, ::13, ::64].clone()          # (frames, 5, 8) of the (frames, 53, 512)
            rec["frames_per_item"] = [len(it["task"]) for it in items]
            rec["history"] = torch.cat([it["curr_gripper_history"] for it in items])
            rec["len"] = len(ds)
            out[tag] = rec
            print(tag, {k: (tuple(v.shape) if torch.is_tensor(v) else v) for k, v in rec.items() if k != "task"})
    save("dataset.pt", out)


# ------------------------------------------------------------------------------------------------------ harness rows (f-4)
class _DictWriter:
    """Stand-in for tensorboard's SummaryWriter (absent here): records what the reference's harness logs."""

    def __init__(self):
        self.scalars, self.images = {}, []

    def add_scalar(self, key, value, step):
        self.scalars[key] = (float(value), int(step))

    def add_image(self, key, img, step):
        self.images.append(key)


def _init_single_process_group():
    import tempfile
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="file://" + tempfile.mktemp(), rank=0, world_size=1)


def _reference_engine():
    """The reference's own engine.py (BaseTrainTester.save_checkpoint / load_checkpoint / get_optimizer), imported under
    another name with torch.utils.tensorboard stubbed (refimport replaces `engine` by an inert placeholder for the model
    imports)."""
    import importlib.util
    import types
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = _DictWriter
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    spec = importlib.util.spec_from_file_location("ref_engine_real", "/root/reference/engine.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden_harness():
    """f-4: records produced by the REFERENCE'S OWN harness code on seeded inputs --
      keypose:    main_keypose.TrainTester.evaluate_nsteps (main_keypose.py:236-281) over two batches, free-running eval
                  forward of the reference Act3D (numpy ghost sampler seeded), every scalar it logs + its return value;
      trajectory: main_trajectory.TrainTester.evaluate_nsteps (main_trajectory.py:206-274) over two batches with two task
                  names (per-task keys), 100-step sampling with injected noise;
      checkpoint: engine.BaseTrainTester.get_optimizer + one AdamW step + save_checkpoint (engine.py:89-102,214-230): the
                  file's structure, every tensor's (sum, abs-sum) and a few whole tensors -- not the 80 MB file.
    The product's KeyposeTrainTester / TrajectoryTrainTester / engine.save_checkpoint are compared with these on the GPU."""
    import types
    _init_single_process_group()
    out = {}
    # ---- keypose evaluate_nsteps
    E, levels, ncam, Ng, B = 60, 2, 1, 48, 2
    for attempt in range(60):
        seed, gain = 300 + attempt, 3.0
        m, _ = build_ref_act3d(E, levels, ncam, Ng, False, seed, gain, Ng_val=Ng)
        m.eval()
        batches = [C.keypose_inputs(seed + 1000 * (j + 1), B, ncam, E, levels) for j in range(2)]
        state = {"j": 0}

        def fake(visible_rgb, visible_pcd, num_cameras, m=m, batches=batches, state=state):
            import einops
            inp = batches[state["j"]]
            pcd = einops.rearrange(visible_pcd, "bt ncam c h w -> (bt ncam) c h w")
            feats, poss, pcds = [], [], []
            for i in range(m.num_sampling_level):
                p_ = F.interpolate(pcd, scale_factor=1. / m.downscaling_factor_pyramid[i], mode='bilinear')
                p_ = einops.rearrange(p_, "(bt ncam) c h w -> bt (ncam h w) c", ncam=num_cameras)
                feats.append(inp["feats"][i])
                poss.append(m.relative_pe_layer(p_))
                pcds.append(p_)
            return feats, poss, pcds
        m._compute_visual_features = fake
        gaps = []
        orig_forward = m.forward

        def spy(*a, m=m, orig_forward=orig_forward, gaps=gaps, state=state, **k):
            o = orig_forward(*a, **k)
            for masks in o["ghost_pcd_masks_pyramid"]:
                top2 = masks[-1].topk(2, dim=-1).values
                gaps.append((top2[:, 0] - top2[:, 1]).min().item())
            state["j"] += 1
            return o
        m.forward = spy
        loader = [{"rgbs": torch.zeros(B, ncam, 3, 256, 256), "pcds": b_["pcd"], "instr": b_["instr"], "curr_gripper": b_["curr_gripper"],
                   "action": b_["action"], "task": ["task_a", "task_b"]} for b_ in batches]
        tester = R.main_keypose.TrainTester.__new__(R.main_keypose.TrainTester)
        tester.args = types.SimpleNamespace()
        tester.writer = _DictWriter()
        crit = R.main_keypose.LossAndMetrics(position_loss="ce", rotation_parametrization="quat_from_query",
                                             ground_truth_gaussian_spread=0.01)
        np.random.seed(seed)
        ret = tester.evaluate_nsteps(m, crit, loader, step_id=7, val_iters=5, split="val")
        if min(gaps) > 1e-2:
            break
    else:
        raise RuntimeError("no keypose harness seed with a safe top-2 logit gap")
    print("harness keypose seed", seed, "gaps", gaps, "scalars", len(tester.writer.scalars))
    out["keypose"] = dict(cfg=dict(E=E, levels=levels, ncam=ncam, Ng=Ng, B=B), seed=seed, gain=gain, batch_seeds=[seed + 1000, seed + 2000],
                          np_seed=seed, step_id=7, scalars=dict(tester.writer.scalars), returned=ret, gaps=gaps)
    # ---- trajectory evaluate_nsteps
    E, B, Ln, ncam = 120, 2, 8, 1
    m = R.dm.DiffusionPlanner(backbone="clip", image_size=(256, 256), embedding_dim=E, output_dim=7, num_vis_ins_attn_layers=2,
                              num_query_cross_attn_layers=6, use_instruction=True, use_goal=True, use_goal_at_test=True,
                              feat_scales_to_use=1, attn_rounds=1, weight_tying=True, gripper_loc_bounds=C.DIFFUSION_BOUNDS,
                              rotation_parametrization="6D", diffusion_timesteps=100)
    shapes, alias = C.unique_param_shapes(m)
    seed = 77
    res = m.load_state_dict(C.expand_aliases(C.seeded_state_dict(shapes, seed, gain=1.5), alias), strict=False)
    assert not res.unexpected_keys
    m.eval()
    tb = [C.trajectory_inputs(seed + 10 * (j + 1), B, Ln, ncam, E, pad_last=2) for j in range(2)]
    state = {"j": 0}

    def fake_encode_images(rgb, pcd):
        import einops
        p_ = einops.rearrange(pcd, "bt ncam c h w -> (bt ncam) c h w")
        p_ = F.interpolate(p_, scale_factor=1. / 8, mode='bilinear')
        p_ = einops.rearrange(p_, "(bt ncam) c h w -> bt (ncam h w) c", ncam=ncam)
        return [tb[state["j"]]["fmap"]], [p_]
    m.prediction_head.encode_images = fake_encode_images
    loader = [{"trajectory": b_["trajectory"], "trajectory_mask": b_["mask"], "rgbs": torch.zeros(B, ncam, 3, 256, 256), "pcds": b_["pcd"],
               "instr": b_["instr"], "curr_gripper": b_["curr_gripper"], "action": b_["goal_gripper"], "task": ["task_a", "task_b"]}
              for b_ in tb]
    tester = R.main_trajectory.TrainTester.__new__(R.main_trajectory.TrainTester)
    tester.args = types.SimpleNamespace()
    tester.writer = _DictWriter()
    tester.synchronize_between_processes = lambda d: d          # BaseTrainTester's (engine.py:232-246) is the identity on one process
    crit = R.main_trajectory.TrajectoryCriterion()
    orig_forward = m.forward

    def fwd(*a, **k):
        inp = tb[state["j"]]
        sn = inp["step_noise"]
        m.position_noise_scheduler.injected_noise = {t: sn[t][..., :3] for t in range(100)}
        m.rotation_noise_scheduler.injected_noise = {t: sn[t][..., 3:] for t in range(100)}
        with patched_rng([inp["init_noise"]], inp["timesteps"]):
            o = orig_forward(*a, **k)
        state["j"] += 1
        return o
    m.forward = fwd
    # the matplotlib / cv2 trajectory plot of the first batch is out of scope (cv2 is a stub here): a placeholder image
    R.main_trajectory.generate_visualizations = lambda pred, gt, mask: np.zeros((3, 4, 4), dtype=np.uint8)
    ret = tester.evaluate_nsteps(m, crit, loader, step_id=11, val_iters=5, split="val")
    print("harness trajectory scalars", len(tester.writer.scalars), "returned", ret)
    out["trajectory"] = dict(cfg=dict(E=E, B=B, L=Ln, ncam=ncam, pad_last=2), seed=seed, gain=1.5, batch_seeds=[seed + 10, seed + 20],
                             step_id=11, scalars=dict(tester.writer.scalars), returned=ret, images=list(tester.writer.images))
    # ---- checkpoint written by the reference's engine
    import tempfile
    from pathlib import Path
    RE = _reference_engine()
    m, _ = build_ref_act3d(60, 2, 1, 48, False, 300, 3.0, Ng_val=48)
    for p_ in m.backbone.parameters():
        p_.requires_grad = False
    bt = RE.BaseTrainTester.__new__(RE.BaseTrainTester)
    with tempfile.TemporaryDirectory() as td:
        bt.args = types.SimpleNamespace(lr=1e-4, log_dir=Path(td))
        opt = bt.get_optimizer(m)
        g = torch.Generator().manual_seed(5)
        unused = [n for n, p_ in m.named_parameters() if "feature_pyramid" in n and (".1.0." in n or ".3.0." in n or ".4.0." in n)]
        for n, p_ in m.named_parameters():
            if p_.requires_grad and n not in unused:
                p_.grad = torch.randn(p_.shape, generator=g) * 0.01
        opt.step()
        best = bt.save_checkpoint(m, opt, step_id=4, new_loss=None, best_loss=None)
        files = sorted(os.listdir(td))
        ck = torch.load(os.path.join(td, "last.pth"), map_location="cpu", weights_only=False)
    chk = lambda t: (float(t.double().sum()), float(t.double().abs().sum()))
    names = [n for n, _ in m.named_parameters()]
    ostate = ck["optimizer"]["state"]
    # torch.optim state indices -> parameter names, through the optimizer's own groups (engine.py:89-102: "bias" group first)
    by_id = {id(p_): n for n, p_ in m.named_parameters()}
    group_names = [[by_id[id(p_)] for p_ in g_["params"]] for g_ in opt.param_groups]
    index_name = [n for g_ in group_names for n in g_]
    nb = lambda n: not n.startswith("backbone")
    out["checkpoint"] = dict(
        files=files, keys=sorted(ck.keys()), iter=ck["iter"], best_loss=ck["best_loss"], returned_best=best,
        weight_keys=[k for k in ck["weight"].keys() if nb(k)],
        weight_checksums={k: chk(v) for k, v in ck["weight"].items() if nb(k) and "feature_pyramid" not in k and v.dtype.is_floating_point},
        param_group_options=[{k: v for k, v in g_.items() if k != "params"} for g_ in ck["optimizer"]["param_groups"]],
        group_sizes=[len(g_["params"]) for g_ in ck["optimizer"]["param_groups"]],
        group_names=[[n for n in g_ if nb(n)] for g_ in group_names],
        state_by_name={index_name[int(i)]: dict(step=float(st["step"]), exp_avg=chk(st["exp_avg"]), exp_avg_sq=chk(st["exp_avg_sq"]))
                       for i, st in ostate.items()},
        named_parameters=[n for n in names if nb(n)], unused=unused, grad_seed=5, grad_scale=0.01,
        model=dict(E=60, levels=2, ncam=1, Ng=48, seed=300, gain=3.0),
        samples={k: ck["weight"][k].clone() for k in ("query_embed.weight", "gripper_state_predictor.2.bias")})
    print("harness checkpoint: files", files, "state entries", len(ostate), "of", len(names))
    save("harness.pt", out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["blocks", "sampling", "act3d", "act3d_cfg1", "act3d_options", "diffusion", "diffusion_multi", "optimizer", "metrics", "dataset", "harness"]
    for w in which:
        globals()["golden_" + w]()
