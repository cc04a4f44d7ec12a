"""Pinned waypoints, restated in torch on the CPU: the rule of a3d_traj_pins (csrc/traj_pins.hip) slot by slot, and a pinned sampling
loop composed from the CPU oracle's pieces (oracle.diffusion.make_conditioning, head_forward, DDPMSchedules.step_with_inpaint).

The rule.  last = L - pad_b - 1 is the scene's last valid row.  Slot p of scene b is APPLIED iff (channels & 7) != 0 and
1 <= index <= last - 1 (use_goal) or 1 <= index <= last (no goal): row 0, the goal row, padded rows and all-padding scenes are never
touched.  An applied slot writes, for every selected channel group (bit 0: signal columns 0..2, bit 1: 3..8, bit 2: 9..D-1) and every
candidate g of the scene, cond_data = sig, cond_mask = 1 and traj = init_noise + sig (one fp32 add).  Slots are applied in ascending
order, so where two select one element the higher slot wins.  Everything else keeps its bits."""
import torch

CHANNEL_COLUMNS = ((1, 0, 3), (2, 3, 9), (4, 9, None))         # (bit, first column, one past the last column; None = D)


def pins_ref(cond_data, cond_mask, traj, init_noise, sig, index, channels, tmask, G, use_goal=True):
    """cond_data / cond_mask / traj (or None) / init_noise (or None): (B G, L, D) CPU tensors; sig: (B, P, D) the pins as network
    signals; index (B, P) integer; channels (B, P) uint8 bit masks; tmask (B, L), non-zero = padded.  Returns new tensors
    (cond_data, cond_mask, traj or None, applied (B, P) uint8); the arguments are left unchanged."""
    cond_data, cond_mask = cond_data.clone(), cond_mask.clone()
    traj = None if traj is None else traj.clone()
    B, P, D = sig.shape
    L = tmask.shape[1]
    applied = torch.zeros((B, P), dtype=torch.uint8)
    for b in range(B):
        last = L - int((tmask[b] != 0).sum()) - 1
        hi = last - 1 if use_goal else last
        for p in range(P):
            ch, row = int(channels[b, p]) & 7, int(index[b, p])
            if ch == 0 or not 1 <= row <= hi:
                continue
            applied[b, p] = 1
            for bit, c0, c1 in CHANNEL_COLUMNS:
                if not ch & bit:
                    continue
                cols = slice(c0, D if c1 is None else min(c1, D))
                for g in range(G):
                    r = b * G + g
                    cond_data[r, row, cols] = sig[b, p, cols]
                    cond_mask[r, row, cols] = 1
                    if traj is not None:
                        traj[r, row, cols] = init_noise[r, row, cols] + sig[b, p, cols]
    return cond_data, cond_mask, traj, applied


def oracle_pinned_loop(P_, inp, tokens, sub, pin_poses, pin_index, pin_channels, n_steps, H, bounds, T=100):
    """The first n_steps steps of the full DDPM chain on the trajectories `sub` of a batch, with pins, from the oracle's pieces.
    inp: the per-trajectory inputs (pcd, curr_gripper, goal_gripper, mask, instr, init_noise (N, L, 9), step_noise (T, N, L, 9) by
    timestep); pin_poses (N, P, 7) / pin_index (N, P) / pin_channels (N, P): the pins of every TRAJECTORY (G = 1 here).  The pins are
    converted by the oracle's own normalize_pos / convert_rot.  Returns (final poses (len(sub), L, 7), [state after every step])."""
    from oracle import diffusion as OD
    from oracle import sampling as OS
    bounds = torch.as_tensor(bounds)
    pcdn = OD.normalize_pos(inp["pcd"][sub].permute(0, 1, 3, 4, 2), bounds).permute(0, 1, 4, 2, 3).contiguous()
    cxyz = torch.from_numpy(OS.pcd_downsample(pcdn.numpy(), 8))

    def to_signal(pose):
        pose = pose.clone()
        pose[..., :3] = OD.normalize_pos(pose[..., :3], bounds)
        return OD.convert_rot(pose)

    cg, gg = to_signal(inp["curr_gripper"][sub]), to_signal(inp["goal_gripper"][sub])
    mask, toks, instr = inp["mask"][sub], tokens[sub], inp["instr"][sub]
    sig = to_signal(pin_poses[sub].reshape(-1, pin_poses.shape[-1])).reshape(len(sub), pin_poses.shape[1], -1)
    cond, cmask = OD.make_conditioning(mask, cg, gg)
    cond, cm_u8, _, _ = pins_ref(cond, cmask.to(torch.uint8), None, None, sig, pin_index[sub], pin_channels[sub], mask, 1, True)
    cmask = cm_u8.bool()
    sched = OD.DDPMSchedules(T)
    traj = inp["init_noise"][sub] + cond
    trace = []
    with torch.no_grad():
        for t in list(range(T - 1, -1, -1))[:n_steps]:
            out = OD.head_forward(P_, traj, mask, torch.full((traj.shape[0],), t, dtype=torch.long), toks, cxyz, cg, gg, instr, H)
            traj = sched.step_with_inpaint(out, traj, inp["step_noise"][t][sub], cond, cmask, t)
            trace.append(traj.clone())
    final = OD.unconvert_rot(traj)
    return torch.cat([OD.unnormalize_pos(final[..., :3], bounds), final[..., 3:]], dim=-1), trace
