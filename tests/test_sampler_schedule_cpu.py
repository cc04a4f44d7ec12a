"""Few-step sampler schedules (diffusion.SamplerSchedule: strided ancestral DDPM and DDIM with eta) on the host: timesteps and
coefficient tables against a float64 restatement written here, the identities that tie the schedules to DDPMTables and to each
other, the argument errors of the public interface, and the host-side argument validation of the new C-ABI entry points."""
import ctypes
import math

import pytest
import torch

from conftest import load_pkg

T = 100
CPU = torch.device("cpu")


def _tables():
    return load_pkg().diffusion.DDPMTables(T, CPU)


# ---- the semantics, restated in float64 (python floats) on the float32 alphas_cumprod of DDPMTables
def ref_timesteps(K):
    r = T // K
    return [(K - 1 - i) * r for i in range(K)], r


def ref_rows(acp, K, scheduler, eta):
    ts, r = ref_timesteps(K)
    rows = []
    for t in ts:
        a_t = float(acp[t])
        a_prev = float(acp[t - r]) if t - r >= 0 else 1.0
        if scheduler == "ddpm":
            cur_a = a_t / a_prev
            var = max((1 - a_prev) / (1 - a_t) * (1 - cur_a), 1e-20)
            rows.append([math.sqrt(a_prev) * (1 - cur_a) / (1 - a_t), math.sqrt(cur_a) * (1 - a_prev) / (1 - a_t),
                         math.sqrt(var) if t - r >= 0 else 0.0])
        else:
            sigma = eta * math.sqrt((1 - a_prev) / (1 - a_t)) * math.sqrt(1 - a_t / a_prev)
            c1 = math.sqrt(max(1 - a_prev - sigma * sigma, 0.0)) / math.sqrt(1 - a_t)
            rows.append([math.sqrt(a_prev) - c1 * math.sqrt(a_t), c1, sigma])
    return torch.tensor(rows, dtype=torch.float64)


@pytest.mark.parametrize("K", [1, 3, 7, 10, 20, 33, 50, 64, 100])
def test_leading_timesteps(K):
    D = load_pkg().diffusion
    ts, r = D.sampler_timesteps(T, K)
    assert (ts, r) == ref_timesteps(K)
    assert len(ts) == K and ts[-1] == 0 and ts[0] == (K - 1) * (T // K) < T
    assert all(a - b == r for a, b in zip(ts, ts[1:]))
    sc = D.SamplerSchedule(_tables(), K)
    assert sc.timesteps == ts and sc.stride == r and sc.K == K and sc.T == T
    assert sc.coef_pos.shape == (K, 3) and sc.coef_rot.shape == (K, 3) and sc.coef_pos.dtype == torch.float32


@pytest.mark.parametrize("K,scheduler,eta", [(10, "ddpm", 0.0), (20, "ddpm", 0.0), (100, "ddpm", 0.0), (7, "ddpm", 0.0),
                                             (10, "ddim", 0.0), (20, "ddim", 0.5), (50, "ddim", 1.0), (100, "ddim", 0.3),
                                             (1, "ddim", 0.0), (1, "ddpm", 0.0)])
def test_tables_against_the_float64_restatement(K, scheduler, eta):
    """The float32 tables are the float64 formulas rounded.  "ddim" is evaluated in float64 and rounded once: half a float32 ulp of
    a coefficient <= 1, 1e-7.  "ddpm" keeps DDPMTables' float32 arithmetic, whose error is the cancellation in 1 - a_t / a_prev: the
    quotient is rounded near 1 (2^-24 absolute) and the posterior divides by 1 - a_t, so a row is held to 4 * 2^-24 / (1 - a_t)
    (quotient, difference, product, root) + 1e-6 -- about 1e-3 at t = 1, where 1 - a_t = 2.3e-4, and 1e-6 over most of the chain."""
    D = load_pkg().diffusion
    tb = _tables()
    sc = D.SamplerSchedule(tb, K, scheduler, eta)
    for got, acp in ((sc.coef_pos, tb.acp_pos), (sc.coef_rot, tb.acp_rot)):
        ref = ref_rows(acp, K, scheduler, eta)
        err = (got.double() - ref).abs().max(dim=1).values
        if scheduler == "ddim":
            tol = torch.full((K,), 1e-7, dtype=torch.float64)
        else:
            tol = torch.tensor([4 * 2.0 ** -24 / (1 - float(acp[t])) + 1e-6 for t in sc.timesteps], dtype=torch.float64)
        assert bool((err <= tol).all()), (scheduler, K, eta, err.max().item())
        # the float64 evaluation of the same function is the restatement to rounding
        got64 = D.sampler_coefficients(acp.double(), sc.timesteps, sc.stride, scheduler, eta)
        assert got64.dtype == torch.float64 and (got64 - ref).abs().max().item() <= 1e-12
    # the terminal row: x_prev = clip(x0), no noise (the kernels return the in-painted output there without reading the row)
    assert sc.coef_pos[-1].tolist() == [1.0, 0.0, 0.0] and sc.coef_rot[-1].tolist() == [1.0, 0.0, 0.0]


def test_full_ddpm_schedule_is_the_training_chain_bit_for_bit():
    D = load_pkg().diffusion
    tb = _tables()
    sc = D.SamplerSchedule(tb, T, "ddpm")
    assert sc.timesteps == list(range(T - 1, -1, -1)) and sc.stride == 1
    assert torch.equal(sc.coef_pos, tb.coef_pos.flip(0)) and torch.equal(sc.coef_rot, tb.coef_rot.flip(0))
    # default K = T
    sd = D.SamplerSchedule(tb)
    assert sd.K == T and torch.equal(sd.coef_pos, sc.coef_pos) and torch.equal(sd.coef_rot, sc.coef_rot)
    # DDPMTables itself still restates the oracle's table
    from oracle import diffusion as OD
    o = OD.DDPMSchedules(T)
    assert torch.equal(tb.coef_pos, o.coef_pos) and torch.equal(tb.coef_rot, o.coef_rot)


@pytest.mark.parametrize("K", [1, 5, 10, 20, 50, 100])
def test_ddim_eta_one_is_strided_ddpm(K):
    """sigma(eta = 1)^2 is the fixed_small posterior variance, and then c1, c0 are the posterior-mean coefficients: algebraically
    equal, compared in float64."""
    D = load_pkg().diffusion
    tb = _tables()
    ts, r = D.sampler_timesteps(T, K)
    for acp in (tb.acp_pos.double(), tb.acp_rot.double()):
        a = D.sampler_coefficients(acp, ts, r, "ddpm")
        b = D.sampler_coefficients(acp, ts, r, "ddim", 1.0)
        assert a.dtype == b.dtype == torch.float64
        assert (a - b).abs().max().item() <= 1e-12, (K, (a - b).abs().max().item())


@pytest.mark.parametrize("K", [1, 10, 20, 100])
def test_ddim_eta_zero_is_noise_free(K):
    D = load_pkg().diffusion
    sc = D.SamplerSchedule(_tables(), K, "ddim", 0.0)
    assert sc.noise_free
    assert torch.equal(sc.coef_pos[:, 2], torch.zeros(K)) and torch.equal(sc.coef_rot[:, 2], torch.zeros(K))
    assert not D.SamplerSchedule(_tables(), K, "ddim", 0.5).noise_free and not D.SamplerSchedule(_tables(), K, "ddpm").noise_free
    # deterministic DDIM keeps the marginal: c0^2-free check of the eps form, x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps
    tb = _tables()
    for got, acp in ((sc.coef_pos, tb.acp_pos), (sc.coef_rot, tb.acp_rot)):
        for i, t in enumerate(sc.timesteps[:-1]):
            a_t, a_prev = float(acp[t]), float(acp[t - sc.stride])
            assert abs(float(got[i, 1]) * math.sqrt(1 - a_t) - math.sqrt(1 - a_prev)) <= 1e-6
            assert abs(float(got[i, 0]) + float(got[i, 1]) * math.sqrt(a_t) - math.sqrt(a_prev)) <= 1e-6


def test_value_errors_of_the_schedule_arguments():
    D = load_pkg().diffusion
    tb = _tables()
    bad = [dict(num_inference_steps=0), dict(num_inference_steps=T + 1), dict(num_inference_steps=-3), dict(num_inference_steps=2.5),
           dict(scheduler="euler"), dict(scheduler="ddim", eta=-0.1), dict(scheduler="ddim", eta=1.5), dict(scheduler="ddpm", eta=0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            D.SamplerSchedule(tb, **kw)
        with pytest.raises(ValueError):
            D.check_sampler_args(T, **kw)
    assert D.check_sampler_args(T) == T and D.check_sampler_args(T, 10, "ddim", 1.0) == 10


def test_compute_trajectory_raises_before_any_launch():
    """The public method checks the schedule arguments and the leading size of step_noise on the host, before it touches the
    device: on CPU tensors the bad calls raise ValueError (a good call would go on to the kernels, which need the GPU)."""
    a3d = load_pkg()
    m = a3d.DiffusionPlanner(embedding_dim=60, num_attn_heads=4, num_query_cross_attn_layers=6, use_instruction=True, use_goal=True,
                             gripper_loc_bounds=[[-1, -1, -1], [1, 1, 1]], rotation_parametrization="6D", diffusion_timesteps=T)
    B, Ln = 2, 8
    mask = torch.zeros(B, Ln, dtype=torch.bool)
    args = (mask, None, torch.zeros(B, 1, 3, 16, 16), torch.zeros(B, 53, 512), torch.zeros(B, 8), torch.zeros(B, 8))
    bad = [dict(num_inference_steps=0), dict(num_inference_steps=T + 1), dict(scheduler="euler"), dict(scheduler="ddim", eta=2.0),
           dict(scheduler="ddim", eta=-1.0), dict(eta=0.5), dict(num_inference_steps=10, eta=1.0),
           dict(num_inference_steps=10, step_noise=torch.zeros(T, B, Ln, 9)),
           dict(num_inference_steps=10, scheduler="ddim", eta=0.5, step_noise=torch.zeros(9, B, Ln, 9)),
           dict(scheduler="ddim", eta=1.0, step_noise=torch.zeros(10, B, Ln, 9))]
    for kw in bad:
        with pytest.raises(ValueError):
            m.compute_trajectory(*args, **kw)
        with pytest.raises(ValueError):                       # and through forward(run_inference=True, ...)
            m(None, *args, run_inference=True, **kw)


def test_sched_c_abi_argument_validation_without_gpu():
    """a3d_dn_persist_sched / a3d_dn_tail_sched / a3d_ddpm_step_sched reject bad arguments on the host before any launch, with the
    error code and the entry's own name in a3d_last_error_string; a3d_dn_persist still answers under its own name."""
    a3d = load_pkg()
    lib = a3d.lib.load()
    L = a3d.lib
    d = ctypes.c_void_p(64)                                                          # aligned, never dereferenced
    hp = L.DnHeadParams(enc_w0=64, enc_w1=64)
    tp = L.DnTailParams(pos_w0=64, rot_w0=64, coef_pos=64, coef_rot=64)

    def persist(B=2, Ln=16, D=9, E=120, H=8, S=100, Sp=128, nsplit=2, row_first=0, nsteps=10, n_rows=10, last=1, head=hp, tail=tp, kvx=None,
                sync=d, stacks=(4, 2, 2)):
        return lib.a3d_dn_persist_sched(d, stacks[0], stacks[1], stacks[2], ctypes.byref(head), ctypes.byref(tail), d, d, d, kvx, d, sync,
                                        B, Ln, D, E, H, S, Sp, nsplit, row_first, nsteps, n_rows, last, None)

    def refused(rc, name):
        assert rc == -22, name
        assert name.encode() in lib.a3d_last_error_string(), lib.a3d_last_error_string()

    refused(persist(Ln=65), "a3d_dn_persist_sched")                                  # L > 64
    refused(persist(E=121), "a3d_dn_persist_sched")                                  # E != 15 H
    refused(persist(B=0), "a3d_dn_persist_sched")
    refused(persist(nsteps=0), "a3d_dn_persist_sched")
    refused(persist(nsteps=11), "a3d_dn_persist_sched")                              # more steps than table rows
    refused(persist(row_first=1), "a3d_dn_persist_sched")                            # rows 1 .. 10 of a 10-row table
    refused(persist(row_first=-1), "a3d_dn_persist_sched")
    refused(persist(n_rows=0, nsteps=1), "a3d_dn_persist_sched")
    refused(persist(last=2), "a3d_dn_persist_sched")                                 # the terminal flag is 0 or 1
    refused(persist(last=-1), "a3d_dn_persist_sched")
    refused(persist(Sp=100), "a3d_dn_persist_sched")                                 # Sp % 64
    refused(persist(nsplit=0), "a3d_dn_persist_sched")
    refused(persist(D=17), "a3d_dn_persist_sched")
    refused(persist(Ln=50), "a3d_dn_persist_sched")                                  # four row tiles need the kvx exchange buffer
    refused(persist(sync=None), "a3d_dn_persist_sched")
    refused(persist(stacks=(4, 0, 2)), "a3d_dn_persist_sched")
    refused(persist(tail=L.DnTailParams(pos_w0=64, rot_w0=64, coef_pos=64)), "a3d_dn_persist_sched")      # no rotation table
    refused(persist(tail=L.DnTailParams(pos_w0=64, rot_w0=64, coef_pos=64, coef_rot=64, cond_mask=64)), "a3d_dn_persist_sched")
    # the parent entry keeps its own name and its own step check (t_first >= nsteps - 1)
    rc = lib.a3d_dn_persist(d, 4, 2, 2, ctypes.byref(hp), ctypes.byref(tp), d, d, d, None, d, d, 2, 16, 9, 120, 8, 100, 128, 2, 3, 10, None)
    assert rc == -22 and b"a3d_dn_persist:" in lib.a3d_last_error_string() and b"from t=3" in lib.a3d_last_error_string()

    def tail(B=2, Ln=16, D=9, E=120, row=0, terminal=0, p=tp):
        return lib.a3d_dn_tail_sched(d, d, d, D, ctypes.byref(p), d, B, Ln, E, row, terminal, None)
    refused(tail(row=-1), "a3d_dn_tail_sched")
    refused(tail(terminal=2), "a3d_dn_tail_sched")
    refused(tail(Ln=17), "a3d_dn_tail_sched")
    refused(tail(D=3), "a3d_dn_tail_sched")
    refused(tail(p=L.DnTailParams(pos_w0=64, rot_w0=64)), "a3d_dn_tail_sched")
    assert lib.a3d_dn_tail(d, d, d, 9, ctypes.byref(tp), d, 2, 16, 120, -1, None) == -22 and b"a3d_dn_tail:" in lib.a3d_last_error_string()

    def step(rows=4, D=9, row=0, terminal=0, out=d, mask=None, cond=None):
        return lib.a3d_ddpm_step_sched(d, d, None, cond, mask, d, d, out, rows, D, 3, row, terminal, None)
    refused(step(row=-1), "a3d_ddpm_step_sched")
    refused(step(terminal=3), "a3d_ddpm_step_sched")
    refused(step(rows=0), "a3d_ddpm_step_sched")
    refused(step(out=None), "a3d_ddpm_step_sched")
    refused(step(mask=d), "a3d_ddpm_step_sched")                                     # a mask without the data to in-paint
    # sync sizing follows the number of executed steps
    n10, n100 = lib.a3d_dn_persist_sync_ints(64, 16, 8, 10), lib.a3d_dn_persist_sync_ints(64, 16, 8, 100)
    assert 0 < n10 < n100 and n100 - n10 >= 90 * 8 * 64
