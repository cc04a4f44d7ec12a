"""diffusion.sampler_plan on the host: which launches serve a compute_trajectory call, decided from the shapes, the module switches
and the CU count alone (no GPU).  The expected column is written from the rule, not produced by the function:

  fused kernels serve the shape   E <= 128, D <= 16, min(L, 16) D <= 160, fused not False (default: FUSED_DENOISE)
  persistent sampler fits         DN_PERSIST, 2 * trajectories * ceil(L / 16) + 16 <= CUs, H <= 8, L <= 64
  multi-round head                -> "multi-round", whatever else holds
  serve and fit                   -> persistent: a3d_dn_persist / _sched (a schedule) / _group (num_samples, on the per-scene cache;
                                     the full chain then runs as the K = T schedule with its noise table flipped)
  serve, not fit, L <= 16         -> per-phase fused launches
  otherwise                       -> op-by-op
"""
from conftest import load_pkg

T = 100
PERSIST, SCHED, GROUP = ("persistent (a3d_dn_persist%s)" % s for s in ("", "_sched", "_group"))
PHASE, OPS, MULTI = "per-phase fused launches", "op-by-op", "multi-round"

# (what the row pins, keyword changes to the base call, module switches, (last_sampler_path, group, flipped noise))
BASE = dict(B=2, G=None, Ln=8, D=9, E=120, H=8, T=T, cus=256)
ROWS = [
    ("base call", {}, {}, (PERSIST, False, False)),
    # 1: one row tile is the most the per-phase launches serve
    ("L = 16 without the persistent sampler", dict(Ln=16), dict(DN_PERSIST=False), (PHASE, False, False)),
    ("L = 17 without the persistent sampler", dict(Ln=17), dict(DN_PERSIST=False), (OPS, False, False)),
    # 2: four row tiles are the most the persistent sampler serves
    ("L = 64", dict(Ln=64), {}, (PERSIST, False, False)),
    ("L = 65", dict(Ln=65), {}, (OPS, False, False)),
    # 3: co-residency at 256 CUs -- 2 * 120 * 1 + 16 = 2 * 60 * 2 + 16 = 256
    ("L = 8 at the CU limit", dict(B=120), {}, (PERSIST, False, False)),
    ("L = 8, one trajectory above the CU limit", dict(B=121), {}, (PHASE, False, False)),
    ("L = 8, one CU short", dict(B=120, cus=255), {}, (PHASE, False, False)),
    ("L = 20 at the CU limit", dict(B=60, Ln=20), {}, (PERSIST, False, False)),
    ("L = 20, one trajectory above the CU limit", dict(B=61, Ln=20), {}, (OPS, False, False)),
    ("L = 20, one CU short", dict(B=60, Ln=20, cus=255), {}, (OPS, False, False)),
    # 4: sixteen heads
    ("H = 16, L = 8", dict(H=16), {}, (PHASE, False, False)),
    ("H = 16, L = 20", dict(H=16, Ln=20), {}, (OPS, False, False)),
    # 5: the trajectory tile of the fused kernels holds 160 floats
    ("D = 10, L = 16 (160 floats)", dict(D=10, Ln=16), {}, (PERSIST, False, False)),
    ("D = 11, L = 16 (176 floats)", dict(D=11, Ln=16), {}, (OPS, False, False)),
    ("D = 11, L = 14 (154 floats)", dict(D=11, Ln=14), {}, (PERSIST, False, False)),
    ("D = 17", dict(D=17, Ln=4), {}, (OPS, False, False)),
    ("E = 132", dict(E=132), {}, (OPS, False, False)),
    # 6: a multi-round head
    ("multi-round", dict(multi=True), {}, (MULTI, False, False)),
    ("multi-round, fused=True", dict(multi=True, fused=True), {}, (MULTI, False, False)),
    ("multi-round, fused=False", dict(multi=True, fused=False), {}, (MULTI, False, False)),
    ("multi-round, num_samples", dict(multi=True, G=2), {}, (MULTI, False, False)),
    # 7: the fused argument and its default
    ("fused=False", dict(fused=False), {}, (OPS, False, False)),
    ("FUSED_DENOISE off", {}, dict(FUSED_DENOISE=False), (OPS, False, False)),
    ("FUSED_DENOISE off, fused=True", dict(fused=True), dict(FUSED_DENOISE=False), (PERSIST, False, False)),
    # 8: candidate groups
    ("G = 2, full chain", dict(G=2), {}, (GROUP, True, True)),
    ("G = 1, full chain", dict(G=1), {}, (GROUP, True, True)),
    ("G = 2, K = 10", dict(G=2, num_inference_steps=10), {}, (GROUP, True, False)),
    ("G = 2 at the CU limit", dict(B=60, G=2), {}, (GROUP, True, True)),
    # 9: candidates the persistent sampler cannot serve run on the expanded context
    ("G = 2 above the CU limit", dict(B=61, G=2), {}, (PHASE, False, False)),
    ("G = 2 above the CU limit, L = 20", dict(B=31, G=2, Ln=20), {}, (OPS, False, False)),
    ("G = 2 without the persistent sampler", dict(G=2), dict(DN_PERSIST=False), (PHASE, False, False)),
    ("G = 2, fused=False", dict(G=2, fused=False), {}, (OPS, False, False)),
    # 10: truncation and schedules
    ("full chain truncated to 7 steps", dict(n_steps=7), {}, (PERSIST, False, False)),
    ("K = 10", dict(num_inference_steps=10), {}, (SCHED, False, False)),
    ("ddim, eta = 0.5, K = T", dict(scheduler="ddim", eta=0.5), {}, (SCHED, False, False)),
    ("K = 10 without the persistent sampler", dict(num_inference_steps=10), dict(DN_PERSIST=False), (PHASE, False, False)),
]


def test_sampler_plan_table(monkeypatch):
    D = load_pkg().diffusion
    for name, change, switches, want in ROWS:
        with monkeypatch.context() as mp:
            for k, v in switches.items():
                mp.setattr(D, k, v)                         # read at call time
            plan = D.sampler_plan(**dict(BASE, **change))
        assert (plan.label, plan.group, plan.flip_noise) == want, name
        assert plan.path == {PERSIST: "persistent", SCHED: "persistent", GROUP: "persistent", PHASE: "per-phase", OPS: "op-by-op",
                             MULTI: "multi-round"}[want[0]], name
    full = tuple(range(T - 1, -1, -1))
    # the step list: the full chain by timestep (truncated: its first steps, still consecutive) ...
    plan = D.sampler_plan(**BASE)
    assert (plan.scheduled, plan.K, plan.steps) == (False, None, full)
    assert D.sampler_plan(**BASE, n_steps=7).steps == full[:7]
    # ... the K leading-spaced timesteps of a schedule ...
    plan = D.sampler_plan(**BASE, num_inference_steps=10, n_steps=4)
    assert (plan.scheduled, plan.K, plan.steps) == (True, 10, (90, 80, 70, 60))
    # ... and for candidate groups the full chain as the K = T schedule
    plan = D.sampler_plan(**dict(BASE, G=2))
    assert (plan.scheduled, plan.K, plan.steps) == (True, T, full)
    plan = D.sampler_plan(**dict(BASE, B=61, G=2))
    assert (plan.scheduled, plan.K, plan.steps) == (False, None, full)
    assert D.persist_fits(120, 8, 8, 256) and not D.persist_fits(121, 8, 8, 256) and not D.persist_fits(1, 65, 8, 256)
