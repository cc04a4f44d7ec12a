"""The fused denoise kernels of csrc/denoise.hip, one launch at a time through lib.py's ctypes binding, against the float64 references
and the bounds of tests/denoise_ref.py (right, fair and with teeth: tests/test_denoise_ref_cpu.py).  No tolerance is chosen here.

  a3d_dn_cross   the partials Op / Mp read back from the workspace, combined in float64 by the test and held against the DERIVED bound
                 (attn16_core_ref's adaptive forward bound + the error of the kernel's own q).  Case table denoise_ref.CROSS_CASES:
                 key counts / padding / splits that give every wave-range length 0-5, 8, 9, 32, 33, dead ranges and ranges that run
                 into a dead half; E = 30 / 60 / 90 / 120 (B H = 12, 18, 24: the XCD grid rounding and its early-return workgroups);
                 L = 1, 7, 15, 16; D = 3, 9, 10; freq / mod / sem NULL; the score profiles that drive the lazy maximum, the dominance
                 threshold and the fp16 floor; Kf / Vt rows [S, Sp) filled with finite garbage must give the same bits as zero padding.
                 Also: Mp is -inf exactly for the splits without a valid key, rows >= L are finite, the workspace's guard bands are
                 untouched, a second launch gives the same bits.
  a3d_dn_rest    x_out against the twin rule err(kernel) <= max(2^-20, 4 err(fp32 twin)) on SYNTHETIC partials (splits at -inf, a head
                 with every split at -inf); E / H / F = 30/2/30 ... 120/8/512; L = 1, 7, 16; nsplit 1, 3, 8; the four key masks; no
                 self-attention block; no FFN; D = 9, 10; every weight matrix at a 4-byte aligned address.
  a3d_dn_head    E = 30 / 60 / 120, D = 4 / 9 / 16, L = 1 / 16, S_lang = 1, 53 and the largest accepted, no instruction branch, B = 3.
  a3d_dn_tail / a3d_dn_tail_sched   E = 30 / 120, D = 4 / 9 / 16, L = 1 / 16, in-painting scattered / whole rows / none, noise NULL or
                 not, rows 0 / T - 1, terminal steps; about a third of |x0| exceeds 1.
  The rest / head / tail tables once more under A3D_DN_THREADS=256 (the 4-wave workgroups; the switch is a static) in ONE fresh child
  process.

Every test prints [parity] lines: the case, the error, the bound or the twin's error, and their ratio.
"""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

import attn16_core_ref as C
import denoise_ref as DR

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
GUARD, POISON = 64, 0xA5


class _Guarded:
    """A device buffer of `shape` inside a poisoned allocation."""
    def __init__(self, shape, dtype, dev):
        n = 1
        for s in shape:
            n *= s
        self.full = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.full.view(torch.uint8).fill_(POISON)
        self.t = self.full[GUARD:GUARD + n].view(*shape)
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        b = self.full.view(torch.uint8)
        w = self.full.element_size()
        return bool((b[:GUARD * w] == POISON).all() and (b[(GUARD + self.n) * w:] == POISON).all())


class _Pool:
    """Device copies of a case's tensors, kept alive for the launch; misalign: the copy starts 4 bytes past a 16-byte boundary."""
    def __init__(self, dev):
        self.dev, self.keep = dev, []

    def __call__(self, t, misalign=False):
        if t is None:
            return None
        t = t.contiguous()
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        off = 1 if misalign else 0
        buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=self.dev)
        d = buf[off:off + t.numel()].view(t.shape)
        d.copy_(t)
        assert buf.data_ptr() % 16 == 0 and d.data_ptr() % 16 == (4 if misalign else 0)
        self.keep.append(buf)
        return d.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ launches
def launch_cross(a3d, dev, x, Kf=None, Vt=None):
    """One a3d_dn_cross launch -> (Op [ns][B][H][16][16], Mp [ns][B][H][16]) on the CPU."""
    L = a3d.lib
    d = _Pool(dev)
    p = L.DnCrossParams(sem=d(x.sem), mod=d(x.mod), q_w=d(x.q_w), q_b=d(x.q_b), freq=d(x.freq), Kf=d(x.Kf if Kf is None else Kf),
                        Vt=d(x.Vt if Vt is None else Vt))
    n = L.load().a3d_dn_cross_ws_floats(x.B, x.H, x.ns)
    assert n == x.ns * x.B * x.H * 16 * 17
    ws = _Guarded((n,), F32, dev)
    L.call("a3d_dn_cross", d(x.x), d(x.traj), x.D, ctypes.byref(p), ws.ptr(), x.B, x.L, x.E, x.H, x.S, x.Sp, x.ns, L.stream())
    torch.cuda.synchronize()
    assert ws.guards_intact(), f"{x.case.name}: bytes outside the workspace were written"
    w = ws.t.cpu()
    no = x.ns * x.B * x.H * 256
    return w[:no].view(x.ns, x.B, x.H, 16, 16), w[no:].view(x.ns, x.B, x.H, 16)


def launch_rest(a3d, dev, x):
    L = a3d.lib
    c, p = x.case, x.p
    d = _Pool(dev)
    mis = not c.walign
    sa = lambda t, m=False: d(t, m) if c.sa else None
    ff = lambda t, m=False: d(t, m) if c.ffn else None
    rp = L.DnRestParams(c_out_w=d(p.c_out_w, mis), c_out_b=d(p.c_out_b), c_ln_g=d(p.c_ln_g), c_ln_b=d(p.c_ln_b), sem=d(x.sem),
                        s_mod=sa(p.s_mod), s_in_w=sa(p.s_in_w, mis), s_in_b=sa(p.s_in_b), s_out_w=sa(p.s_out_w, mis), s_out_b=sa(p.s_out_b),
                        s_ln_g=sa(p.s_ln_g), s_ln_b=sa(p.s_ln_b), freq=d(x.freq), kmask=d(x.kmask), f_mod=ff(p.f_mod),
                        f_w1=ff(p.f_w1, mis), f_b1=ff(p.f_b1), f_w2=ff(p.f_w2, mis), f_b2=ff(p.f_b2), f_ln_g=ff(p.f_ln_g),
                        f_ln_b=ff(p.f_ln_b), F=x.F)
    ws = d(torch.cat((x.Op.flatten(), x.Mp.flatten())))
    out = _Guarded((x.B, x.L, x.E), F32, dev)
    L.call("a3d_dn_rest", d(x.x), d(x.traj), x.D, ws, ctypes.byref(rp), out.ptr(), x.B, x.L, x.E, x.H, x.ns, L.stream())
    torch.cuda.synchronize()
    assert out.guards_intact(), f"{c.name}: bytes outside x_out were written"
    return out.t.cpu()


def launch_head(a3d, dev, x):
    L = a3d.lib
    p = x.p
    d = _Pool(dev)
    hp = L.DnHeadParams(enc_w0=d(p.enc_w0), enc_b0=d(p.enc_b0), enc_w1=d(p.enc_w1), enc_b1=d(p.enc_b1), sem=d(p.sem), lang_kv=d(x.lang_kv),
                        S_lang=x.S_lang or 0, q_w=d(p.q_w), q_b=d(p.q_b), out_w=d(p.out_w), out_b=d(p.out_b), ln_g=d(p.ln_g), ln_b=d(p.ln_b))
    out = _Guarded((x.B, x.L, x.E), F32, dev)
    L.call("a3d_dn_head", d(x.traj), x.D, ctypes.byref(hp), out.ptr(), x.B, x.L, x.E, x.H, L.stream())
    torch.cuda.synchronize()
    assert out.guards_intact(), f"{x.case.name}: bytes outside x_out were written"
    return out.t.cpu()


def launch_tail(a3d, dev, x):
    L = a3d.lib
    c, p = x.case, x.p
    d = _Pool(dev)
    tp = L.DnTailParams(pos_w0=d(p.pos_w0), pos_b0=d(p.pos_b0), pos_w1=d(p.pos_w1), pos_b1=d(p.pos_b1), rot_w0=d(p.rot_w0),
                        rot_b0=d(p.rot_b0), rot_w1=d(p.rot_w1), rot_b1=d(p.rot_b1), noise=d(p.noise), cond_data=d(p.cond_data),
                        cond_mask=d(p.cond_mask), coef_pos=d(p.coef_pos), coef_rot=d(p.coef_rot))
    out = _Guarded((x.B, x.L, x.D), F32, dev)
    args = (d(x.pos_feats), d(x.rot_feats), d(x.traj), x.D, ctypes.byref(tp), out.ptr(), x.B, x.L, x.E)
    if c.entry == "tail":
        L.call("a3d_dn_tail", *args, c.row, L.stream())
    else:
        L.call("a3d_dn_tail_sched", *args, c.row, c.terminal, L.stream())
    torch.cuda.synchronize()
    assert out.guards_intact(), f"{c.name}: bytes outside traj_out were written"
    return out.t.cpu()


LAUNCH = {"rest": launch_rest, "head": launch_head, "tail": launch_tail}


def check_dense(a3d, dev, kind, name, tag=""):
    """One launch of a dense-chain case against the twin rule; returns err / limit."""
    x, ref, et = DR.prepared(kind, name)
    got = LAUNCH[kind](a3d, dev, x)
    e, lim = DR.rel_err(got, ref), DR.twin_limit(et)
    print(f"[parity] dn_{kind} {name}{tag}: err={e:.3e} twin={et:.3e} limit=max(2^-20, 4 twin)={lim:.3e} err/limit={e / lim:.3f} "
          f"err/twin={e / et:.2f}")
    assert torch.isfinite(got).all(), (kind, name)
    return e / lim, got


# ------------------------------------------------------------------------------------------------ cross attention
@pytest.mark.parametrize("name", [c.name for c in DR.CROSS_CASES if not c.garbage])
def test_cross_partials_within_the_derived_bound(a3d, dev, name):
    x = DR.build_cross(name)
    r = DR.cross_reference(x)
    Op, Mp = launch_cross(a3d, dev, x)
    assert torch.isfinite(Op).all() and not torch.isnan(Mp).any() and not (Mp == math.inf).any(), name
    # a split is at -inf exactly when none of its four waves' ranges begins below S
    rng = DR.wave_ranges(x.Sp, x.ns)
    for s in range(x.ns):
        empty = not any(he > hb and hb * 32 < x.S for hb, he in rng[4 * s:4 * s + 4])
        assert bool(torch.isinf(Mp[s]).all()) == empty and bool(torch.isinf(Mp[s]).any()) == empty, (name, s, empty)
        if empty:
            assert (Op[s] == 0).all(), (name, s)
    O = DR.combine_partials(Op, Mp)
    assert torch.isfinite(O).all(), name                                   # rows >= L included
    err = O[:, :, :x.L] - r.O
    ratio, ratio0 = C.ratio(err, r.bound), C.ratio(err, r.bound_no_extra)
    print(f"[parity] dn_cross {name} E={x.E} L={x.L} S={x.S} Sp={x.Sp} nsplit={x.ns}: max(err/bound)={ratio:.3f} "
          f"(max_abs_err {err.abs().max():.2e} of {r.O.abs().max():.2e}; against the bound without the q term {ratio0:.3f})")
    assert ratio <= 1.0, (name, ratio)
    Op2, Mp2 = launch_cross(a3d, dev, x)
    assert torch.equal(_bits(Op), _bits(Op2)) and torch.equal(_bits(Mp), _bits(Mp2)), f"{name}: partials differ between two launches"


def test_cross_padding_is_masked_by_position(a3d, dev):
    x = DR.build_cross("pad_garbage_s65_sp256")
    r = DR.cross_reference(x)
    Op, Mp = launch_cross(a3d, dev, x)
    Kf, Vt = DR.garbage_operands(x)
    assert torch.equal(Kf[:, :, :x.S], x.Kf[:, :, :x.S]) and not torch.equal(Kf, x.Kf) and torch.isfinite(Kf.float()).all()
    Opg, Mpg = launch_cross(a3d, dev, x, Kf, Vt)
    ratio = C.ratio(DR.combine_partials(Op, Mp)[:, :, :x.L] - r.O, r.bound)
    print(f"[parity] dn_cross pad_garbage_s65_sp256: max(err/bound)={ratio:.3f}; garbage rows [S, Sp): partials "
          f"{'identical' if torch.equal(_bits(Op), _bits(Opg)) else 'DIFFER'}")
    assert ratio <= 1.0
    assert torch.equal(_bits(Op), _bits(Opg)) and torch.equal(_bits(Mp), _bits(Mpg)), "rows [S, Sp) of Kf / Vt reached the partials"


# ------------------------------------------------------------------------------------------------ dense chains
@pytest.mark.parametrize("name", [c.name for c in DR.REST_CASES])
def test_rest_within_the_twin_rule(a3d, dev, name):
    r, got = check_dense(a3d, dev, "rest", name)
    assert r <= 1.0, (name, r)
    assert torch.equal(_bits(got), _bits(launch_rest(a3d, dev, DR.prepared("rest", name)[0]))), f"{name}: x_out differs between two launches"


@pytest.mark.parametrize("name", [c.name for c in DR.HEAD_CASES])
def test_head_within_the_twin_rule(a3d, dev, name):
    r, _ = check_dense(a3d, dev, "head", name)
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("name", [c.name for c in DR.TAIL_CASES])
def test_tail_within_the_twin_rule(a3d, dev, name):
    r, got = check_dense(a3d, dev, "tail", name)
    assert r <= 1.0, (name, r)
    x, ref, _ = DR.prepared("tail", name)
    if x.p.cond_mask is not None and x.terminal:                           # the in-painted elements of a terminal step are copies
        assert torch.equal(got[x.p.cond_mask], x.p.cond_data[x.p.cond_mask]), name


N_DENSE = len(DR.REST_CASES) + len(DR.HEAD_CASES) + len(DR.TAIL_CASES)


def _threads256_child():
    """Body of the child process: the rest / head / tail tables under whatever A3D_DN_THREADS the environment holds."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import importlib
    a3d = importlib.import_module("act3d-chained-diffuser_amd")
    dev = torch.device("cuda:0")
    worst = 0.0
    for kind, cases in (("rest", DR.REST_CASES), ("head", DR.HEAD_CASES), ("tail", DR.TAIL_CASES)):
        for c in cases:
            r, _ = check_dense(a3d, dev, kind, c.name, " [A3D_DN_THREADS=256]")
            worst = max(worst, r)
    assert worst <= 1.0, worst
    print(f"dn-child ok {N_DENSE} cases worst {worst:.3f}")


def test_four_wave_workgroups_in_a_fresh_process(dev):
    """A3D_DN_THREADS=256 is read once into a static: the 4-wave variant of the per-sample kernels runs in a process of its own."""
    env = dict(os.environ)
    env["A3D_DN_THREADS"] = "256"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "threads256-child"], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"dn-child ok {N_DENSE} cases" in p.stdout


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "threads256-child":
    _threads256_child()
