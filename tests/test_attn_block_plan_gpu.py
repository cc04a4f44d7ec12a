"""An attention block launches what ops.attn_block_plan predicts: the entry names one ops.attn_block forward and one backward issue,
recorded at lib.call, equal launches_forward() / launches_backward() in order, for every case of tests/attn_block_cases.py (the three
modes, each under every switch value of tests/test_attn_block_plan_cpu.py that applies to it; that test pins the plan itself).  What
is recorded behind the block's own backward -- the sink gate's two GEMMs for a parked block, the reduce queue's flush -- is listed
per case."""
import math

import pytest
import torch

import attn_block_cases as AC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", AC.CASES, ids=[c["name"] for c in AC.CASES])
def test_attn_block_launches_what_the_plan_predicts(a3d, dev, monkeypatch, c):
    O = a3d.ops
    for k, v in c["switches"].items():
        assert hasattr(O, k)
        monkeypatch.setattr(O, k, v)
    monkeypatch.setattr(O.ReduceQueue, "current", None)
    r = AC.run_case(a3d, dev, c)
    route = O.attn_block_plan(**r["plan"])
    assert r["fwd"] == route.launches_forward()
    assert all(torch.isfinite(t).all() for t in r["tensors"].values())
    if c["grad"]:
        assert r["bwd"] == route.launches_backward() + c["after"]
    else:
        assert route.core_bwd is None and route.launches_backward() == []


@pytest.fixture(scope="module")
def cached_pair(a3d, dev):
    """{fused: (kv_cache_build launches, attn_block_cached launches, y)}: both projection routes, computed once"""
    old, out = a3d.ops.FUSED_PROJ, {}
    try:
        for fused in (True, False):
            a3d.ops.FUSED_PROJ = fused
            out[fused] = AC.run_cached(a3d, dev)
    finally:
        a3d.ops.FUSED_PROJ = old
    return out


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_cached_pair_launches_what_its_two_groups_predict(cached_pair, fused):
    """kv_cache_build is the (k, v) group and attn_block_cached the q group of mode "kv" in the bf16 family, forward only."""
    build, block, y = cached_pair[fused]
    tail = ["a3d_attn_fwd", "a3d_linear_fwd", "a3d_add_layernorm_fwd"]
    if fused:
        assert build == ["a3d_proj_rope_split"] and block == ["a3d_proj_rope_split"] + tail
    else:
        assert build == ["a3d_linear_fwd", "a3d_rope_split", "a3d_rope_split"]
        assert block == ["a3d_linear_fwd", "a3d_rope_split"] + tail
    assert torch.isfinite(y).all()


def test_cached_pair_fused_and_unfused_outputs_agree(cached_pair):
    """The relation asserted is the one the tree before the table shows, which is NOT bit-identity: at B=2, Lq=8, S=70, E=120, H=8 its
    fused and unfused outputs differ by at most 9.5e-7 where max |y| = 6.35, which is 2 ulp of fp32 at that magnitude
    (cached_pair_fused_vs_unfused in profiles/attn_block_plan_equivalence.json, where this tree's two outputs carry the parent's
    digests).  Asserted: max |dy| <= 4 ulp of max |y| -- the recorded relation with a factor of two of headroom (the kernels are deterministic:
    both trees give the same two digests), two orders of magnitude below the operand writers' own 2e-5 agreement bound."""
    y_f, y_u = cached_pair[True][2], cached_pair[False][2]
    err, scale = (y_f - y_u).abs().max().item(), y_u.abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(scale)) - 23)
    print("cached pair, fused against unfused: max |dy| = %.3e = %.1f ulp of max |y| = %.3e" % (err, err / ulp, scale))
    assert err <= 4 * ulp
