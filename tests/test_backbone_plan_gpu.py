"""The frozen backbone launches what nn.backbone_plan predicts: the entry names one run_frozen_backbone call issues, recorded at
lib.call, equal the plan's list in order, under every switch value (tests/test_backbone_plan_cpu.py pins the plan itself)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (case, module switches, BatchNorm training mode, raw images through the fused stem)
CASES = [
    ("default", {}, True, False),
    ("residual off", dict(FUSED_CONV3_RESIDUAL=False), True, False),
    ("gram", dict(FUSED_CONV3_RESIDUAL="gram"), True, False),
    ("downsample fold off", dict(FOLD_DOWNSAMPLE_BN=False), True, False),
    ("both convolution switches off", dict(FUSED_CONV1X1=False, FUSED_CONV3X3=False), True, False),
    ("eval mode", {}, False, False),
    ("raw images", {}, True, True),
]


@pytest.fixture(scope="module")
def backbone(a3d, dev):
    torch.manual_seed(0)
    return a3d.nn.SyntheticCLIPResNet50().to(dev).train()


def launches(a3d, fn):
    """Entry names of the launches fn() issues, in order (lib.call wrapped as in test_sampler_schedule_gpu.py)."""
    seen, call = [], a3d.lib.call
    a3d.ops.L.call = lambda entry, *args: (seen.append(entry), call(entry, *args))[1]
    try:
        result = fn()
    finally:
        a3d.ops.L.call = call
    return seen, result


@pytest.mark.parametrize("name,switches,train,raw", CASES, ids=[c[0] for c in CASES])
def test_backbone_launches_what_the_plan_predicts(a3d, dev, backbone, monkeypatch, name, switches, train, raw):
    N = a3d.nn
    torch.manual_seed(1)
    x = torch.rand(2, 3, 128, 128, device=dev)
    normalize = N.ClipNormalize().to(dev) if raw else None
    for k, v in switches.items():
        monkeypatch.setattr(N, k, v)
    backbone.train(train)
    try:
        want = N.backbone_plan(backbone, 2, 128, 128, fused_stem=None if raw else False).launches()
        with torch.no_grad():
            seen, maps = launches(a3d, lambda: N.run_frozen_backbone(backbone, x, torch.bfloat16, normalize=normalize))
    finally:
        backbone.train(True)
    torch.cuda.synchronize()
    assert seen == want
    assert (seen[0] == "a3d_stem_conv_bn_fwd") == raw
    assert list(maps) == ["res1", "res2", "res3", "res4", "res5"] and all(torch.isfinite(v).all() for v in maps.values())


def test_backbone_writes_the_five_maps_into_out_buffers(a3d, dev, backbone):
    N = a3d.nn
    torch.manual_seed(2)
    x = torch.rand(2, 3, 128, 128, device=dev)
    with torch.no_grad():
        first = N.run_frozen_backbone(backbone, x, torch.bfloat16, keep_dtype=True)
        bufs = {k: torch.full_like(v, float("nan")) for k, v in first.items()}
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        seen, got = launches(a3d, lambda: N.run_frozen_backbone(backbone, x, torch.bfloat16, keep_dtype=True, out=bufs))
    torch.cuda.synchronize()
    assert seen == N.backbone_plan(backbone, 2, 128, 128, fused_stem=False).launches()
    assert sorted(ptrs) == ["res1", "res2", "res3", "res4", "res5"]
    for k in ptrs:
        assert got[k].data_ptr() == ptrs[k] and bufs[k].data_ptr() == ptrs[k], k
        assert got[k].shape == first[k].shape and torch.isfinite(bufs[k]).all(), k       # written in place: no NaN of the fill is left
