"""nn.backbone_plan on the host: which launches serve each of the 16 bottlenecks of the frozen backbone, decided from the module's
structure, the module switches and the library's shape queries alone (no GPU, nothing launched).  The expected table is written out
by hand from the rules of the forward it replaces, not produced by the function:

  1x1 on the own GEMM            FUSED_CONV1X1 and a3d_conv1x1_streams(K, N): the resident-weight kernel (K in {64, 128, 256} within 96 KB
                                 of LDS) or, with a3d_conv1x1_deep_mode on, the deep GEMM -- which besides layers 3 - 4 serves layer 2's
                                 512 -> 128 conv1 of the blocks [1] .. [3] and its 256 -> 512 downsample convolution
  3x3 fused                      FUSED_CONV3X3 and a3d_conv3x3_serves: <= 64 channels, H % 8 == 0, W % 32 == 0 -- the stem and layer 1
  bn2                            rides on conv3's operand load where the block has no pool and conv3 is an own kernel; stride-2 blocks
                                 normalise and pool in one a3d_bn_apply_pool2
  conv3 residual route           FUSED_CONV3_RESIDUAL, a3d_conv1x1_bn_residual_serves (64 -> 256, 128 -> 512), and the NEXT block's
                                 downsample does not want the pooled output (that one comes from the final a3d_bn_apply_pool2, which
                                 needs the raw conv3 map)
  downsample BatchNorm           folded into the final apply / epilogue with FOLD_DOWNSAMPLE_BN, except under a final a3d_bn_apply_pool2
"""
import collections

import pytest

from conftest import load_pkg

COLS = ("name", "conv1", "stats1", "conv2", "stats2", "bn2", "conv3", "stats3", "ds_input", "ds_conv", "ds_stats", "ds_bn", "final", "writes")
G, EPI, LIB, BS = "gemm", "epilogue", "library", "bn_stats"
PRO, P2, APPLY = "conv3_prologue", "bn_apply_pool2", "bn_apply"
RES, SP, CE = "residual", "stats_pass", "conv3_epilogue"
NO_DS = (None, None, None, None)
# SyntheticCLIPResNet50().train(), default switches, 4 x 3 x 128 x 128: layer 1 at 32 x 32, layer 2 at 16 x 16, 3 at 8 x 8, 4 at 4 x 4
DEFAULT = [
    # name        conv1      conv2 (bn1)     bn2   conv3 + bn3's statistics  downsample: input, conv, stats, bn         final  writes
    ("layer1[0]", G, EPI, "fused", EPI, PRO, RES, SP, "identity", G, EPI, "folded", CE, None),
    ("layer1[1]", G, EPI, "fused", EPI, PRO, RES, SP, *NO_DS, CE, None),
    ("layer1[2]", G, EPI, "fused", EPI, PRO, G, EPI, *NO_DS, P2, "res2"),           # layer2[0]'s downsample wants the pooled map
    ("layer2[0]", G, EPI, LIB, BS, P2, RES, SP, "producer_pooled", G, EPI, "folded", CE, None),      # no prologue: input normalised and pooled
    ("layer2[1]", G, EPI, LIB, BS, PRO, RES, SP, *NO_DS, CE, None),
    ("layer2[2]", G, EPI, LIB, BS, PRO, RES, SP, *NO_DS, CE, None),
    ("layer2[3]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, P2, "res3"),
    ("layer3[0]", G, EPI, LIB, BS, P2, G, EPI, "producer_pooled", G, EPI, "folded", APPLY, None),
    ("layer3[1]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, APPLY, None),
    ("layer3[2]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, APPLY, None),
    ("layer3[3]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, APPLY, None),
    ("layer3[4]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, APPLY, None),
    ("layer3[5]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, P2, "res4"),
    ("layer4[0]", G, EPI, LIB, BS, P2, G, EPI, "producer_pooled", G, EPI, "folded", APPLY, None),
    ("layer4[1]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, APPLY, None),
    ("layer4[2]", G, EPI, LIB, BS, PRO, G, EPI, *NO_DS, APPLY, "res5"),
]
DEFAULT_STEM = ("stem_conv", "fused", "fused", (EPI, EPI, EPI), P2)
RESIDUAL_BLOCKS = ["layer1[0]", "layer1[1]", "layer2[0]", "layer2[1]", "layer2[2]"]
FIRST = ["layer1[0]", "layer2[0]", "layer3[0]", "layer4[0]"]


def table(change=lambda row: {}):
    """DEFAULT with the columns change(row as a dict) names replaced"""
    rows = []
    for row in DEFAULT:
        d = dict(zip(COLS, row))
        d.update(change(dict(d)))
        rows.append(tuple(d[c] for c in COLS))
    return rows


def library_1x1(d, deep_only):
    """the row with its 1x1 convolutions on the library: all of them, or (deep_only) those only the deep GEMM serves"""
    deep = d["name"][:6] in ("layer3", "layer4")
    c = {}
    if not deep_only or deep or d["name"] in ("layer2[1]", "layer2[2]", "layer2[3]"):          # 512 -> 128 and deeper: K > 256
        c.update(conv1=LIB, stats1=BS)
    if not deep_only or deep:
        c.update(conv3=LIB, stats3=BS, bn2=P2 if d["bn2"] == P2 else APPLY)
        if d["conv3"] == RES:                                                                # no residual route without the own GEMM
            c.update(final=APPLY)
    if d["ds_input"] is not None and (not deep_only or deep or d["name"] == "layer2[0]"):    # 256 -> 512: its weight block exceeds 96 KB
        c.update(ds_conv=LIB, ds_stats=BS)
    return c


def no_stats(d):
    return {k: "none" for k in ("stats1", "stats2", "stats3", "ds_stats") if d[k] is not None}


@pytest.fixture(scope="module")
def N():
    a3d = load_pkg()
    a3d.build()
    return a3d.nn


@pytest.fixture(scope="module")
def bb(N):
    return N.SyntheticCLIPResNet50().train()


def census(plan):
    return collections.Counter(plan.launches())


def test_default_routes_of_all_sixteen_blocks(N, bb):
    plan = N.backbone_plan(bb, 4, 128, 128)
    assert tuple(plan.stem) == DEFAULT_STEM
    assert [tuple(b) for b in plan.blocks] == DEFAULT
    by = {b.name: b for b in plan.blocks}
    # conv3: five blocks on the residual route, two of them with the downsample BatchNorm folded into the epilogue, layer2[0] without
    # a prologue; the last blocks of layers 1 and 2 keep the GEMM with statistics; layers 3 - 4 run the GEMM with statistics
    assert [b.name for b in plan.blocks if b.conv3 == "residual"] == RESIDUAL_BLOCKS
    assert all(by[n].ds_bn == "folded" and by[n].final == "conv3_epilogue" for n in ("layer1[0]", "layer2[0]"))
    assert [n for n in RESIDUAL_BLOCKS if by[n].bn2 != "conv3_prologue"] == ["layer2[0]"] and by["layer2[0]"].bn2 == "bn_apply_pool2"
    assert all((by[n].conv3, by[n].stats3, by[n].final) == ("gemm", "epilogue", "bn_apply_pool2") for n in ("layer1[2]", "layer2[3]"))
    assert all((b.conv3, b.stats3) == ("gemm", "epilogue") for b in plan.blocks if b.name[:6] in ("layer3", "layer4"))
    # downsample branch
    assert [by[n].ds_input for n in FIRST] == ["identity", "producer_pooled", "producer_pooled", "producer_pooled"]
    assert [b.name for b in plan.blocks if b.ds_input is not None] == FIRST
    # launches, summed over the plan
    c = census(plan)
    assert sum(b.conv2 == "library" for b in plan.blocks) == 13                      # bn1 applies ahead of the library's wide 3x3
    assert sum(b.final == "bn_apply" for b in plan.blocks) == 8
    assert c["a3d_bn_apply"] == 13 + 8
    assert [b.name for b in plan.blocks if b.bn2 == "bn_apply_pool2"] == FIRST[1:]
    assert [b.name for b in plan.blocks if b.final == "bn_apply_pool2"] == ["layer1[2]", "layer2[3]", "layer3[5]"]
    assert c["a3d_bn_apply_pool2"] == 1 + 3 + 3                                      # the stem, bn2 of the stride-2 blocks, three finals
    assert c["a3d_conv1x1_bn_residual_fwd"] == 5
    assert sum(b.stats3 == "stats_pass" for b in plan.blocks) == 5
    assert c["a3d_conv1x1_bn_fwd"] == 16 + 4 + 11 + 5                                # conv1, downsample, conv3 with a stored map, statistics only
    assert c["a3d_bn_gram"] == 0 and c["a3d_stem_conv_bn_fwd"] == 1 and c["a3d_conv3x3_bn_fwd"] == 2 + 3
    # a3d_bn_stats only behind the library's 3x3 convolutions, never behind an own GEMM
    assert c["a3d_bn_stats"] == 13 and all(b.stats2 == "bn_stats" for b in plan.blocks if b.conv2 == "library")
    assert all("bn_stats" not in (b.stats1, b.stats3, b.ds_stats) for b in plan.blocks)
    assert c["a3d_bn_finalize"] == 3 + 3 * 16 + 4
    # per block: what layer2[0] launches, in order (written from the parent's loop)
    assert by["layer2[0]"].launches() == [
        "a3d_conv1x1_bn_fwd", "a3d_bn_finalize", "a3d_bn_apply",                     # conv1; bn1 ahead of the library's 3x3
        "a3d_bn_stats", "a3d_bn_finalize", "a3d_bn_apply_pool2",                     # bn2 + pool
        "a3d_conv1x1_bn_fwd", "a3d_bn_finalize",                                     # downsample conv on the producer's pooled map; its bn folded
        "a3d_conv1x1_bn_fwd", "a3d_bn_finalize", "a3d_conv1x1_bn_residual_fwd"]      # statistics-only pass, bn3, conv3 + bn3 + add + ReLU
    assert by["layer1[2]"].launches() == [
        "a3d_conv1x1_bn_fwd", "a3d_bn_finalize", "a3d_conv3x3_bn_fwd", "a3d_bn_finalize", "a3d_conv1x1_bn_fwd", "a3d_bn_finalize",
        "a3d_bn_apply_pool2"]
    # the BatchNorms whose num_batches_tracked advance: all 55, each once
    assert len(plan.bns) == len(set(plan.bns)) == 3 + 3 * 16 + 4
    assert set(plan.bns) == {n for n, m in bb.named_modules() if type(m).__name__ == "BatchNorm2d"}


def test_routes_under_each_switch(N, bb, monkeypatch):
    rows = lambda plan: [tuple(b) for b in plan.blocks]
    base = N.backbone_plan(bb, 4, 128, 128)

    # FUSED_CONV3_RESIDUAL off: conv3 + a3d_bn_apply
    off = table(lambda d: dict(conv3=G, stats3=EPI, final=APPLY) if d["conv3"] == RES else {})
    with monkeypatch.context() as mp:
        mp.setattr(N, "FUSED_CONV3_RESIDUAL", False)                    # read at call time
        plan = N.backbone_plan(bb, 4, 128, 128)
    assert rows(plan) == off and census(plan)["a3d_bn_apply"] == 26 and census(plan)["a3d_conv1x1_bn_residual_fwd"] == 0

    # "gram": the statistics from the Gram matrix, no store-nothing pass
    gram = table(lambda d: dict(stats3="gram", final="conv3_epilogue_gram") if d["conv3"] == RES else {})
    with monkeypatch.context() as mp:
        mp.setattr(N, "FUSED_CONV3_RESIDUAL", "gram")
        plan = N.backbone_plan(bb, 4, 128, 128)
    c = census(plan)
    assert rows(plan) == gram and c["a3d_bn_gram"] == c["a3d_bn_gram_stats"] == 5 and c["a3d_conv1x1_bn_fwd"] == 16 + 4 + 11
    assert plan.blocks[1].launches()[-4:] == ["a3d_bn_gram", "a3d_bn_gram_stats", "a3d_bn_finalize", "a3d_conv1x1_bn_residual_fwd"]

    # FOLD_DOWNSAMPLE_BN off: four materialised branch applies
    with monkeypatch.context() as mp:
        mp.setattr(N, "FOLD_DOWNSAMPLE_BN", False)
        plan = N.backbone_plan(bb, 4, 128, 128)
    assert rows(plan) == table(lambda d: dict(ds_bn="materialised") if d["ds_input"] is not None else {})
    assert census(plan)["a3d_bn_apply"] == 21 + 4

    # FUSED_CONV1X1 off: every 1x1 on the library, no residual route
    with monkeypatch.context() as mp:
        mp.setattr(N, "FUSED_CONV1X1", False)
        plan = N.backbone_plan(bb, 4, 128, 128)
    c = census(plan)
    assert rows(plan) == table(lambda d: library_1x1(d, deep_only=False))
    assert c["a3d_conv1x1_bn_fwd"] == 0 and c["a3d_conv1x1_bn_residual_fwd"] == 0
    assert c["a3d_bn_apply"] == 13 + 13 + 13 and c["a3d_bn_stats"] == 16 + 13 + 16 + 4      # bn1 (library 3x3), bn2, finals | bn1, bn2, bn3, ds

    # FUSED_CONV3X3 off: no fused 3x3 rows
    with monkeypatch.context() as mp:
        mp.setattr(N, "FUSED_CONV3X3", False)
        plan = N.backbone_plan(bb, 4, 128, 128)
    assert rows(plan) == table(lambda d: dict(conv2=LIB, stats2=BS))
    assert tuple(plan.stem) == ("stem_conv", LIB, LIB, (EPI, BS, BS), P2) and census(plan)["a3d_conv3x3_bn_fwd"] == 0

    # without the deep GEMM: layers 3 - 4 on the library (and the two layer-2 shapes only the deep GEMM serves)
    lib = N.O.L.load()
    prev = lib.a3d_conv1x1_deep_mode(0)
    try:
        plan = N.backbone_plan(bb, 4, 128, 128)
    finally:
        lib.a3d_conv1x1_deep_mode(prev)
    assert rows(plan) == table(lambda d: library_1x1(d, deep_only=True))
    assert all((b.conv1, b.conv3, b.ds_conv) in ((LIB, LIB, None), (LIB, LIB, LIB)) for b in plan.blocks if b.name[:6] in ("layer3", "layer4"))
    assert [b.name for b in plan.blocks if b.conv3 == RES] == RESIDUAL_BLOCKS
    assert N.backbone_plan(bb, 4, 128, 128) == base                      # the mode is restored

    # FUSED_STEM off, or a caller that feeds normalised images (the passed value wins)
    with monkeypatch.context() as mp:
        mp.setattr(N, "FUSED_STEM", False)
        plan = N.backbone_plan(bb, 4, 128, 128)
        assert N.backbone_plan(bb, 4, 128, 128, fused_stem=True) == base
    assert plan == N.backbone_plan(bb, 4, 128, 128, fused_stem=False) and plan.blocks == base.blocks
    assert tuple(plan.stem) == (LIB, "fused", "fused", (BS, EPI, EPI), P2)
    assert N.backbone_plan(bb, 4, 128, 128, fused_stem=False).launches()[:3] == ["a3d_bn_stats", "a3d_bn_finalize", "a3d_conv3x3_bn_fwd"]

    # eval(): the same routes, no statistics launch anywhere
    try:
        plan = N.backbone_plan(bb.eval(), 4, 128, 128)
    finally:
        bb.train()
    c = census(plan)
    assert rows(plan) == table(no_stats) and tuple(plan.stem) == ("stem_conv", "fused", "fused", ("none",) * 3, P2)
    assert c["a3d_bn_stats"] == c["a3d_bn_gram"] == 0 and c["a3d_conv1x1_bn_fwd"] == 16 + 4 + 11 and c["a3d_conv1x1_bn_residual_fwd"] == 5
    assert c["a3d_bn_finalize"] == 55


def test_unserved_width_falls_back_row_by_row_and_the_plan_ignores_the_batch(N, bb):
    # W = 96: the stem's maps are 48 wide and layer 1's 24 -- a3d_conv3x3_serves wants W % 32 == 0, a3d_stem_conv_bn_fwd W % 64 == 0;
    # every map stays even, so nothing else moves
    plan = N.backbone_plan(bb, 4, 128, 96)
    assert tuple(plan.stem) == (LIB, LIB, LIB, (BS, BS, BS), P2)
    assert [tuple(b) for b in plan.blocks] == table(lambda d: dict(conv2=LIB, stats2=BS))
    # odd maps: H = 144 gives layer 3 nine rows (36 -> 18 -> 9 -> 4), which only torch's pool halves: layer4[0] and its producer fall back
    plan = N.backbone_plan(bb, 4, 144, 128)
    by = {b.name: b for b in plan.blocks}
    assert (by["layer2[3]"].final, by["layer3[0]"].bn2, by["layer3[0]"].ds_input) == (P2, P2, "producer_pooled")       # 18 -> 9 rows
    assert (by["layer3[5]"].final, by["layer4[0]"].bn2, by["layer4[0]"].ds_input) == (APPLY, "bn_apply+torch_pool", "torch_pool")   # 9 -> 4
    # built from a CPU module, equal for 4 and 256 images
    assert all(not p.is_cuda for p in bb.parameters())
    assert N.backbone_plan(bb, 4, 128, 128) == N.backbone_plan(bb, 256, 128, 128)
