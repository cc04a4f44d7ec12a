"""bn3 + residual + ReLU folded into the bottleneck's conv3 (csrc/bn_gram.hip, conv1x1_stream_kernel's RS epilogue): the Gram matrix of
conv3's input, the statistics of its output derived from it, the fused convolution, and the backbone with the route on and off.
Everything is called through lib.py; references are float64 on the CPU."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1024          # floats of poisoned guard band on each side of an output
POISON = -12345.0
_cases = {}


def _chunk_rows(K):
    return 8192 // K                                  # a3d_bn_gram deals rows in chunks of 8192 / K (include/act3d_hip.h)


def _staged(x, sc, sh, relu=True):
    """the bf16 A operand the GEMM multiplies, as _check_conv1x1 (test_kernels_gpu.py) restates it: x * scale + shift as ONE rounding"""
    if sc is None:
        return x.double()
    v = (x.double() * sc.double() + sh.double()).float()
    return (torch.relu(v) if relu else v).to(torch.bfloat16).double()


def _gram_case(a3d, dev, M, K, pro):
    """one a3d_bn_gram launch per (M, K, pro), shared by the Gram and the statistics tests; the reference operand stays on the CPU"""
    key = (M, K, pro)
    if key in _cases:
        return _cases[key]
    L = a3d.lib
    g = torch.Generator().manual_seed(7 * M + K + int(pro))
    x = (torch.randn(M, K, generator=g) * 1.3 + 0.2).to(torch.bfloat16)
    sc = (1.0 + 0.3 * torch.randn(K, generator=g)) if pro else None
    sh = (0.2 * torch.randn(K, generator=g) + 0.1) if pro else None           # non-zero shift: a padded row would add relu(shift)
    nslab = L.load().a3d_bn_gram_nslab(M, K)
    nchunk = -(-M // _chunk_rows(K))
    assert 1 <= nslab <= nchunk
    ng, ns = nslab * K * K, nslab * K
    buf = torch.full((3 * GUARD + ng + ns,), POISON, device=dev, dtype=torch.float32)
    gp, sp = buf[GUARD:GUARD + ng], buf[2 * GUARD + ng:2 * GUARD + ng + ns]
    xd = x.to(dev)
    scd, shd = (None, None) if not pro else (sc.to(dev), sh.to(dev))
    args = (xd.data_ptr(), None if scd is None else scd.data_ptr(), None if shd is None else shd.data_ptr(), 1 if pro else 0)
    L.call("a3d_bn_gram", *args, gp.data_ptr(), sp.data_ptr(), M, K, nslab, L.stream())
    torch.cuda.synchronize()
    first = buf.clone()
    L.call("a3d_bn_gram", *args, gp.data_ptr(), sp.data_ptr(), M, K, nslab, L.stream())
    torch.cuda.synchronize()
    case = dict(a=_staged(x.float(), sc, sh), nslab=nslab, rows_per_slab=-(-nchunk // nslab) * _chunk_rows(K), buf=buf, first=first,
                gp=gp.view(nslab, K, K), sp=sp.view(nslab, K), ng=ng, ns=ns)
    _cases[key] = case
    return case


@pytest.mark.parametrize("M,K", [(130, 64), (5000, 64), (4096, 128), (70001, 128)])
@pytest.mark.parametrize("pro", [False, True])
def test_gram_matrix_and_column_sums_of_the_staged_operand(a3d, dev, M, K, pro):
    """a3d_bn_gram: sum over slabs of the partial Gram matrices / column sums against float64 a^T a / sum_m a of the staged bf16
    operand.  The bf16 products are exact in fp32, only the accumulation rounds: per element at most
    (rows_per_slab + nslab) 2^-24 sum_m |a_mk| |a_ml| (resp. sum_m |a_mk|).  Two launches give the same bits; the guard bands stay."""
    c = _gram_case(a3d, dev, M, K, pro)
    a = c["a"]
    n_acc = c["rows_per_slab"] + c["nslab"]
    G = c["gp"].double().sum(0).cpu()
    S = c["sp"].double().sum(0).cpu()
    ref_g, bound_g = a.t() @ a, n_acc * 2.0 ** -24 * (a.abs().t() @ a.abs())
    ref_s, bound_s = a.sum(0), n_acc * 2.0 ** -24 * a.abs().sum(0)
    eg, es = (G - ref_g).abs(), (S - ref_s).abs()
    print(f"[parity] gram M={M} K={K} pro={pro}: nslab={c['nslab']} max err/bound G={(eg / bound_g.clamp_min(1e-30)).max().item():.3f} "
          f"S={(es / bound_s.clamp_min(1e-30)).max().item():.3f}")
    assert torch.isfinite(G).all() and torch.isfinite(S).all()
    assert (eg <= bound_g).all(), f"Gram: max err {eg.max().item():.3e}"
    assert (es <= bound_s).all(), f"column sums: max err {es.max().item():.3e}"
    assert torch.equal(c["first"], c["buf"]), "two launches differ"
    buf, ng, ns = c["buf"], c["ng"], c["ns"]
    for lo, hi in [(0, GUARD), (GUARD + ng, 2 * GUARD + ng), (2 * GUARD + ng + ns, 3 * GUARD + ng + ns)]:
        assert (buf[lo:hi] == POISON).all(), "guard band written"


@pytest.mark.parametrize("M,K,N", [(5000, 64, 256), (70001, 128, 512)])
def test_output_statistics_from_the_gram_matrix(a3d, dev, M, K, N):
    """a3d_bn_gram_stats + a3d_bn_finalize on the partials above: scale, shift and the running statistics against float64 BatchNorm
    statistics of the exact product a w^T, at the running-statistics tolerances of test_fused_batchnorm_train_relu_residual
    (atol 1e-5, rtol 1e-4); then the eval-mode finalize on the running statistics just written."""
    L = a3d.lib
    c = _gram_case(a3d, dev, M, K, True)
    g = torch.Generator().manual_seed(M + N)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    eps, mom = 1e-5, 0.1
    wd, gd, bd = w.to(dev), gamma.to(dev), beta.to(dev)
    work = torch.empty(K * K + K, device=dev, dtype=torch.float64)
    stats = torch.full((1, 2, N), float("nan"), device=dev, dtype=torch.float32)
    rm, rv = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    out = torch.full((2, N), float("nan"), device=dev, dtype=torch.float32)
    L.call("a3d_bn_gram_stats", c["gp"].data_ptr(), c["sp"].data_ptr(), c["nslab"], wd.data_ptr(), K, N, work.data_ptr(), stats.data_ptr(),
           L.stream())
    L.call("a3d_bn_finalize", stats.data_ptr(), 1, M, N, eps, mom, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
           out[0].data_ptr(), out[1].data_ptr(), 1, L.stream())
    torch.cuda.synchronize()
    o = c["a"] @ w.double().t()
    mean, var = o.mean(0), o.var(0, unbiased=False)
    sc = gamma.double() / torch.sqrt(var + eps)
    refs = {"scale": sc, "shift": beta.double() - mean * sc, "running_mean": mom * mean,
            "running_var": (1 - mom) * 1.0 + mom * var * M / (M - 1)}
    got = {"scale": out[0], "shift": out[1], "running_mean": rm, "running_var": rv}
    for k, r in refs.items():
        e = (got[k].double().cpu() - r).abs()
        print(f"[parity] gram stats {K}->{N} {k}: max_abs_err={e.max().item():.3e} ref_absmax={r.abs().max().item():.3e}")
        assert torch.isfinite(got[k]).all() and (e <= 1e-5 + 1e-4 * r.abs()).all(), k
    # eval mode: no statistics at all, scale / shift from the running statistics, which stay as they are
    rm0, rv0 = rm.clone(), rv.clone()
    ev = torch.full((2, N), float("nan"), device=dev, dtype=torch.float32)
    L.call("a3d_bn_finalize", None, 1, M, N, eps, mom, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(), ev[0].data_ptr(),
           ev[1].data_ptr(), 0, L.stream())
    torch.cuda.synchronize()
    esc = gamma.double() / torch.sqrt(rv0.double().cpu() + eps)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    assert ((ev[0].double().cpu() - esc).abs() <= 1e-5 + 1e-4 * esc.abs()).all()
    esh = beta.double() - rm0.double().cpu() * esc
    assert ((ev[1].double().cpu() - esh).abs() <= 1e-5 + 1e-4 * esh.abs()).all()


@pytest.mark.parametrize("M", [1000, 4099, 70001])
@pytest.mark.parametrize("K,N", [(64, 256), (128, 512)])
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("relu", [True, False])
def test_conv3_with_batchnorm_residual_relu_epilogue(a3d, dev, M, K, N, rs, relu):
    """a3d_conv1x1_bn_residual_fwd: y = bf16(max(f(x) w^T * osc + osh + r, lo)), r = res or res * rsc + rsh, against float64 on the same
    bf16 operands at the one-rounding bar of _check_conv1x1 (2^-8 |ref| + 1e-3).  The producer's BatchNorm prologue rides along except
    on the (folded downsample, 128 -> 512) cases -- layer 2's first block feeds conv3 an already normalised pooled map.  The output
    and 64 rows behind it are pre-filled with NaN: every row is written, none beyond."""
    L = a3d.lib
    pro = not (rs and K == 128)
    g = torch.Generator().manual_seed(M + K + N + 2 * int(rs) + int(relu))
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    sc = (1.0 + 0.3 * torch.randn(K, generator=g)) if pro else None
    sh = (0.2 * torch.randn(K, generator=g)) if pro else None
    osc, osh = 1.0 + 0.3 * torch.randn(N, generator=g), 0.2 * torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16)
    rsc = (1.0 + 0.3 * torch.randn(N, generator=g)) if rs else None
    rsh = (0.2 * torch.randn(N, generator=g)) if rs else None
    d = lambda t: None if t is None else t.to(dev).contiguous()
    xd, wd, scd, shd, oscd, oshd, resd, rscd, rshd = map(d, (x, w, sc, sh, osc, osh, res, rsc, rsh))
    p = lambda t: None if t is None else t.data_ptr()
    y = torch.full((M + 64, N), float("nan"), device=dev, dtype=torch.bfloat16)
    assert L.load().a3d_conv1x1_bn_residual_serves(K, N) == 1
    L.call("a3d_conv1x1_bn_residual_fwd", xd.data_ptr(), wd.data_ptr(), p(scd), p(shd), 1 if pro else 0, oscd.data_ptr(), oshd.data_ptr(),
           resd.data_ptr(), p(rscd), p(rshd), 1 if relu else 0, 0, y.data_ptr(), M, K, N, L.stream())
    torch.cuda.synchronize()
    r = res.double() if not rs else res.double() * rsc.double() + rsh.double()
    ref = (_staged(x.float(), sc, sh) @ w.double().t()) * osc.double() + osh.double() + r
    if relu:
        ref = torch.relu(ref)
    got = y[:M].double().cpu()
    err = (got - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-3
    print(f"[parity] conv3+bn+res M={M} {K}->{N} rs={rs} relu={relu}: max_abs_err={err.max().item():.3e} worst err/tol={(err / tol).max().item():.3f}")
    assert torch.isfinite(got).all(), "rows left unwritten"
    assert (err <= tol).all(), f"max err {err.max().item():.3e} at {torch.nonzero(err > tol)[:3].tolist()}"
    assert torch.isnan(y[M:]).all(), "rows behind the output written"


@pytest.mark.parametrize("M,K,N", [(4099, 64, 256), (70001, 128, 512)])
@pytest.mark.parametrize("rs", [False, True])
def test_round_first_route_equals_the_unfused_kernels_bit_for_bit(a3d, dev, M, K, N, rs):
    """Statistics-only a3d_conv1x1_bn_fwd (y NULL) leaves the partial sums of the full call; a3d_conv1x1_bn_residual_fwd with
    round_conv on their finalized scale / shift equals a3d_conv1x1_bn_fwd + a3d_bn_apply: torch.equal, ragged row counts included."""
    L = a3d.lib
    g = torch.Generator().manual_seed(M + N + int(rs))
    d = lambda t: t.to(dev).contiguous()
    x = d(torch.randn(M, K, generator=g).to(torch.bfloat16))
    w = d((torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16))
    sc, sh = d(1.0 + 0.3 * torch.randn(K, generator=g)), d(0.2 * torch.randn(K, generator=g))
    res = d(torch.randn(M, N, generator=g).to(torch.bfloat16))
    rsc, rsh = (d(1.0 + 0.3 * torch.randn(N, generator=g)), d(0.2 * torch.randn(N, generator=g))) if rs else (None, None)
    gamma, beta = d(torch.rand(N, generator=g) + 0.5), d(torch.randn(N, generator=g) * 0.2)
    p = lambda t: None if t is None else t.data_ptr()
    nslab = L.load().a3d_conv1x1_nslab(M, K, N)
    o3 = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
    part_a = torch.full((nslab, 2, N), float("nan"), device=dev)
    part_b = torch.full((nslab, 2, N), float("nan"), device=dev)
    L.call("a3d_conv1x1_bn_fwd", x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), 1, o3.data_ptr(), part_a.data_ptr(), M, K, N, L.stream())
    L.call("a3d_conv1x1_bn_fwd", x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), 1, None, part_b.data_ptr(), M, K, N, L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(part_b).all() and torch.equal(part_a, part_b)
    ss = torch.empty((2, N), device=dev)
    rm, rv = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    L.call("a3d_bn_finalize", part_b.data_ptr(), nslab, M, N, 1e-5, 0.1, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(),
           ss[0].data_ptr(), ss[1].data_ptr(), 1, L.stream())
    want = torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
    L.call("a3d_bn_apply", o3.data_ptr(), res.data_ptr(), p(rsc), p(rsh), ss[0].data_ptr(), ss[1].data_ptr(), want.data_ptr(), M, N, 1, L.stream())
    got = torch.full((M + 64, N), float("nan"), device=dev, dtype=torch.bfloat16)
    L.call("a3d_conv1x1_bn_residual_fwd", x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), 1, ss[0].data_ptr(), ss[1].data_ptr(),
           res.data_ptr(), p(rsc), p(rsh), 1, 1, got.data_ptr(), M, K, N, L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and torch.equal(got[:M], want)
    assert torch.isnan(got[M:]).all()


def test_conv3_residual_refuses_unserved_shapes(a3d, dev):
    lib = a3d.lib.load()
    t = torch.zeros(64, device=dev)
    q = t.data_ptr()
    for K, N in [(64, 64), (256, 512), (64, 320)]:
        assert lib.a3d_conv1x1_bn_residual_serves(K, N) == 0
        assert lib.a3d_conv1x1_bn_residual_fwd(q, q, None, None, 0, q, q, q, None, None, 1, 0, q, 16, K, N, None) == -22


@pytest.mark.parametrize("mode", [True, "gram"])
def test_backbone_with_conv3_residual_route(a3d, dev, mode):
    """The backbone with conv3 + bn3 + add + ReLU in one launch -- FUSED_CONV3_RESIDUAL True (default: statistics of the rounded conv3
    outputs, round-first epilogue) and "gram" (statistics from the Gram matrix, one rounding) -- is as close to the fp32 module as
    the route it replaces (flag off), by the criterion of test_backbone_with_fused_1x1_convolutions_matches_miopen_path; the default
    mode reproduces the flag-off maps and running statistics bit for bit; the
    running statistics of a block on the new route follow the fp32 module; the route is deterministic and writes `out=` in place.
    The library's 3x3 convolution of layer 2 (128 channels, 32 x 32) is not run-to-run reproducible in its default algorithm -- with
    the route on or off -- so the bf16 runs pin the library to its deterministic algorithms for the bit-for-bit comparisons."""
    torch.manual_seed(0)
    bb32 = a3d.nn.SyntheticCLIPResNet50().to(dev).train()
    nets = {"off": copy.deepcopy(bb32), "on": copy.deepcopy(bb32), "on2": copy.deepcopy(bb32), "out": copy.deepcopy(bb32)}
    x = torch.rand(4, 3, 128, 128, device=dev).contiguous(memory_format=torch.channels_last)
    outs = {}
    keep, keep_det = a3d.nn.FUSED_CONV3_RESIDUAL, torch.backends.cudnn.deterministic
    with torch.no_grad():
        ref = bb32(x)
        try:
            torch.backends.cudnn.deterministic = True
            for name in ("off", "on", "on2"):
                a3d.nn.FUSED_CONV3_RESIDUAL = False if name == "off" else mode
                outs[name] = a3d.nn.run_frozen_backbone(nets[name], x.clone(), torch.bfloat16, keep_dtype=True)
            a3d.nn.FUSED_CONV3_RESIDUAL = mode
            bufs = {k: torch.full_like(v, float("nan")) for k, v in outs["on"].items()}
            ptrs = {k: v.data_ptr() for k, v in bufs.items()}
            got = a3d.nn.run_frozen_backbone(nets["out"], x.clone(), torch.bfloat16, keep_dtype=True, out=bufs)
        finally:
            a3d.nn.FUSED_CONV3_RESIDUAL, torch.backends.cudnn.deterministic = keep, keep_det
    torch.cuda.synchronize()
    rms = lambda t: t.float().pow(2).mean().sqrt().item()
    for k in ref:
        e_on, e_off, sc = rms(outs["on"][k].float() - ref[k]), rms(outs["off"][k].float() - ref[k]), rms(ref[k])
        print(f"[parity] backbone {k}: mode={mode} rms_err conv3-residual on={e_on:.3e} off={e_off:.3e} ref_rms={sc:.3e}")
        assert torch.isfinite(outs["on"][k]).all() and e_on <= 1.25 * e_off + 1e-3 * sc, k
        assert torch.equal(outs["on"][k], outs["on2"][k]), k
        assert mode == "gram" or torch.equal(outs["on"][k], outs["off"][k]), k
        assert got[k].data_ptr() == ptrs[k] and bufs[k].data_ptr() == ptrs[k] and torch.equal(bufs[k], outs["on"][k]), k
    tol = lambda r: 1e-3 + 1e-2 * r.abs()
    rv_on, rv_ref = nets["on"].layer1[0].bn3.running_var, bb32.layer1[0].bn3.running_var
    rm_on, rm_ref = nets["on"].layer2[3].bn3.running_mean, bb32.layer2[3].bn3.running_mean
    print(f"[parity] layer1[0].bn3.running_var max_abs_err={(rv_on - rv_ref).abs().max().item():.3e}; "
          f"layer2[3].bn3.running_mean max_abs_err={(rm_on - rm_ref).abs().max().item():.3e}")
    assert ((rv_on - rv_ref).abs() <= tol(rv_ref)).all()
    assert ((rm_on - rm_ref).abs() <= tol(rm_ref)).all()
    for (n, p), (_, q), (_, r) in zip(bb32.named_buffers(), nets["on"].named_buffers(), nets["off"].named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert torch.equal(p, q), n
        assert mode == "gram" or torch.equal(q, r), n
