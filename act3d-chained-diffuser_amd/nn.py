"""Parameter containers that mirror the reference's module tree (names, shapes, initialisation) so that state
dicts are interchangeable, with forward passes that launch the HIP operators of ops.py.

Reference classes mirrored: MultiheadCustomAttention (multihead_custom_attention.py:14-94), RelativeCrossAttentionLayer /
FeedforwardLayer / RelativeCrossAttentionModule (layers.py:293-351), ParallelAttentionLayer / ParallelAttention / AdaLN
(layers.py:7-290), torchvision's FeaturePyramidNetwork (third-party; restated) and a synthetic CLIP-RN50-shaped backbone.
"""
import collections
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops as O


class MultiheadCustomAttention(nn.Module):
    """Holds in_proj_weight (3E,E), in_proj_bias (3E), out_proj (Linear E->E); init as multihead_custom_attention.py:80-94."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        assert embed_dim % num_heads == 0 and embed_dim // num_heads == 15, \
            "the HIP attention kernels are specialised for head_dim 15 (60/4, 120/8), as in both reference models"
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.out_proj.bias, 0.0)


class RelativeCrossAttentionLayer(nn.Module):
    def __init__(self, embedding_dim, num_heads, dropout=0.0):
        super().__init__()
        self.multihead_attn = MultiheadCustomAttention(embedding_dim, num_heads, dropout=dropout)
        self.norm = nn.LayerNorm(embedding_dim)
        self.num_heads = num_heads

    def forward(self, query, value, query_xyz=None, value_xyz=None, pad_mask=None, sink=None, kv_pair=None):
        """query (B, Lq, E), value (B, S, E) batch-first; xyz instead of materialised rotary codes.  sink: the GradSink of
        `value` when its consumers share one gradient buffer (ops.GradSink).  kv_pair: this layer's k | v operand rows when the
        caller projected the context for several layers at once (ops.ctx_kv_operands16)."""
        return O.attn_block(query, value, value, query, query_xyz, value_xyz, pad_mask, self.multihead_attn, self.norm,
                            self.num_heads, sink=sink, kv_pair=kv_pair)


class FeedforwardLayer(nn.Module):
    def __init__(self, embedding_dim, hidden_dim, dropout=0.0):
        super().__init__()
        self.linear1 = nn.Linear(embedding_dim, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, embedding_dim)
        self.norm = nn.LayerNorm(embedding_dim)
        for p in self.parameters():                   # layers.py:323-326
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, x):
        return O.mlp(x, self.linear1, self.linear2, self.norm)


class RelativeCrossAttentionModule(nn.Module):
    def __init__(self, embedding_dim, num_attn_heads, num_layers):
        super().__init__()
        self.attn_layers = nn.ModuleList(
            [RelativeCrossAttentionLayer(embedding_dim, num_attn_heads) for _ in range(num_layers)])
        self.ffw_layers = nn.ModuleList([FeedforwardLayer(embedding_dim, embedding_dim) for _ in range(num_layers)])

    def forward(self, query, value, query_xyz=None, value_xyz=None):
        """Returns the list of per-layer outputs (layers.py:345-351), batch-first."""
        output = []
        sink = getattr(value, "_a3d_sink", None)      # the context's shared gradient buffer (act3d.py attaches it), or None
        # the ghost stream: every layer projects the SAME context rows -- their k | v operands in one launch that reads them once
        pairs = None
        mhas = [a.multihead_attn for a in self.attn_layers]
        if (len(mhas) > 0 and query.shape[1] != 1 and query.is_cuda and query.dtype == torch.float32 and
                not O.query_layer_applicable(query, value, mhas[0].embed_dim, self.attn_layers[0].num_heads,
                                             self.ffw_layers[0].linear1.out_features) and
                all(a.num_heads == self.attn_layers[0].num_heads for a in self.attn_layers) and
                O.ctx_kv_applicable(value, value_xyz, mhas, self.attn_layers[0].num_heads, query.shape[1])):
            pairs = O.ctx_kv_operands16(value, value_xyz, mhas, self.attn_layers[0].num_heads)
        for j, (attn, ffw) in enumerate(zip(self.attn_layers, self.ffw_layers)):
            mha = attn.multihead_attn
            if O.query_layer_applicable(query, value, mha.embed_dim, attn.num_heads, ffw.linear1.out_features):
                # the one-query stream: attention block + FFN of a layer as the fused launches of csrc/query_stream.hip
                query = O.QueryLayerFn.apply(query, value, query_xyz, value_xyz, mha.in_proj_weight, mha.in_proj_bias,
                                             mha.out_proj.weight, mha.out_proj.bias, attn.norm.weight, attn.norm.bias,
                                             ffw.linear1.weight, ffw.linear1.bias, ffw.linear2.weight, ffw.linear2.bias,
                                             ffw.norm.weight, ffw.norm.bias, attn.num_heads, sink)
            else:
                query = ffw(attn(query, value, query_xyz, value_xyz, sink=sink, kv_pair=None if pairs is None else pairs[j]))
            output.append(query)
        return output


class AdaLN(nn.Module):
    def __init__(self, embedding_dim):
        super().__init__()
        self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(embedding_dim, 2 * embedding_dim, bias=True))
        nn.init.constant_(self.modulation[-1].weight, 0)
        nn.init.constant_(self.modulation[-1].bias, 0)

    def forward(self, x, silu_t):
        """x (B, N, C); silu_t = SiLU(t) (B, C), computed once per forward and shared by every AdaLN."""
        return O.AdaLNFn.apply(x, O.linear(silu_t, self.modulation[1]))


class ParallelAttentionLayer(nn.Module):
    """The seq1-only configuration the hot path uses (cross_attention1 [+ self_attention1] [+ ffn]); layers.py:7-218."""

    def __init__(self, d_model=256, dropout=0.1, n_heads=8, pre_norm=False, self_attention1=True,
                 self_attention2=False, cross_attention1=True, cross_attention2=False, apply_ffn=True,
                 slot_attention12=False, slot_attention21=False, rotary_pe=False, use_adaln=False):
        super().__init__()
        if pre_norm or self_attention2 or cross_attention2 or slot_attention12 or slot_attention21 or not cross_attention1:
            raise NotImplementedError("only the seq1 / post-norm configuration of ParallelAttentionLayer is on the hot "
                                      "path (SURVEY §8a-12); other options are not implemented")
        self.self_attention1, self.apply_ffn, self.rotary_pe = self_attention1, apply_ffn, rotary_pe
        self.n_heads, self.dropout_p = n_heads, dropout
        self.site_base = O.site_id("parallel_attention_layer")     # re-assigned from the module's name by its owner
        if self_attention1:
            self.adaln_1 = AdaLN(d_model) if use_adaln else None
            self.sa1 = MultiheadCustomAttention(d_model, n_heads, dropout=dropout)
            self.norm_1 = nn.LayerNorm(d_model)
        self.adaln_12 = AdaLN(d_model) if use_adaln else None
        self.cross_12 = MultiheadCustomAttention(d_model, n_heads, dropout=dropout)
        self.norm_12 = nn.LayerNorm(d_model)
        # the reference builds FFN-1 whenever seq1 is updated, even if apply_ffn=False leaves it unused
        self.adaln_ff1 = AdaLN(d_model) if use_adaln else None
        self.ffn_12 = nn.Sequential(nn.Linear(d_model, 4 * d_model), nn.ReLU(), nn.Dropout(dropout),
                                    nn.Linear(4 * d_model, d_model), nn.Dropout(dropout))
        self.norm_122 = nn.LayerNorm(d_model)

    def forward(self, seq1, seq1_key_padding_mask, seq2, seq1_xyz=None, seq2_xyz=None, seq1_sem_pos=None, silu_t=None,
                drop=None, cross_cache=None):
        """drop: ops.DropCtx of this forward pass (None: no dropout).  Training with dropout_p > 0 needs one -- the owner
        (DiffusionHead.begin_dropout) creates it; there is no silent un-regularised path.
        cross_cache: this layer's prebuilt K/V operands (ops.kv_cache_build): the cross-attention block reads them instead of
        projecting seq2, which is then unused (inference against the step-invariant context: no autograd, no dropout)."""
        cached = cross_cache is not None
        if self.training and self.dropout_p > 0 and drop is None and not cached:
            raise RuntimeError("ParallelAttentionLayer in training mode with dropout=%g needs the forward pass's DropCtx "
                               "(DiffusionHead.begin_dropout())" % self.dropout_p)
        if drop is not None and (cached or not self.training or self.dropout_p <= 0):
            drop = None
        sb = self.site_base
        rope = self.rotary_pe
        q1 = seq1 if seq1_sem_pos is None else O.AddRowsFn.apply(seq1, seq1_sem_pos)
        qa = self.adaln_12(q1, silu_t) if (self.adaln_12 is not None and silu_t is not None) else q1
        if cached:
            seq1 = O.attn_block_cached(qa, seq1, seq1_xyz if rope else None, cross_cache, self.cross_12, self.norm_12, self.n_heads)
        else:
            # (seq2 may carry a shared gradient sink -- DiffusionHead.forward_tokens attaches one to the context all its
            # cross-attention layers read: their k | v projection gradients are then parked and run as ONE input- and ONE
            # weight-gradient GEMM)
            seq1 = O.attn_block(qa, seq2, seq2, seq1, seq1_xyz if rope else None, seq2_xyz if rope else None, None,
                                self.cross_12, self.norm_12, self.n_heads, drop=drop, site=sb, sink=getattr(seq2, "_a3d_sink", None))
        if self.self_attention1:
            q1 = seq1 if seq1_sem_pos is None else O.AddRowsFn.apply(seq1, seq1_sem_pos)
            if self.adaln_1 is not None and silu_t is not None:
                qk, vv = self.adaln_1(q1, silu_t), self.adaln_1(seq1, silu_t)
            else:
                qk, vv = q1, seq1
            # (the fp16 attention core takes the site as a launch argument even where nothing is dropped: the cached walk keeps
            # handing it the 0 it always has)
            seq1 = O.attn_block(qk, qk, vv, seq1, seq1_xyz if rope else None, seq1_xyz if rope else None,
                                seq1_key_padding_mask, self.sa1, self.norm_1, self.n_heads, drop=drop, site=0 if cached else sb + 2)
        if self.apply_ffn:
            y = self.adaln_ff1(seq1, silu_t) if (self.adaln_ff1 is not None and silu_t is not None) else seq1
            seq1 = O.mlp(y, self.ffn_12[0], self.ffn_12[3], self.norm_122, drop=drop, site_hidden=sb + 4, site_out=sb + 5)
        return seq1


class ParallelAttention(nn.Module):
    def __init__(self, num_layers=1, **kw):
        super().__init__()
        self.layers = nn.ModuleList([ParallelAttentionLayer(**kw) for _ in range(num_layers)])

    def forward(self, seq1, seq1_key_padding_mask, seq2, cross_caches=None, **kw):
        """cross_caches: one K/V cache per layer, in layer order (ParallelAttentionLayer.forward's cross_cache)."""
        for i, layer in enumerate(self.layers):
            seq1 = layer(seq1, seq1_key_padding_mask, seq2, cross_cache=None if cross_caches is None else cross_caches[i], **kw)
        return seq1


# ------------------------------------------------------------------------------------------------ adjacent: vision
class _Upsample2AddFn(torch.autograd.Function):
    """lat + bias + F.interpolate(top, 2x, nearest) for bf16 channels_last maps in one kernel; backward: dtop = 2x2 sums of
    dy and, in the same pass, the column sums of dy = the bias gradient, accumulated straight into bias.grad (as every wgrad
    kernel of ops.py does).  `bias`: the lateral convolution's fp32 Parameter (<= C entries; the convolution itself runs
    bias-free) or None; `top` None at the pyramid's top level."""

    @staticmethod
    def forward(ctx, lat, top, bias):
        N, C, H, W = lat.shape
        y = torch.empty_like(lat)
        O.L.call("a3d_upsample2_add_fwd", lat.data_ptr(), None if top is None else top.data_ptr(),
                 None if bias is None else bias.data_ptr(), 0 if bias is None else bias.numel(), y.data_ptr(), N, H, W, C,
                 O.L.stream())
        ctx.bias = bias
        ctx.has_top = top is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        dy, dtop = _top_down_backward(dy, ctx.bias, ctx.has_top and ctx.needs_input_grad[1])
        return (dy if ctx.needs_input_grad[0] else None), dtop, None


def _top_down_backward(dy, bias, want_top):
    """backward of y = lat + bias + up2(top) from dy (N, C, H, W) bf16: d top = the 2x2 sums of dy, d bias accumulated straight into
    bias.grad (the lateral branch's gradient is dy itself).  Returns (dy channels_last, d top or None)."""
    N, C, H, W = dy.shape
    want_bias = bias is not None and bias.requires_grad
    dtop = None
    if want_top or want_bias:
        dy = dy.contiguous(memory_format=torch.channels_last)
        if want_top:
            dtop = torch.empty((N, C, H // 2, W // 2), device=dy.device, dtype=dy.dtype, memory_format=torch.channels_last)
        ws = gb = None
        if want_bias:
            ws = torch.empty((O.L.load().a3d_upsample2_add_bwd_ws_floats(N, H, W, C),), device=dy.device, dtype=torch.float32)
            gb = O.grad_buf(bias)
        O.L.call("a3d_upsample2_add_bwd", dy.data_ptr(), None if dtop is None else dtop.data_ptr(),
                 None if gb is None else gb.data_ptr(), 0 if gb is None else gb.numel(), None if ws is None else ws.data_ptr(),
                 N, H, W, C, O.L.stream())
    return dy, dtop


# The FPN's lateral 1x1 convolutions of the fine levels (K <= 256 input channels: res1 / res2 of the CLIP ResNet) as ONE launch with the
# bias and the top-down add in the epilogue (a3d_conv1x1_topdown_fwd) instead of library convolution + a3d_upsample2_add_fwd: at the
# bench shape 332 + 375 us -> one ~1.2 GB pass for the 128 x 128 level (profiles/r06_fpn_fwd_probe.json).  A3D_FPN_LATERAL=0: A/B.
FUSED_FPN_LATERAL = os.environ.get("A3D_FPN_LATERAL", "1") not in ("0", "", "off")
# The FPN's 3x3 output convolutions (64 padded channels) through the backbone's implicit-GEMM stream kernel (a3d_conv3x3_bn_fwd without
# its BatchNorm folds) instead of the library: 911 -> 405 us for the 128 x 128 level of 256 images.  A3D_FPN_OUT3X3=0: A/B.
FUSED_FPN_OUT3X3 = os.environ.get("A3D_FPN_OUT3X3", "1") not in ("0", "", "off")


class _LateralTopDownFn(torch.autograd.Function):
    """bf16(conv1x1(x, w) + bias + up2(top)) in one launch (torchvision FPN: inner_blocks[i] + the top-down add).  x bf16 channels_last
    (the frozen backbone's map), w the fp32 weight (Co, K, 1, 1) (already zero-padded to the map width), bias the fp32 Parameter
    (<= Co entries), top bf16 channels_last at half the resolution.  Backward: (d top, d bias) as _Upsample2AddFn, d w from the library's
    weight-gradient kernel (the same one the unfused convolution's autograd runs), d x only when asked for."""

    @staticmethod
    def forward(ctx, x, w, bias, top):
        N, K, H, W = x.shape
        Co = w.shape[0]
        w16 = w.detach().to(torch.bfloat16).reshape(Co, K).contiguous()
        y = torch.empty((N, Co, H, W), device=x.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
        O.L.call("a3d_conv1x1_topdown_fwd", x.data_ptr(), w16.data_ptr(), None if bias is None else bias.data_ptr(),
                 0 if bias is None else bias.numel(), None if top is None else top.data_ptr(), y.data_ptr(), N, H, W, K, Co, O.L.stream())
        ctx.save_for_backward(x, w16)
        ctx.bias = bias
        ctx.has_top = top is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16 = ctx.saved_tensors
        dy, dtop = _top_down_backward(dy, ctx.bias, ctx.has_top and ctx.needs_input_grad[3])
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        if need_x or need_w:
            dy = dy.contiguous(memory_format=torch.channels_last)
            w4 = w16.view(w16.shape[0], w16.shape[1], 1, 1)
            dx, dw, _ = torch.ops.aten.convolution_backward(dy, x, w4, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, (need_x, need_w, False))
        return dx, (None if dw is None else dw.float()), None, dtop


def _fused_lateral_ok(x, Co, last):
    cl = torch.channels_last
    return bool(FUSED_FPN_LATERAL and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous(memory_format=cl)
                and O.L.load().a3d_conv1x1_topdown_serves(x.shape[1], Co)
                and (last is None or (last.dtype == torch.bfloat16 and last.is_contiguous(memory_format=cl) and last.shape[1] == Co
                                      and x.shape[-2] == 2 * last.shape[-2] and x.shape[-1] == 2 * last.shape[-1])))


def _fused_top_down_ok(lat, last, with_bias=False):
    cl = torch.channels_last
    ok = (lat.is_cuda and lat.dtype == torch.bfloat16 and lat.shape[1] % 4 == 0 and lat.shape[-2] % 2 == 0 and lat.shape[-1] % 2 == 0
          and lat.is_contiguous(memory_format=cl))
    if last is not None:
        ok = ok and (last.dtype == torch.bfloat16 and lat.shape[-2] == 2 * last.shape[-2] and lat.shape[-1] == 2 * last.shape[-1]
                     and last.is_contiguous(memory_format=cl))
    if with_bias:
        ok = ok and 256 % (lat.shape[1] // 4) == 0
    return ok


def fpn_top_down(lat, last, bias=None):
    """inner_lateral (+ its convolution's bias, when the convolution ran bias-free) + nearest-upsampled last_inner
    (torchvision FPN); fused HIP kernel for the exact-2x bf16 NHWC case."""
    if _fused_top_down_ok(lat, last, bias is not None):
        return _Upsample2AddFn.apply(lat, last, bias)
    if bias is not None:
        lat = lat + F.pad(bias, (0, lat.shape[1] - bias.numel())).to(lat.dtype).view(1, -1, 1, 1)
    return lat if last is None else lat + F.interpolate(last, size=lat.shape[-2:], mode="nearest")


class _LayerConv3x3Fn(torch.autograd.Function):
    """The FPN's 3x3 output convolution (bias-free, stride 1, padding 1, bf16 channels_last, 64 channels) with a SPLIT backward:
    the input gradient is the library's (MIOpen), the weight gradient is taken from the map's gather consumers when they have
    computed it token-sparsely (ops.SparseConvCtx / csrc/fpn_sparse.hip) -- the dense weight-gradient kernel (0.72 ms per step at
    the bench shape, over a gradient map that is non-zero on 6 - 12 % of its pixels) then does not run at all."""

    @staticmethod
    def forward(ctx, x, w, cc):
        w16 = w.to(x.dtype)
        if (FUSED_FPN_OUT3X3 and x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
                and O.L.load().a3d_conv3x3_serves(x.shape[1], w16.shape[0], x.shape[2], x.shape[3])):
            # the backbone's implicit-GEMM stream kernel without its BatchNorm folds (a3d_conv3x3_bn_fwd; w [Cout][3][3][Cin] in memory)
            w16 = w16.contiguous(memory_format=torch.channels_last)
            y = torch.empty((x.shape[0], w16.shape[0], x.shape[2], x.shape[3]), device=x.device, dtype=torch.bfloat16,
                            memory_format=torch.channels_last)
            O.L.call("a3d_conv3x3_bn_fwd", x.data_ptr(), w16.data_ptr(), None, None, 0, y.data_ptr(), None, x.shape[0], x.shape[2], x.shape[3],
                     x.shape[1], w16.shape[0], O.L.stream())
        else:
            y = F.conv2d(x, w16, None, padding=1)
        ctx.save_for_backward(x, w16)
        ctx.cc = cc
        cc.x, cc.dw, cc.dense = x, None, False
        cc.mask, cc.ntok = None, 0
        if O.SPARSE_FPN_DGRAD and ctx.needs_input_grad[0] and O.L.load().a3d_conv3x3_tile_count(x.shape[0], x.shape[2], x.shape[3]) > 0 \
                and x.shape[2] // 8 <= 255 and x.shape[3] // 32 <= 255:
            # tile marks of this step's backward (a fill KERNEL: captured memsets replay wrong on this stack)
            cc.mask = torch.zeros((O.L.load().a3d_conv3x3_tile_count(x.shape[0], x.shape[2], x.shape[3]),), device=x.device, dtype=torch.uint8)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16 = ctx.saved_tensors
        cc = ctx.cc
        sparse = cc.dw is not None and not cc.dense
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = None
        # token-sparse input gradient: every consumer of the map was a gather that marked its tiles, and together they hold at most
        # SPARSE_FPN_DGRAD_MAX of the map's pixels (a static bound: the marked-tile count lives on the device)
        N, _, H, W = x.shape
        sparse_x = (need_x and sparse and cc.mask is not None and 0 < cc.ntok <= O.SPARSE_FPN_DGRAD_MAX * N * H * W and dy.dtype == torch.bfloat16)
        if sparse_x:
            dy = dy.contiguous(memory_format=torch.channels_last)
            wt = w16.flip(2, 3).permute(1, 2, 3, 0).contiguous()            # wt[ci][kh][kw][co] = w[co][ci][2 - kh][2 - kw]
            dx = torch.empty_like(x, memory_format=torch.channels_last)
            ws = torch.empty((O.L.load().a3d_conv3x3_dgrad_tiles_ws_ints(N, H, W),), device=x.device, dtype=torch.int32)
            O.L.call("a3d_conv3x3_dgrad_tiles", dy.data_ptr(), wt.data_ptr(), cc.mask.data_ptr(), ws.data_ptr(), dx.data_ptr(), N, H, W, O.L.stream())
            need_x = False
        if need_x or (need_w and not sparse):
            dy = dy.contiguous(memory_format=torch.channels_last)
            dxl, dw, _ = torch.ops.aten.convolution_backward(dy, x, w16, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
                                                             (need_x, need_w and not sparse, False))
            if need_x:
                dx = dxl
        if need_w and sparse:
            dw = cc.dw.permute(2, 3, 0, 1).contiguous()        # [kh][kw][co][ci] -> the weight's [co][ci][kh][kw]
        cc.dw, cc.mask = None, None
        return dx, (None if dw is None else dw.float()), None


class FeaturePyramidNetwork(nn.Module):
    """torchvision.ops.FeaturePyramidNetwork (0.14 naming: inner_blocks.i.0 / layer_blocks.i.0), restated: 1x1 lateral
    convs, nearest top-down pathway, 3x3 output convs.  Runs on PyTorch-ROCm/MIOpen (adjacent to the hot path,
    SURVEY §2a-8 / §8f-1).  `needed` restricts the 3x3 output convs to the maps the policy actually reads."""

    def __init__(self, in_channels_list, out_channels):
        super().__init__()
        self.inner_blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(c, out_channels, 1)) for c in in_channels_list])
        self.layer_blocks = nn.ModuleList(
            [nn.Sequential(nn.Conv2d(out_channels, out_channels, 3, padding=1)) for _ in in_channels_list])
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)

    def forward(self, feats, needed=None, pad_to=None, defer_output_bias=None, sparse_ncam=None):
        """pad_to: run every convolution with its output (and, for the 3x3 layer blocks, input) channel count zero-padded
        to this width and return the padded maps (pad channels are exact zeros).  MIOpen's bf16 NHWC kernels for C = 60
        are ~2x slower than for C = 64 (measured on MI355X, N = 256 at 128 x 128: forward + backward 5.2 ms vs 2.6 ms);
        the parameters keep the reference's shapes, the padding is a per-step F.pad that autograd slices back.

        Biases (bf16 CUDA maps): the lateral 1x1 convolutions run bias-free and their bias is added by the top-down kernel
        that reads the lateral map anyway (forward) / reduced by the kernel that reads its gradient anyway (backward).
        defer_output_bias=True also runs the 3x3 output convolutions bias-free: the consumer adds the bias to the token rows
        it gathers (ops.BuildContextFn) -- a level reads 6 % of the fine map.  Whenever the keyword is passed (True OR False)
        the return value is the pair (maps, {name: bias Parameter owed}); without it, the plain dict of maps.
        sparse_ncam (cameras per sample; only with defer_output_bias=True): the caller reads the output maps through
        ops.BuildContextFn gathers and passes each map's ops.SparseConvCtx on to them -- the return value is then the triple
        (maps, biases, {name: SparseConvCtx}) and the output convolutions' weight gradients come from the gathers (_LayerConv3x3Fn)."""
        names = list(feats.keys())
        xs = list(feats.values())
        C = self.inner_blocks[0][0].out_channels
        pad = 0 if pad_to is None else max(0, pad_to - C)

        def conv(m, x, wpad, with_bias, **kw):
            w = F.pad(m.weight, wpad) if pad else m.weight
            b = None
            if with_bias:
                b = F.pad(m.bias, (0, pad)) if pad else m.bias
            return F.conv2d(x, w, b, **kw)

        def inner(i, x, last):
            m = self.inner_blocks[i][0]
            wpad = (0, 0, 0, 0, 0, 0, 0, pad)
            Co = C + pad
            bf16 = x.dtype == torch.bfloat16 or (torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == torch.bfloat16)
            fuse = (x.is_cuda and bf16 and Co % 4 == 0 and 256 % (Co // 4) == 0 and x.shape[-1] % 2 == 0 and x.shape[-2] % 2 == 0
                    and (last is None or (x.shape[-2] == 2 * last.shape[-2] and x.shape[-1] == 2 * last.shape[-1])))
            if not fuse:
                lat = conv(m, x, wpad, True)
                return lat if last is None else fpn_top_down(lat, last)
            if _fused_lateral_ok(x, Co, last):                              # convolution + bias + top-down add in one launch
                return _LateralTopDownFn.apply(x, F.pad(m.weight, wpad) if pad else m.weight, m.bias, last)
            return fpn_top_down(conv(m, x, wpad, False), last, m.bias)      # bias-free convolution, bias in the top-down kernel

        out_bias, out_ctx = {}, {}

        def layer(i, x):
            m = self.layer_blocks[i][0]
            defer = defer_output_bias and x.is_cuda
            if defer:
                out_bias[names[i]] = m.bias
            if (defer and sparse_ncam and O.SPARSE_FPN_WGRAD and C + pad == 64 and x.dtype == torch.bfloat16 and x.shape[1] == 64
                    and x.is_contiguous(memory_format=torch.channels_last) and x.shape[0] % sparse_ncam == 0):
                cc = O.SparseConvCtx(sparse_ncam)
                out_ctx[names[i]] = cc
                w = F.pad(m.weight, (0, 0, 0, 0, 0, pad, 0, pad)) if pad else m.weight
                return _LayerConv3x3Fn.apply(x, w, cc)
            return conv(m, x, (0, 0, 0, 0, 0, pad, 0, pad), not defer, padding=1)

        last = inner(len(xs) - 1, xs[-1], None)
        out = {}
        lowest = min(names.index(n) for n in needed) if needed is not None else 0
        if needed is None or names[-1] in needed:
            out[names[-1]] = layer(len(xs) - 1, last)
        for i in range(len(xs) - 2, lowest - 1, -1):
            last = inner(i, xs[i], last)
            if needed is None or names[i] in needed:
                out[names[i]] = layer(i, last)
        if defer_output_bias is None:
            return out
        return (out, out_bias, out_ctx) if sparse_ncam else (out, out_bias)


class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.avgpool = nn.AvgPool2d(stride) if stride > 1 else nn.Identity()
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = None
        if stride > 1 or inplanes != planes * 4:
            self.downsample = nn.Sequential(nn.AvgPool2d(stride), nn.Conv2d(inplanes, planes * 4, 1, bias=False),
                                            nn.BatchNorm2d(planes * 4))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(self.avgpool(out)))
        return F.relu(out + (x if self.downsample is None else self.downsample(x)))


class SyntheticCLIPResNet50(nn.Module):
    """Random-init network with the layer structure of CLIP's ModifiedResNet RN50 (3-conv stem, avg-pool
    anti-aliased bottlenecks [3,4,6,3], width 64), returning res1..res5 with channels 64/256/512/1024/2048 at strides
    2/4/8/16/32 like model/utils/clip.py:22-43.  The real weights (openai/CLIP) are not available offline; the
    arithmetic cost and map shapes are the real ones.  Frozen; runs on MIOpen."""

    def __init__(self, width=64, layers=(3, 4, 6, 3)):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width // 2, 3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width // 2)
        self.conv2 = nn.Conv2d(width // 2, width // 2, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width // 2)
        self.conv3 = nn.Conv2d(width // 2, width, 3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(width)
        self.avgpool = nn.AvgPool2d(2)
        self._inplanes = width
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2)

    def _make_layer(self, planes, blocks, stride=1):
        layers = [_Bottleneck(self._inplanes, planes, stride)]
        self._inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(_Bottleneck(self._inplanes, planes))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = F.relu(self.bn1(self.conv1(x)))
        x = F.relu(self.bn2(self.conv2(x)))
        x0 = F.relu(self.bn3(self.conv3(x)))
        x1 = self.layer1(self.avgpool(x0))
        x2 = self.layer2(x1)
        x3 = self.layer3(x2)
        x4 = self.layer4(x3)
        return {"res1": x0, "res2": x1, "res3": x2, "res4": x3, "res5": x4}


class ClipNormalize(nn.Module):
    """CLIP's preprocessing normalisation (clip_transforms.transforms[-1], model/utils/clip.py:19)."""

    def __init__(self):
        super().__init__()
        self.register_buffer("mean", torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("std", torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1), persistent=False)

    def forward(self, x):
        return (x - self.mean) / self.std


def load_synthetic_clip():
    return SyntheticCLIPResNet50(), ClipNormalize()


def bn_scale_shift(x, bn, partial=None):
    """(2, C) fp32 [scale | shift] of BatchNorm2d `bn` for the bf16 channels_last activation x: batch statistics when
    bn.training (one read of x -- or none, when the producing a3d_conv1x1_bn_fwd already left its `partial` sums), running
    statistics otherwise; the finalize kernel also applies the running-stat update."""
    N, C, H, W = x.shape
    rows = N * H * W
    dev = x.device
    st = O.L.stream()
    scale = torch.empty((2, C), device=dev, dtype=torch.float32)
    train = 1 if bn.training else 0
    nslab = 1
    if train and partial is None:
        nslab = O.L.load().a3d_bn_nslab(rows, C)
        partial = torch.empty((nslab, 2, C), device=dev, dtype=torch.float32)
        O.L.call("a3d_bn_stats", x.data_ptr(), partial.data_ptr(), rows, C, nslab, st)
    elif train:
        nslab = partial.shape[0]
    O.L.call("a3d_bn_finalize", None if not train else partial.data_ptr(), nslab, rows, C, float(bn.eps),
             float(bn.momentum if bn.momentum is not None else 0.1), bn.weight.data_ptr(), bn.bias.data_ptr(),
             bn.running_mean.data_ptr(), bn.running_var.data_ptr(), scale[0].data_ptr(), scale[1].data_ptr(), train, st)
    return scale


def _conv1x1_operands(x, conv, in_scale, in_relu):
    """The operand checks every 1x1 entry point shares and (M, K, Cout, pointer of the (Cout, K) weight, the (in_scale, in_shift,
    in_relu) argument triple of the producer's BatchNorm-apply on the operand load)."""
    N, K, H, W = x.shape
    Cout = conv.weight.shape[0]
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    assert conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.bias is None and conv.weight.dtype == torch.bfloat16
    w2 = conv.weight.reshape(Cout, K)
    assert w2.is_contiguous()                                      # (a view: the pointer is the weight's own)
    pre = (None, None) if in_scale is None else (in_scale[0].data_ptr(), in_scale[1].data_ptr())
    return N * H * W, K, Cout, w2.data_ptr(), pre + (1 if in_relu else 0,)


def conv1x1_bn(x, conv, in_scale=None, in_relu=False, want_stats=True, store=True):
    """1x1 stride-1 convolution of a bf16 channels_last activation as the fused GEMM of csrc/conv1x1.hip: optional
    BatchNorm-apply (+ ReLU) of the producer on the input (`in_scale` = bn_scale_shift of that layer), and the partial
    statistics of the output for the BatchNorm that follows.  Returns (y, partial or None).  store=False (the bottleneck's conv3
    shapes, a3d_conv1x1_bn_residual_serves): the same kernel and the same sums of the bf16-rounded outputs, nothing stored
    (a3d_conv1x1_bn_fwd with y = NULL) -- returns (None, partial)."""
    M, K, Cout, w, pre = _conv1x1_operands(x, conv, in_scale, in_relu)
    assert store or want_stats
    y = partial = None
    if store:
        y = torch.empty((x.shape[0], Cout) + x.shape[2:], device=x.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    if want_stats:
        partial = torch.empty((O.L.load().a3d_conv1x1_nslab(M, K, Cout), 2, Cout), device=x.device, dtype=torch.float32)
    O.L.call("a3d_conv1x1_bn_fwd", x.data_ptr(), w, *pre, None if y is None else y.data_ptr(),
             None if partial is None else partial.data_ptr(), M, K, Cout, O.L.stream())
    return y, partial


def conv1x1_gram_stats(x, conv, in_scale=None, in_relu=False):
    """(1, 2, Cout) fp32 (sum, sum of squares) over rows of the OUTPUT of the 1x1 convolution `conv` on the bf16 channels_last x
    (with the producer's BatchNorm-apply `in_scale` folded in as conv1x1_bn folds it), computed from the K x K Gram matrix of its
    INPUT (csrc/bn_gram.hip): the record bn_scale_shift(partial=...) finalizes -- the statistics exist before the convolution runs."""
    M, K, Cout, w, pre = _conv1x1_operands(x, conv, in_scale, in_relu)
    dev, st = x.device, O.L.stream()
    nslab = O.L.load().a3d_bn_gram_nslab(M, K)
    part = torch.empty((nslab * (K * K + K),), device=dev, dtype=torch.float32)
    gpart, spart = part[:nslab * K * K], part[nslab * K * K:]
    work = torch.empty((K * K + K,), device=dev, dtype=torch.float64)
    stats = torch.empty((1, 2, Cout), device=dev, dtype=torch.float32)
    O.L.call("a3d_bn_gram", x.data_ptr(), *pre, gpart.data_ptr(), spart.data_ptr(), M, K, nslab, st)
    O.L.call("a3d_bn_gram_stats", gpart.data_ptr(), spart.data_ptr(), nslab, w, K, Cout, work.data_ptr(), stats.data_ptr(), st)
    return stats


def conv1x1_bn_residual(x, conv, out_scale, residual, in_scale=None, in_relu=False, residual_scale=None, relu=True, out=None,
                        round_conv=False):
    """relu?(bn(conv(f(x))) + r) in ONE launch (a3d_conv1x1_bn_residual_fwd): the 1x1 convolution of conv1x1_bn with the BatchNorm-apply
    of its OWN output (`out_scale` = bn_scale_shift of conv1x1_gram_stats), the residual add (`residual_scale`: the folded BatchNorm of
    the downsample branch) and the ReLU as its epilogue, one rounding from the fp32 accumulator; the raw convolution output is never
    written.  round_conv: the accumulator is rounded to bf16 first -- with `out_scale` from conv1x1_bn(store=False) the result is
    conv1x1_bn + bn_act's, bit for bit.  out: a preallocated tensor for the result."""
    M, K, Cout, w, pre = _conv1x1_operands(x, conv, in_scale, in_relu)
    assert residual.shape == (x.shape[0], Cout) + x.shape[2:] and residual.dtype == torch.bfloat16 and \
        residual.is_contiguous(memory_format=torch.channels_last)
    if out is not None:
        assert out.shape == residual.shape and out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last)
    y = out if out is not None else torch.empty_like(residual)
    O.L.call("a3d_conv1x1_bn_residual_fwd", x.data_ptr(), w, *pre, out_scale[0].data_ptr(), out_scale[1].data_ptr(),
             residual.data_ptr(), None if residual_scale is None else residual_scale[0].data_ptr(),
             None if residual_scale is None else residual_scale[1].data_ptr(), 1 if relu else 0, 1 if round_conv else 0, y.data_ptr(),
             M, K, Cout, O.L.stream())
    return y


def _conv3x3_ok(conv, Cin, H, W):
    """the structure of `conv` and the (Cin, H, W) of its input are what a3d_conv3x3_bn_fwd serves"""
    return bool(conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1) and
                conv.groups == 1 and conv.bias is None and O.L.load().a3d_conv3x3_serves(Cin, conv.out_channels, H, W))


def conv3x3_serves(x, conv):
    """the 3x3 convolution `conv` on the bf16 channels_last map x is one a3d_conv3x3_bn_fwd serves (stride 1, padding 1, no bias,
    32 -> 32 / 32 -> 64 / 64 -> 64 channels, H % 8 == 0, W % 32 == 0)"""
    return conv.weight.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and _conv3x3_ok(conv, x.shape[1], x.shape[2], x.shape[3])


def conv3x3_bn(x, conv, in_scale=None, in_relu=False, want_stats=True):
    """3x3 stride-1 padding-1 convolution of a bf16 channels_last activation as the implicit GEMM of csrc/conv3x3.hip: optional
    BatchNorm-apply (+ ReLU) of the producer on the input (`in_scale` = bn_scale_shift of that layer; the zero padding is applied
    after it, as F.conv2d pads the normalised map), and the partial statistics of the output for the BatchNorm that follows.
    Returns (y, partial or None)."""
    N, Cin, H, W = x.shape
    Cout = conv.weight.shape[0]
    assert x.is_contiguous(memory_format=torch.channels_last) and conv3x3_serves(x, conv)
    wt = conv.weight
    assert wt.is_contiguous(memory_format=torch.channels_last)        # [Cout][3][3][Cin] in memory
    y = torch.empty((N, Cout, H, W), device=x.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    partial = None
    if want_stats:
        partial = torch.empty((O.L.load().a3d_conv3x3_nslab(N, H, W, Cin, Cout), 2, Cout), device=x.device, dtype=torch.float32)
    O.L.call("a3d_conv3x3_bn_fwd", x.data_ptr(), wt.data_ptr(), None if in_scale is None else in_scale[0].data_ptr(),
             None if in_scale is None else in_scale[1].data_ptr(), 1 if in_relu else 0, y.data_ptr(),
             None if partial is None else partial.data_ptr(), N, H, W, Cin, Cout, O.L.stream())
    return y, partial


FUSED_STEM = os.environ.get("A3D_FUSED_STEM", "1") == "1"


def stem_serves(x, conv, normalize):
    """conv1 of the CLIP stem on the raw fp32 images x with ClipNormalize in front is one a3d_stem_conv_bn_fwd serves"""
    return bool(FUSED_STEM and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.is_contiguous() and
                isinstance(normalize, ClipNormalize) and conv.weight.dtype == torch.bfloat16 and
                _stem_conv_ok(conv, x.shape[0], x.shape[2], x.shape[3]))


def stem_conv_bn(x, conv, normalize, want_stats=True):
    """CLIP normalisation + the stem's strided conv1 + the partial statistics of its output in one launch (csrc/stem.hip): the
    normalised bf16 image is never written, the 268 MB output never re-read for its BatchNorm.  Returns (y, partial or None)."""
    N, _, H, W = x.shape
    w2 = conv.weight.reshape(32, 27)                 # [co][ci][kh][kw] whatever the memory format of the 4-d weight
    if not w2.is_contiguous():
        w2 = conv.weight.contiguous().reshape(32, 27)
    y = torch.empty((N, 32, H // 2, W // 2), device=x.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    partial = None
    if want_stats:
        partial = torch.empty((O.L.load().a3d_stem_conv_nslab(N, H, W), 2, 32), device=x.device, dtype=torch.float32)
    O.L.call("a3d_stem_conv_bn_fwd", x.data_ptr(), normalize.mean.reshape(-1).contiguous().data_ptr(),
             normalize.std.reshape(-1).contiguous().data_ptr(), w2.data_ptr(), y.data_ptr(), None if partial is None else partial.data_ptr(),
             N, H, W, O.L.stream())
    return y, partial


def bn_act(x, bn, relu=True, residual=None, pool=False, keep_full=True, partial=None, residual_scale=None, out=None):
    """Fused BatchNorm2d (batch statistics when bn.training, running-stat update) + optional residual add + ReLU on a
    bf16 channels_last activation (vision.hip).  Three launches: stats (skipped when the producer left `partial` sums),
    finalize, apply.  pool=True also applies the nn.AvgPool2d(2) that follows in the CLIP ResNet inside the apply kernel and
    returns (full, pooled); full is None when keep_full=False.  bn=None: no normalisation (plain 2x2 average pool of x).
    out: a preallocated tensor for the full-resolution result (the backbone's returned maps, run_frozen_backbone(out=...))."""
    N, C, H, W = x.shape
    if out is not None:
        assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous(memory_format=torch.channels_last)
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    if residual is not None:
        assert residual.shape == x.shape and residual.dtype == x.dtype and \
            residual.is_contiguous(memory_format=torch.channels_last)
    rows = N * H * W
    dev = x.device
    st = O.L.stream()
    sc_ptr = sh_ptr = None
    if bn is not None:
        scale = bn_scale_shift(x, bn, partial)
        sc_ptr, sh_ptr = scale[0].data_ptr(), scale[1].data_ptr()
    res_ptr = None if residual is None else residual.data_ptr()
    if not pool:
        y = out if out is not None else torch.empty_like(x)
        O.L.call("a3d_bn_apply", x.data_ptr(), res_ptr, None if residual_scale is None else residual_scale[0].data_ptr(),
                 None if residual_scale is None else residual_scale[1].data_ptr(), sc_ptr, sh_ptr, y.data_ptr(), rows, C,
                 1 if relu else 0, st)
        return y
    assert residual_scale is None, "the pooled apply takes a materialised residual"
    y = (out if out is not None else torch.empty_like(x)) if keep_full else None
    yp = torch.empty((N, C, H // 2, W // 2), device=dev, dtype=x.dtype, memory_format=torch.channels_last)
    O.L.call("a3d_bn_apply_pool2", x.data_ptr(), res_ptr, sc_ptr, sh_ptr, None if y is None else y.data_ptr(), yp.data_ptr(),
             N, H, W, C, 1 if relu else 0, st)
    return y, yp


def _is_pool(m, k):
    return isinstance(m, nn.AvgPool2d) and m.kernel_size in (k, (k, k))


def _pool2_ok(m, hw):
    """m is the nn.AvgPool2d(2) of a stride-2 CLIP bottleneck and the map has even spatial size hw (else: torch's pool)."""
    return _is_pool(m, 2) and hw[0] % 2 == 0 and hw[1] % 2 == 0


def _out_hw(m, hw):
    """spatial size of module m's output for an input of size hw (nn.Conv2d, nn.AvgPool2d or nn.Identity)"""
    if isinstance(m, nn.Identity):
        return hw
    k, s, p = ((v, v) if isinstance(v, int) else v for v in (m.kernel_size, m.stride, m.padding))
    return (hw[0] + 2 * p[0] - k[0]) // s[0] + 1, (hw[1] + 2 * p[1] - k[1]) // s[1] + 1


# The stem's route.  conv1: "stem_conv" (a3d_stem_conv_bn_fwd on the raw images: normalisation + convolution + statistics) | "library";
# conv2, conv3: "fused" (a3d_conv3x3_bn_fwd, the producer's BatchNorm on its operand load) | "library" (a3d_bn_apply + the library);
# stats: per BatchNorm "epilogue" (the producing kernel left them) | "bn_stats" | "none" (eval); final: "bn_apply_pool2" (res1 and its
# pooled map in one launch) | "bn_apply" (+ torch's pool)
StemRoute = collections.namedtuple("StemRoute", ("conv1", "conv2", "conv3", "stats", "final"))


class BlockRoute(collections.namedtuple("BlockRoute", (
        "name", "conv1", "stats1", "conv2", "stats2", "bn2", "conv3", "stats3", "ds_input", "ds_conv", "ds_stats", "ds_bn", "final", "writes"))):
    """One bottleneck's route.
      name      "layer2[0]"
      conv1     "gemm" (a3d_conv1x1_bn_fwd) | "library"
      conv2     "fused" (a3d_conv3x3_bn_fwd with bn1 + ReLU on its operand load) | "library" (a3d_bn_apply + the library)
      bn2       "conv3_prologue" (rides on conv3's operand load) | "bn_apply_pool2" (the pooled map only) | "bn_apply+torch_pool" | "bn_apply"
      conv3     "residual" (a3d_conv1x1_bn_residual_fwd; its prologue is bn2 == "conv3_prologue", none on an already pooled input) |
                "gemm" (a3d_conv1x1_bn_fwd with statistics) | "library"
      stats1, stats2, ds_stats   "epilogue" (the producing kernel left them) | "bn_stats" | "none" (eval)
      stats3    those, or on the residual route "stats_pass" (a3d_conv1x1_bn_fwd that stores nothing) | "gram" (a3d_bn_gram + a3d_bn_gram_stats)
      ds_input  None (no downsample branch) | "producer_pooled" (the previous block's a3d_bn_apply_pool2 emitted it) | "pool2" (pool-only
                a3d_bn_apply_pool2) | "identity" (AvgPool2d(1)) | "torch_pool"
      ds_conv   None | "gemm" | "library"
      ds_bn     None | "folded" (into the final apply or epilogue) | "materialised" (a3d_bn_apply of its own)
      final     "conv3_epilogue" (round-first: bit for bit a3d_bn_apply's) | "conv3_epilogue_gram" (one rounding from the accumulator) |
                "bn_apply" | "bn_apply_pool2" (also emits the pooled map for the next block's downsample branch)
      writes    "res2" .. "res5" for a layer's last block, else None"""
    __slots__ = ()

    def launches(self):
        """entry-point names the block launches, in order"""
        scale = lambda stats: ["a3d_bn_stats"] * (stats == "bn_stats") + ["a3d_bn_finalize"]
        gemm = lambda route: ["a3d_conv1x1_bn_fwd"] * (route == "gemm")
        seq = gemm(self.conv1) + scale(self.stats1) + ["a3d_conv3x3_bn_fwd" if self.conv2 == "fused" else "a3d_bn_apply"] + scale(self.stats2)
        if self.bn2 != "conv3_prologue":
            seq += ["a3d_bn_apply_pool2" if self.bn2 == "bn_apply_pool2" else "a3d_bn_apply"]
        seq += gemm(self.conv3)
        if self.ds_input is not None:
            seq += ["a3d_bn_apply_pool2"] * (self.ds_input == "pool2") + gemm(self.ds_conv) + scale(self.ds_stats)
            seq += ["a3d_bn_apply"] * (self.ds_bn == "materialised")
        if self.conv3 == "residual":
            stats = {"stats_pass": ["a3d_conv1x1_bn_fwd"], "gram": ["a3d_bn_gram", "a3d_bn_gram_stats"], "none": []}[self.stats3]
            return seq + stats + ["a3d_bn_finalize", "a3d_conv1x1_bn_residual_fwd"]
        return seq + scale(self.stats3) + ["a3d_" + self.final]


class BackbonePlan(collections.namedtuple("BackbonePlan", ("stem", "blocks", "bns"))):
    """stem: StemRoute; blocks: one BlockRoute per bottleneck in execution order; bns: the dotted names of the BatchNorm modules the
    forward passes through (their num_batches_tracked advance in training mode)"""
    __slots__ = ()

    def launches(self):
        """entry-point names of the whole forward, in order (conv1 == "library": from the normalised bf16 image on)"""
        s, scale = self.stem, lambda stats: ["a3d_bn_stats"] * (stats == "bn_stats") + ["a3d_bn_finalize"]
        seq = ["a3d_stem_conv_bn_fwd"] * (s.conv1 == "stem_conv")
        for route, stats in zip((s.conv2, s.conv3), s.stats):
            seq += scale(stats) + ["a3d_conv3x3_bn_fwd" if route == "fused" else "a3d_bn_apply"]
        seq += scale(s.stats[2]) + ["a3d_" + s.final]
        return seq + [e for b in self.blocks for e in b.launches()]


def _stem_conv_ok(conv, images, H, W):
    """conv is the CLIP stem's strided conv1 and a3d_stem_conv_bn_fwd serves (images, H, W)"""
    return bool(isinstance(conv, nn.Conv2d) and conv.in_channels == 3 and conv.out_channels == 32 and conv.kernel_size == (3, 3) and
                conv.stride == (2, 2) and conv.padding == (1, 1) and conv.bias is None and O.L.load().a3d_stem_conv_nslab(images, H, W) > 0)


def backbone_plan(bb, images, H, W, fused_stem=None):
    """Which launches serve a fused_frozen_backbone_forward call, from host values alone: the SyntheticCLIPResNet50 `bb` (only its
    structure and each BatchNorm's `training` bit are read: it may live on the CPU) on `images` raw images of H x W.  The module
    switches FUSED_CONV1X1, FUSED_CONV3X3, FUSED_CONV3_RESIDUAL, FOLD_DOWNSAMPLE_BN and (unless the caller says whether the stem kernel
    ran: fused_stem) FUSED_STEM are read here, at call time.  Assumes what run_frozen_backbone establishes (bf16 convolution weights,
    channels_last bf16 maps); nothing is allocated or launched -- the library answers the shape queries a3d_stem_conv_nslab,
    a3d_conv3x3_serves, a3d_conv1x1_streams (which follows a3d_conv1x1_deep_mode) and a3d_conv1x1_bn_residual_serves on the host."""
    fused_stem = FUSED_STEM if fused_stem is None else fused_stem
    fuse1, fuse3, res_mode, fold = FUSED_CONV1X1, FUSED_CONV3X3, FUSED_CONV3_RESIDUAL, FOLD_DOWNSAMPLE_BN
    lib = O.L.load()
    stats = lambda own, bn: "none" if not bn.training else ("epilogue" if own else "bn_stats")
    plain1x1 = lambda m: m.kernel_size == (1, 1) and m.stride == (1, 1)
    # the route predicates: m a convolution, hw the spatial size of its input
    c3x3 = lambda m, hw: "fused" if fuse3 and _conv3x3_ok(m, m.in_channels, hw[0], hw[1]) else "library"
    c1x1 = lambda m: "gemm" if fuse1 and plain1x1(m) and lib.a3d_conv1x1_streams(m.in_channels, m.out_channels) else "library"
    res_ok = lambda m: bool(res_mode and fuse1 and plain1x1(m) and m.bias is None and
                            lib.a3d_conv1x1_bn_residual_serves(m.in_channels, m.out_channels))

    conv1 = "stem_conv" if fused_stem and _stem_conv_ok(bb.conv1, images, H, W) else "library"
    hw = _out_hw(bb.conv1, (H, W))
    conv2 = c3x3(bb.conv2, hw)
    hw = _out_hw(bb.conv2, hw)
    conv3 = c3x3(bb.conv3, hw)
    hw = _out_hw(bb.conv3, hw)
    pool2 = _pool2_ok(bb.avgpool, hw)
    stem = StemRoute(conv1, conv2, conv3, (stats(conv1 == "stem_conv", bb.bn1), stats(conv2 == "fused", bb.bn2), stats(conv3 == "fused", bb.bn3)),
                     "bn_apply_pool2" if pool2 else "bn_apply")
    hw = _out_hw(bb.avgpool, hw)

    bns = ["bn1", "bn2", "bn3"]
    named = [("layer%d" % (li + 1), bi, blk) for li in range(4) for bi, blk in enumerate(getattr(bb, "layer%d" % (li + 1)))]
    routes, have_pooled = [], False                    # have_pooled: the producer of the block's input also emitted AvgPool2d(2) of it
    for i, (layer, bi, blk) in enumerate(named):
        nxt = named[i + 1][2] if i + 1 < len(named) else None
        r1 = c1x1(blk.conv1)
        hw1 = _out_hw(blk.conv1, hw)
        r2 = c3x3(blk.conv2, hw1)
        hw2 = _out_hw(blk.conv2, hw1)
        no_pool = isinstance(blk.avgpool, nn.Identity) or _is_pool(blk.avgpool, 1)
        hw3 = hw2 if no_pool else _out_hw(blk.avgpool, hw2)             # conv3's input and the block's output
        # the next block's downsample branch wants the pooled output: the final a3d_bn_apply_pool2 emits it, so conv3 keeps its raw map
        pooled_next = nxt is not None and nxt.downsample is not None and _pool2_ok(nxt.downsample[0], hw3)
        r3 = "residual" if not pooled_next and res_ok(blk.conv3) else c1x1(blk.conv3)
        if no_pool and r3 != "library":
            bn2 = "conv3_prologue"
        else:
            bn2 = "bn_apply_pool2" if _pool2_ok(blk.avgpool, hw2) else "bn_apply" if no_pool else "bn_apply+torch_pool"
        if r3 == "residual":
            st3 = "none" if not blk.bn3.training else "gram" if res_mode == "gram" else "stats_pass"
            final = "conv3_epilogue_gram" if res_mode == "gram" else "conv3_epilogue"
        else:
            st3, final = stats(r3 == "gemm", blk.bn3), "bn_apply_pool2" if pooled_next else "bn_apply"
        ds_input = ds_conv = ds_stats = ds_bn = None
        if blk.downsample is not None:
            dpool, dconv, dbn = blk.downsample
            ds_input = "producer_pooled" if have_pooled else "pool2" if _pool2_ok(dpool, hw) else "identity" if _is_pool(dpool, 1) else "torch_pool"
            ds_conv = c1x1(dconv)
            ds_stats = stats(ds_conv == "gemm", dbn)
            ds_bn = "folded" if fold and final != "bn_apply_pool2" else "materialised"       # (the pooled apply takes a materialised residual)
            bns.append("%s.%d.downsample.2" % (layer, bi))
        bns += ["%s.%d.bn%d" % (layer, bi, j) for j in (1, 2, 3)]
        last = bi == len(getattr(bb, layer)) - 1
        routes.append(BlockRoute("%s[%d]" % (layer, bi), r1, stats(r1 == "gemm", blk.bn1), r2, stats(r2 == "fused", blk.bn2), bn2, r3, st3,
                                 ds_input, ds_conv, ds_stats, ds_bn, final, "res%d" % (int(layer[-1]) + 1) if last else None))
        hw, have_pooled = hw3, final == "bn_apply_pool2"
    return BackbonePlan(stem, tuple(routes), tuple(bns))


def fused_frozen_backbone_forward(bb, x, stem=None, out=None):
    """SyntheticCLIPResNet50.forward with MIOpen bf16 NHWC convolutions and the fused BatchNorm of vision.hip.
    Same dataflow as the module's own forward (CLIP ModifiedResNet, model/utils/clip.py:28-43); every AvgPool2d(2) is
    folded into the BatchNorm-apply kernel that produces its input (the block output also feeds the next block's
    downsample branch pooled, so that kernel emits both).  Runs what backbone_plan decides for its input: every step below
    dispatches on the record's strings.  x: the normalised bf16 channels_last images, or None with stem = (raw output of conv1,
    partial statistics) from stem_conv_bn.  out: {res1..res5} preallocated maps the five returned maps are written into by the
    kernels that produce them (no copy)."""
    c1, p1 = stem if stem is not None else (None, None)
    images, H, W = (c1.shape[0], 2 * c1.shape[2], 2 * c1.shape[3]) if stem is not None else (x.shape[0], x.shape[2], x.shape[3])
    plan = backbone_plan(bb, images, H, W, fused_stem=stem is not None)
    assert (plan.stem.conv1 == "stem_conv") == (stem is not None)
    # what the plan assumes of its input and of the frozen weights (run_frozen_backbone converts them once)
    src = c1 if stem is not None else x
    assert src.dtype == torch.bfloat16 and src.is_contiguous(memory_format=torch.channels_last)
    assert all(m.weight.dtype == torch.bfloat16 for m in bb.modules() if isinstance(m, nn.Conv2d))
    maps = {} if out is None else out
    conv = lambda m, t: F.conv2d(t, m.weight, None, m.stride, m.padding)

    def conv3x3(route, m, t, bn_in, p_in, want_stats):
        """3x3 convolution m of relu(bn_in(t)) (t = the raw output of the previous convolution, p_in its partial statistics or
        None) + the partial statistics of its own output: one a3d_conv3x3_bn_fwd -- relu(bn_in(t)) is then never materialised --
        or BatchNorm-apply + MIOpen"""
        if route == "fused":
            return conv3x3_bn(t, m, in_scale=bn_scale_shift(t, bn_in, p_in), in_relu=True, want_stats=want_stats)
        return conv(m, bn_act(t, bn_in, partial=p_in)), None

    def conv1x1(route, m, t, **kw):
        """1x1 convolution + the partial statistics of its output (None on the MIOpen path)"""
        return conv1x1_bn(t, m, **kw) if route == "gemm" else (conv(m, t), None)

    s = plan.stem
    if stem is None:
        c1 = conv(bb.conv1, x)
    c2, p2 = conv3x3(s.conv2, bb.conv2, c1, bb.bn1, p1, bb.bn2.training)
    c3, p3 = conv3x3(s.conv3, bb.conv3, c2, bb.bn2, p2, bb.bn3.training)
    if s.final == "bn_apply_pool2":
        x0, x = bn_act(c3, bb.bn3, pool=True, partial=p3, out=maps.get("res1"))
    else:
        x0 = bn_act(c3, bb.bn3, partial=p3, out=maps.get("res1"))
        x = bb.avgpool(x0)
    outs = {"res1": x0}
    x_pooled = None                                    # AvgPool2d(2)(x), when the producer of x already emitted it
    blocks = [blk for layer in (bb.layer1, bb.layer2, bb.layer3, bb.layer4) for blk in layer]
    for r, blk in zip(plan.blocks, blocks):
        c1, p1 = conv1x1(r.conv1, blk.conv1, x, want_stats=blk.bn1.training)
        c2, p2 = conv3x3(r.conv2, blk.conv2, c1, blk.bn1, p1, blk.bn2.training)
        # a3 (+ a3_scale): conv3's input (+ its pending BatchNorm-apply, which then rides on conv3's operand load: c2 is never rewritten)
        a3_scale = None
        if r.bn2 == "conv3_prologue":
            a3, a3_scale = c2, bn_scale_shift(c2, blk.bn2, p2)
        elif r.bn2 == "bn_apply_pool2":
            a3 = bn_act(c2, blk.bn2, pool=True, keep_full=False, partial=p2)[1]
        else:
            a3 = blk.avgpool(bn_act(c2, blk.bn2, partial=p2))
        pre = dict(in_scale=a3_scale, in_relu=a3_scale is not None)
        if r.conv3 != "residual":
            o3, p3 = conv1x1(r.conv3, blk.conv3, a3, want_stats=blk.bn3.training, **pre)
        idn, idn_scale = x, None
        if r.ds_input is not None:
            dpool, dconv, dbn = blk.downsample
            if r.ds_input == "producer_pooled":
                xin = x_pooled
            elif r.ds_input == "pool2":
                xin = bn_act(x, None, relu=False, pool=True, keep_full=False)[1]
            else:
                xin = x if r.ds_input == "identity" else dpool(x)
            cd, pd = conv1x1(r.ds_conv, dconv, xin, want_stats=dbn.training)
            if r.ds_bn == "folded":
                # the branch's BatchNorm rides in the block's final apply: bn_d(cd) is never materialised
                idn, idn_scale = cd, bn_scale_shift(cd, dbn, pd)
            else:
                idn = bn_act(cd, dbn, relu=False, partial=pd)
        o_x, x_pooled = maps.get(r.writes), None               # a layer's last block writes the returned map
        if r.conv3 == "residual":
            # bn3's statistics first (none in eval mode) -- the sums of the bf16-rounded conv3 outputs from a pass of the GEMM that stores
            # nothing, or ("gram") of the unrounded product from the Gram matrix of conv3's input --, then conv3 + bn3 + add + ReLU in
            # one launch: the raw conv3 map is never written
            st3 = None
            if r.stats3 == "gram":
                st3 = conv1x1_gram_stats(a3, blk.conv3, **pre)
            elif r.stats3 == "stats_pass":
                st3 = conv1x1_bn(a3, blk.conv3, store=False, **pre)[1]
            sc3 = bn_scale_shift(idn, blk.bn3, partial=st3)        # (idn has conv3's output shape: rows and channels)
            x = conv1x1_bn_residual(a3, blk.conv3, sc3, idn, residual_scale=idn_scale, relu=True, out=o_x,
                                    round_conv=r.final == "conv3_epilogue", **pre)
        elif r.final == "bn_apply_pool2":
            x, x_pooled = bn_act(o3, blk.bn3, relu=True, residual=idn, pool=True, partial=p3, out=o_x)
        else:
            x = bn_act(o3, blk.bn3, relu=True, residual=idn, partial=p3, residual_scale=idn_scale, out=o_x)
        if r.writes is not None:
            outs[r.writes] = x
    if bb.training:
        torch._foreach_add_([bb.get_submodule(n).num_batches_tracked for n in plan.bns], 1)
    return outs


FUSED_BN = os.environ.get("A3D_FUSED_BN", "1") == "1"
# BatchNorm of the bottleneck's downsample branch applied inside the block's final BatchNorm-apply + add + ReLU kernel (a second
# scale / shift pair on the residual operand) instead of its own pass.  A3D_FOLD_DS_BN=0: the branch's map is materialised (A/B).
FOLD_DOWNSAMPLE_BN = os.environ.get("A3D_FOLD_DS_BN", "1") not in ("0", "", "off")
# conv3 of the layer-1 / layer-2 bottlenecks with bn3 + residual add + ReLU as its epilogue (a3d_conv1x1_bn_residual_fwd): bn3's batch
# statistics exist before the GEMM that applies them runs, so the raw conv3 map is never written and re-read by the final
# BatchNorm-apply.  True (default): the statistics of the bf16-ROUNDED conv3 outputs from a pass of the GEMM that stores nothing, and
# an epilogue that rounds the accumulator first -- the block output is the unfused path's, bit for bit.  "gram"
# (A3D_FUSED_CONV3_RES=gram): the statistics of the unrounded product from the K x K Gram matrix of conv3's INPUT (a3d_bn_gram) and
# one rounding from the accumulator: cheaper (no second GEMM), and every block output moves by up to a bf16 ulp -- which the deep
# layers of this network amplify to tens of percent of res5's rms, like any other perturbation of that size.
# A3D_FUSED_CONV3_RES=0: conv3 + a3d_bn_apply as before (A/B).
_c3r = os.environ.get("A3D_FUSED_CONV3_RES", "1")
FUSED_CONV3_RESIDUAL = False if _c3r in ("0", "", "off") else ("gram" if _c3r == "gram" else True)
# The backbone's 1x1 convolutions of the HBM-bound layers (1 and 2: K <= 256, the shapes a3d_conv1x1_streams accepts) through
# a3d_conv1x1_bn_fwd, with BatchNorm-apply of the producer and the statistics of the consumer folded into the GEMM; the deep,
# compute-bound layers stay on MIOpen (profiles/r04_conv1x1_layers.json).  A3D_FUSED_CONV1X1=0: MIOpen everywhere (A/B).
FUSED_CONV1X1 = os.environ.get("A3D_FUSED_CONV1X1", "1") not in ("0", "", "off")
# The 3x3 convolutions with <= 64 channels (the stem's conv2 / conv3, layer1's conv2) through a3d_conv3x3_bn_fwd, with BatchNorm-apply
# of the producer and the statistics of the consumer folded in; wider layers stay on MIOpen.  A3D_FUSED_CONV3X3=0: MIOpen (A/B).
FUSED_CONV3X3 = os.environ.get("A3D_FUSED_CONV3X3", "1") not in ("0", "", "off")


def normalize_to_nhwc_bf16(x, normalize):
    """ClipNormalize + channels-last + bf16 cast of the raw images (N, 3, H, W) fp32 in one kernel (vision.hip)."""
    x = x.float().contiguous()
    N, _, H, W = x.shape
    y = torch.empty((N, 3, H, W), device=x.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    O.L.call("a3d_rgb_normalize_nhwc_bf16", x.data_ptr(), normalize.mean.data_ptr(), normalize.std.data_ptr(), y.data_ptr(), N, H, W,
             O.L.stream())
    return y


def run_frozen_backbone(backbone, x, dtype, keep_dtype=False, normalize=None, out=None):
    """Forward of the frozen backbone under no_grad.  `normalize`: the ClipNormalize module when `x` are the RAW images
    (None: already normalised).  For a reduced dtype the convolution weights are converted ONCE
    (the backbone is frozen, so there is no master copy to keep) instead of being re-cast by autocast at every step;
    BatchNorm keeps fp32 parameters / running statistics and, as in the reference's train() mode, batch statistics.
    On the GPU with bf16 the BatchNorm + ReLU + residual chain runs as the fused HIP kernels of vision.hip.
    out: {res1..res5} preallocated maps (as a previous call returned them) to write the result into -- the fused path's kernels
    write them directly, the other paths copy."""
    def deliver(feats):
        if out is None:
            return feats
        for k, v in feats.items():
            if v.data_ptr() != out[k].data_ptr():
                out[k].copy_(v)
        return out
    fused = FUSED_BN and x.is_cuda and dtype == torch.bfloat16 and isinstance(backbone, SyntheticCLIPResNet50)
    if normalize is not None and not (fused and isinstance(normalize, ClipNormalize) and (x.shape[-1] * x.shape[-2]) % 4 == 0):
        x = normalize(x).contiguous(memory_format=torch.channels_last)
        normalize = None
    if dtype == torch.float32:
        return deliver(backbone(x))
    if getattr(backbone, "_conv_dtype", None) != dtype:
        for m in backbone.modules():
            if isinstance(m, nn.Conv2d):
                m.to(dtype)
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
        backbone._conv_dtype = dtype
    if fused:
        if normalize is not None and stem_serves(x, backbone.conv1, normalize):
            feats = fused_frozen_backbone_forward(backbone, None, stem=stem_conv_bn(x, backbone.conv1, normalize, want_stats=backbone.bn1.training),
                                                  out=out if keep_dtype else None)
        else:
            xb = normalize_to_nhwc_bf16(x, normalize) if normalize is not None else x.to(dtype).contiguous(memory_format=torch.channels_last)
            feats = fused_frozen_backbone_forward(backbone, xb, out=out if keep_dtype else None)
    else:
        feats = backbone(x.to(dtype))
    return deliver(feats if keep_dtype else {k: v.float() for k, v in feats.items()})
