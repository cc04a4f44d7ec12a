"""Autograd-level operators of the hot path: thin torch.autograd.Function wrappers that pair the forward and
backward launches of libact3d_hip.so.  PyTorch only provides device memory, the stream and the autograd tape.

Parameter gradients are accumulated by the wgrad kernels straight into ``param.grad`` (the flat gradient buffer
when the model is wrapped by ``FlatParams``) instead of being returned through autograd; see DESIGN.md.
"""
import collections
import ctypes
import math
import os

import torch

from . import lib as L

F32 = torch.float32
QKW = 48      # bf16 elements per q / k operand row: hi(16) | lo(16) | lo2(16)  (a3d_common.h)


def ceil_to(x, m):
    return (x + m - 1) // m * m


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _or_empty(device, *ts):          # optional tensors (xyz, key mask) for save_for_backward: empty for None, a flag in ctx.meta says so
    return tuple(torch.empty(0, device=device) if t is None else t for t in ts)


def _or_none(present, *ts):
    return ts if present else (None,) * len(ts)


def grad_buf(p):
    """The tensor wgrad kernels accumulate into for parameter ``p`` (created zeroed on first use)."""
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


_freq_cache = {}


def rope_freq(E, device):
    """div_term of RotaryPositionEncoding3D (position_encodings.py:72-75), evaluated with the same torch ops."""
    key = (E, str(device))
    if key not in _freq_cache:
        _freq_cache[key] = torch.exp(
            torch.arange(0, E // 3, 2, dtype=F32, device=device) * (-math.log(10000.0) / (E // 3))).contiguous()
    return _freq_cache[key]


# ------------------------------------------------------------------------------------------------ raw launchers
# the nn.Dropout behind a Linear / in front of a post-norm applied by the producing kernel (same bits as the separate a3d_dropout
# launch, 84 launches fewer per ChainedDiffuser training step); A3D_DROPOUT_FOLD=0: separate launches (the A/B and test switch)
DROP_FOLD = os.environ.get("A3D_DROPOUT_FOLD", "1") != "0"


def linear_raw(x_ptr, ldx, W_ptr, ldw, b_ptr, M, N, K, device, act=0, mask_ptr=None, ldm=0, transposed=False,
               out=None, drop=None, site=0):
    """drop / site: DropCtx and site of an nn.Dropout applied to the result (None: none)."""
    y = out if out is not None else torch.empty((M, N), device=device, dtype=F32)
    if drop is not None and DROP_FOLD:
        L.call("a3d_linear_fwd_drop", x_ptr, ldx, W_ptr, ldw, b_ptr, y.data_ptr(), N, mask_ptr, ldm, M, N, K, act,
               1 if transposed else 0, drop.state.data_ptr(), int(site), drop.p, L.stream())
        return y
    L.call("a3d_linear_fwd", x_ptr, ldx, W_ptr, ldw, b_ptr, y.data_ptr(), N, mask_ptr, ldm, M, N, K, act,
           1 if transposed else 0, L.stream())
    if drop is not None:
        L.call("a3d_dropout", y.data_ptr(), y.data_ptr(), y.numel(), drop.state.data_ptr(), int(site), drop.p, L.stream())
    return y


def linear2d(x2d, W, b, act=0, drop=None, site=0):
    """y = dropout?(act(x W^T + b)) for contiguous x2d [M,K], W [N,K]."""
    M, K = x2d.shape
    N = W.shape[0]
    if W.shape[1] != K or (b is not None and b.numel() != N):
        raise ValueError("linear: activation rows of %d features against a weight of shape %s / bias of %s" %
                         (K, tuple(W.shape), None if b is None else tuple(b.shape)))
    return linear_raw(x2d.data_ptr(), K, W.data_ptr(), W.shape[1], None if b is None else b.data_ptr(), M, N, K,
                      x2d.device, act=act, drop=drop, site=site)


def dgrad2d(dy2d, W, mask=None, drop=None, site=0, accum_into=None):
    """dx = dropout?(dy W (optionally masked by mask > 0)) for dy [M,N], W [N,K] -> [M,K]; accum_into: a contiguous [M,K] gradient
    that the product is ADDED to in place (and returned) instead."""
    M, N = dy2d.shape
    K = W.shape[1]
    if accum_into is not None:
        if mask is not None or drop is not None or tuple(accum_into.shape) != (M, K) or not accum_into.is_contiguous():
            raise ValueError("dgrad2d: accum_into takes a contiguous [M, K] buffer and neither mask nor dropout")
        return linear_raw(dy2d.data_ptr(), N, W.data_ptr(), K, None, M, K, N, dy2d.device, act=3, transposed=True, out=accum_into)
    return linear_raw(dy2d.data_ptr(), N, W.data_ptr(), K, None, M, K, N, dy2d.device,
                      act=2 if mask is not None else 0, mask_ptr=None if mask is None else mask.data_ptr(),
                      ldm=K, transposed=True, drop=drop, site=site)


# Deferred gradient reductions.  Every two-stage column sum of the backward pass (the split-M weight gradients, the LayerNorm
# dgamma / dbeta of the ghost-token rows, the FPN output bias owed to gathered rows) used to finish with a launch of its own: 41 + 12
# dependent, latency-bound launches per keypose step that add into buffers nobody reads before AdamW (or the all-reduce of the hot
# segments).  With a ReduceQueue active the first stages only leave their partial slabs behind and append a record; ONE
# a3d_grad_reduce_table launch at the end of the backward pass (an autograd-engine callback, so loss.backward() returns with complete
# .grad tensors) adds them -- per output: the slabs of a record in a fixed order, the records of one destination (tied weights: one
# per pyramid level) in the order they were appended, then one add into the gradient.  No atomics, the same bits on every run.
# A3D_DEFER_REDUCE=0: no queue is ever created and every reduction is launched where it arises (the A/B switch).
DEFER_REDUCE = os.environ.get("A3D_DEFER_REDUCE", "1") not in ("0", "", "off")


def build_reduce_table(records):
    """Host side of the table: records = [(partial_ptr, nsplit, slab_stride, count, row_len, dst_ptr, dst_stride, bias_ptr)] in the
    order they were appended -> a ctypes array of lib.GradReduceRec in which the records of one destination are adjacent (groups in
    the order of their first record, members in append order) and each group's first record carries the group's size."""
    groups = {}
    for r in records:
        partial, nsplit, slab, count, row_len, dst, dst_stride, bias = r
        key = (int(dst), int(bias or 0), int(count), int(row_len), int(dst_stride))
        groups.setdefault(key, []).append(r)
    table = (L.GradReduceRec * len(records))()
    i = 0
    for members in groups.values():
        for j, (partial, nsplit, slab, count, row_len, dst, dst_stride, bias) in enumerate(members):
            t = table[i]
            t.partial, t.dst, t.bias = int(partial), int(dst), (int(bias) if bias else None)
            t.nsplit, t.slab_stride, t.count, t.row_len, t.dst_stride = int(nsplit), int(slab), int(count), int(row_len), int(dst_stride)
            t.group_len = len(members) if j == 0 else 0
            i += 1
    return table


def reduce_table_launch(records, device, st=None):
    """One a3d_grad_reduce_table launch over `records` (see build_reduce_table) on the current stream."""
    if not records:
        return
    table = build_reduce_table(records)
    n, nwg = len(records), ctypes.c_int(0)
    L.call("a3d_grad_reduce_table_plan", table, n, ctypes.byref(nwg))
    st = L.stream() if st is None else st
    dev = torch.empty((n * ctypes.sizeof(L.GradReduceRec) // 8,), device=device, dtype=torch.int64)
    L.call("a3d_grad_reduce_table_upload", dev.data_ptr(), table, n, st)
    L.call("a3d_grad_reduce_table", dev.data_ptr(), n, nwg.value, st)


class ReduceQueue:
    """The pending second stages of one backward pass.  Records are taken only on the stream the forward pass ran on (autograd runs
    the main path's backward nodes there, and the caller of backward() goes on there; a first stage on another stream -- the query
    stream's side stream -- keeps its own second stage) and only while the autograd engine runs (the flush is its final callback)."""
    current = None                                # the queue of the last forward pass (begin_grad_sinks), None: nothing is deferred
    flushes = 0                                   # table launches so far (tests and traces look at it)

    def __init__(self, stream=None, device=None):
        self.records, self.keep = [], []
        self.stream, self.device, self.armed = stream, device, False

    def accepts(self, device):
        """Whether a first stage enqueued now on the current stream may leave its reduction to the flush; arms the flush."""
        if self.stream is None or torch.cuda.current_stream(device) != self.stream:
            return False
        if not self.armed:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(self._callback)
            except RuntimeError:                  # not inside a backward pass: nobody would flush
                return False
            if self.records:                      # left over by a pass that never reached its callback (an exception)
                self.records, self.keep = [], []
            self.armed = True
        return True

    def add(self, owner, partial_ptr, nsplit, slab_stride, count, row_len, dst_ptr, dst_stride, bias_ptr=None):
        """owner: the tensor that holds the partial slabs (kept alive until the flush has been enqueued)"""
        self.keep.append(owner)
        self.records.append((partial_ptr, nsplit, slab_stride, count, row_len, dst_ptr, dst_stride, bias_ptr))

    def flush(self):
        if not self.records:
            return
        records, self.records, self.keep, keep = self.records, [], [], self.keep
        with torch.cuda.stream(self.stream):
            reduce_table_launch(records, self.device, self.stream.cuda_stream)
        ReduceQueue.flushes += 1
        del keep

    def _callback(self):
        self.armed = False
        self.flush()


def reduce_queue(device):
    """The active queue if it takes a record from the current stream now, else None."""
    q = ReduceQueue.current
    return q if (q is not None and q.accepts(device)) else None


def flush_reduce_queue():
    """Enqueue the pending reductions now (the split backward calls it at its hot-path boundary; a no-op when none are pending)."""
    if ReduceQueue.current is not None:
        ReduceQueue.current.flush()


def wgrad_raw(dy_ptr, lddy, x_ptr, ldx, gw_ptr, lddw, gb_ptr, M, N, K, device, st=None):
    """dW += dY^T X, db += sum dY through a3d_linear_wgrad_ws: large-M reductions run two-stage (per-split partials in
    a workspace + ordered reduce) instead of memory-side float atomics.  With a ReduceQueue active the ordered reduce of a
    two-stage shape is left to the queue's flush."""
    nbytes = L.load().a3d_linear_wgrad_ws_bytes(M, N, K, 0 if gb_ptr is None else 1)
    ws = torch.empty((nbytes // 4,), device=device, dtype=F32) if nbytes else None
    q = reduce_queue(device) if (nbytes and (st is None or st == L.stream())) else None
    if q is not None:
        ns, KE = ctypes.c_int(0), K + (0 if gb_ptr is None else 1)
        L.call("a3d_linear_wgrad_partials", dy_ptr, lddy, x_ptr, ldx, 0 if gb_ptr is None else 1, M, N, K, ws.data_ptr(), nbytes,
               ctypes.byref(ns), L.stream())
        q.add(ws, ws.data_ptr(), ns.value, N * KE, N * KE, KE, gw_ptr, lddw, gb_ptr)
        return
    L.call("a3d_linear_wgrad_ws", dy_ptr, lddy, x_ptr, ldx, gw_ptr, lddw, gb_ptr, M, N, K,
           None if ws is None else ws.data_ptr(), nbytes, st if st is not None else L.stream())


def wgrad2d(dy2d, x2d, W, b):
    """W.grad += dy^T x ; b.grad += sum dy   (W, b are Parameters or None)"""
    M, N = dy2d.shape
    K = x2d.shape[1]
    gW = grad_buf(W)
    gb = grad_buf(b) if b is not None else None
    wgrad_raw(dy2d.data_ptr(), N, x2d.data_ptr(), K, gW.data_ptr(), gW.shape[1],
              None if gb is None else gb.data_ptr(), M, N, K, dy2d.device)


def add_layernorm(a2d, r2d, g, b, eps=1e-5):
    M, E = a2d.shape
    y = torch.empty_like(a2d)
    mean = torch.empty((M,), device=a2d.device, dtype=F32)
    rstd = torch.empty((M,), device=a2d.device, dtype=F32)
    L.call("a3d_add_layernorm_fwd", a2d.data_ptr(), None if r2d is None else r2d.data_ptr(), g.data_ptr(),
           b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, E, eps, L.stream())
    return y, mean, rstd


def add_layernorm_bwd(a2d, r2d, g, b, mean, rstd, dy2d, drop=None, site=0):
    """dS = d (a + r).  With `drop`: returns (dS, dropout(dS, site)) -- the gradients of LayerNorm(x + dropout(branch)) with respect
    to x and to the branch."""
    M, E = a2d.shape
    ds = torch.empty_like(a2d)
    gg, gb = grad_buf(g), grad_buf(b)
    cnt = L.load().a3d_add_layernorm_bwd_partials_count(M, E) if DEFER_REDUCE else 0
    if cnt > 0 and ((a2d.data_ptr() | (0 if r2d is None else r2d.data_ptr()) | dy2d.data_ptr() | ds.data_ptr()) & 15) == 0:
        # E <= 64: per-workgroup (sum dy * xhat, sum dy) records instead of same-address atomics, added in a fixed order by the
        # queue's flush (or right here when nothing is deferred)
        part = torch.empty((cnt, 2, E), device=a2d.device, dtype=F32)
        L.call("a3d_add_layernorm_bwd_partials", a2d.data_ptr(), None if r2d is None else r2d.data_ptr(), g.data_ptr(),
               mean.data_ptr(), rstd.data_ptr(), dy2d.data_ptr(), ds.data_ptr(), part.data_ptr(), M, E, L.stream())
        recs = [(part.data_ptr(), cnt, 2 * E, E, E, gg.data_ptr(), E, None),
                (part.data_ptr() + 4 * E, cnt, 2 * E, E, E, gb.data_ptr(), E, None)]
        q = reduce_queue(a2d.device)
        if q is not None:
            for r in recs:
                q.add(part, *r)
        else:
            reduce_table_launch(recs, a2d.device)
        if drop is not None:
            return ds, dropout_raw(ds, drop, site)
        return ds
    if drop is not None and DROP_FOLD:
        dsd = torch.empty_like(a2d)
        L.call("a3d_add_layernorm_bwd_drop", a2d.data_ptr(), None if r2d is None else r2d.data_ptr(), g.data_ptr(),
               mean.data_ptr(), rstd.data_ptr(), dy2d.data_ptr(), ds.data_ptr(), dsd.data_ptr(), gg.data_ptr(), gb.data_ptr(),
               M, E, drop.state.data_ptr(), int(site), drop.p, L.stream())
        return ds, dsd
    L.call("a3d_add_layernorm_bwd", a2d.data_ptr(), None if r2d is None else r2d.data_ptr(), g.data_ptr(),
           mean.data_ptr(), rstd.data_ptr(), dy2d.data_ptr(), ds.data_ptr(), gg.data_ptr(), gb.data_ptr(), M, E,
           L.stream())
    if drop is not None:
        return ds, dropout_raw(ds, drop, site)
    return ds


ATTN_TARGET_WGS = int(os.environ.get("A3D_ATTN_WGS", "768"))


def pick_nsplit(B, H, Lqp, Sp):
    """Key-range splits of the forward / dQ kernels: enough workgroups for several waves per SIMD on 256 CUs."""
    qw = 128 if Lqp > 64 else 64           # queries per workgroup: two 16-query tiles per wave once Lq > 64 (attention.hip)
    wgs = B * H * ((Lqp + qw - 1) // qw)
    ns = max(1, min(16, Sp // 64, -(-ATTN_TARGET_WGS // wgs)))
    return ns


# "f16": split-fp16 kernels (attention16.hip, default, the parity path); "bf16x3": attention.hip (A/B reference);
# "fp8": OPT-IN e4m3 forward (attention8.hip, BASELINE configs[4]) on the fp16 operands -- e4m3 tolerance, not the 1e-3 bar.
# It serves forwards that keep NO gradient (evaluation, inference, sampling); a forward whose backward will run stays on
# the split-fp16 kernels: the backward recomputes the weights from 16-bit logits and needs the forward's O and LSE to be
# consistent with them (sum_k G = 0), and with an fp8 O / LSE the ghost-attention gradients were measured 40-100 % off
#  -- the gradient of a near-uniform attention is a small covariance on a large common mode.
ATTN_MODE = os.environ.get("A3D_ATTN_MODE", "f16")
if ATTN_MODE not in ("f16", "bf16x3", "fp8"):
    raise ValueError("A3D_ATTN_MODE must be f16, bf16x3 or fp8, got %r" % ATTN_MODE)
LOG2E = 1.4426950408889634


ATTN16_BWD_MAX_LQP = 7296     # a3d_attn16_bwd's prep kernel sorts one (b, h)'s query rows in LDS: 12 B per query + 64 KB <= 150 KB


def _use16(Lq, need_bwd):
    """The split-fp16 operand formats feed every pass of the default and the fp8 mode (with and without dropout), except a
    forward whose backward would exceed the split-fp16 backward's query limit: that block runs on the bf16x3 family."""
    return ATTN_MODE in ("f16", "fp8") and not (need_bwd and ceil_to(Lq, 64) > ATTN16_BWD_MAX_LQP)


PLANE_PARTS = 2       # q / k planes of the backward: hi and lo parts


V_PLANES = 2 | 4      # value planes: hi and lo parts, padded channel 15 of the hi plane = 1.0 (the softmax-denominator channel)
V_ROWS = 2 | 8        # value rows of the rows-only operand set: the same 1.0 in channel 15 of the hi part of every row

# Rows-only operand set (round 6, default): the projection kernels write ONE layout of q, k and v (rows16); the forward forms V^T and
# the dQ kernel K^T with transposed LDS reads (ds_read_b64_tr_b16) of the rows tiles.  Per key and head 128 B of operands instead of
# 256 B (k rows + k planes + v rows + v planes), and forward and backward read the same tensors.  A3D_ATTN_ROWS_ONLY=0: the round-5
# rows + planes set (A/B).  The fp8 mode keeps the planes (attention8.hip packs its value operand from them).
ROWS_ONLY = os.environ.get("A3D_ATTN_ROWS_ONLY", "1") == "1"


def _rows_only():
    return ROWS_ONLY and ATTN_MODE != "fp8"


FUSED_PROJ = os.environ.get("A3D_FUSED_PROJ", "1") == "1"


def _fused_proj(E):
    """Whether a3d_proj_rope_split[16] serves an in-projection of width E: q | k | v = x W^T + b computed per 64-row tile and written
    straight in the operand formats (the projected rows never reach HBM); else a linear launch, then RoPE + operand formatting."""
    return FUSED_PROJ and E % 4 == 0 and E <= 128


# The packed in-projection of an attention block.  Per mode -- "kv": key is value, packed k,v projection
# (multihead_custom_attention.py:251-275); "qk": query is key, value differs (:277-303); "none": three inputs -- a list of GROUPS
# (index of the input in (q_in, k_in, v_in), first E-row block of in_proj_weight, roles).  A group is ONE GEMM over one input: it covers
# len(roles) consecutive E-row blocks of in_proj_weight and writes the roles' operands; the backward reads the roles' gradients side by
# side from one [rows, len(roles) E] buffer.  A role fixes its rotation (q_xyz / k_xyz / none), its scale (the softmax scale on q --
# times log2 e in the fp16 family, whose scores are in log2 units -- else 1.0) and its row count (Lq, else S).  Forward writer, backward
# loop, the cached inference pair and attn_block_plan all iterate this table.
PROJ_GROUPS = {
    "kv": ((0, 0, ("q",)), (1, 1, ("k", "v"))),
    "qk": ((0, 0, ("q", "k")), (2, 2, ("v",))),
    "none": ((0, 0, ("q",)), (1, 1, ("k",)), (2, 2, ("v",))),
}
Role = collections.namedtuple("Role", "xyz scale n npad grad nsplit", defaults=(None, 1))   # grad, nsplit: the backward's, from the core
Slot = collections.namedtuple("Slot", "rows planes word", defaults=(None,) * 3)             # a role's operands (alloc_operands)


def group_layout(w0, roles, E):
    """-> (byte offset of the group's rows in in_proj_weight, in in_proj_bias, byte offset of each role's column slice in the group's
    fp32 rows, their leading dimension in floats).  With InProj, the one place the pointer arithmetic of the packed projection is done."""
    return w0 * E * E * 4, w0 * E * 4, tuple(i * E * 4 for i in range(len(roles))), len(roles) * E


class InProj:
    """Addresses inside one packed fp32 projection (in_proj_weight [3E][E], in_proj_bias [3E]), built once per Function call and plain
    ints from then on (the eager per-launch path).  wq / wk / wv, bq / bk / bv: device pointers of a role's weight rows and bias (block
    i of group_layout); grad: the same addressing of the parameters' gradient buffers, which are created when it is first asked for."""
    __slots__ = ("weight", "bias", "E", "wq", "wk", "wv", "bq", "bk", "bv", "_grad")

    def __init__(self, weight, bias, E):
        wp, bp = weight.data_ptr(), bias.data_ptr()
        self.weight, self.bias, self.E, self._grad = weight, bias, E, None
        self.wq, self.wk, self.wv = wp, wp + E * E * 4, wp + 2 * E * E * 4
        self.bq, self.bk, self.bv = bp, bp + E * 4, bp + 2 * E * 4

    @property
    def grad(self):
        if self._grad is None:
            self._grad = InProj(grad_buf(self.weight), grad_buf(self.bias), self.E)
        return self._grad

    def group(self, w0, roles):                   # group_layout: the byte offsets are from wq / bq, and the same in grad
        return group_layout(w0, roles, self.E)

    def rows(self, w0, roles):                    # the group's rows as a slice, for the callers that need tensor VIEWS (weight[rows])
        return slice(w0 * self.E, (w0 + len(roles)) * self.E)


def alloc_operands(f16, roles, B, H, Lqp, Sp, device, need_bwd):
    """-> {role: Slot}: the operand slots of `roles` in one family.  word is what the split kernels take next to the two pointers:
    the rows width of the bf16 family (QKW for q / k: hi | lo | lo2, 32 for v) or the plane parts of the fp16 family (PLANE_PARTS,
    V_ROWS, V_PLANES).  bf16: q / k rows and v planes serve the forward, the other format of each the backward.
    fp16: q / k rows alone (no kernel reads q / k planes); v rows in the rows-only set, else v planes plus the rows the backward reads."""
    dt = torch.float16 if f16 else torch.bfloat16
    rows = lambda n, w: torch.empty((B, H, n, w), device=device, dtype=dt)
    planes = lambda n: torch.empty((B, H, 2, 16, n), device=device, dtype=dt)    # hi and lo planes, transposed
    slots = {}
    for r in roles:
        n = Lqp if r == "q" else Sp
        if r != "v":
            slots[r] = Slot(rows(n, 32), None, PLANE_PARTS) if f16 else Slot(rows(n, QKW), planes(n) if need_bwd else None, QKW)
        elif f16 and _rows_only():
            slots[r] = Slot(rows(n, 32), None, V_ROWS)
        else:
            slots[r] = Slot(rows(n, 32) if need_bwd else None, planes(n), V_PLANES if f16 else 32)
    return slots


def write_operands(f16, groups, role, slots, freq, B, E, H, device, x=None, wp=None, bp=None, fused=True, pre=None):
    """Write the operands of `groups` (entries of PROJ_GROUPS) into `slots`.  role: {role: Role}; slots: {role: Slot}; x: the (q_in,
    k_in, v_in) inputs; wp / bp: device pointers of in_proj_weight [3E][E] / in_proj_bias [3E].
    fused: one a3d_proj_rope_split[16] per group (blk0, blk1 = the group's roles).  Else one linear launch per group, then one
    a3d_rope_split[16] per role on its column slice; pre = {role: (pointer, leading dimension)} names rows that are projected already."""
    st, fp = L.stream(), freq.data_ptr()

    def blk(r):                                  # a role's launch arguments: xyz, scale, its slot in the family's order
        xyz, scale, s = L.nz(role[r].xyz), role[r].scale, slots[r]
        return (xyz, scale, L.nz(s.rows), L.nz(s.planes), s.word) if f16 else (xyz, scale, L.nz(s.rows), s.word, L.nz(s.planes))

    if fused:
        absent = (None, 1.0, None, None, 1) if f16 else (None, 1.0, None, 32, None)
        for src, w0, roles in groups:
            w_off, b_off, _, _ = group_layout(w0, roles, E)
            first = role[roles[0]]
            L.call("a3d_proj_rope_split16" if f16 else "a3d_proj_rope_split", x[src].data_ptr(), E, wp + w_off, E, bp + b_off, E,
                   *blk(roles[0]), *(blk(roles[1]) if len(roles) > 1 else absent), fp, B, first.n, first.npad, E, H, st)
        return
    keep = []
    if pre is None:
        pre = {}
        for src, w0, roles in groups:
            w_off, b_off, cols, ld = group_layout(w0, roles, E)
            keep.append(linear_raw(x[src].data_ptr(), E, wp + w_off, E, bp + b_off, B * role[roles[0]].n, ld, E, device))
            pre.update((r, (keep[-1].data_ptr() + c, ld)) for r, c in zip(roles, cols))
    for r in (r for r in "qkv" if r in pre):
        xyz, *rest = blk(r)                                      # freq goes between xyz and scale here
        L.call("a3d_rope_split16" if f16 else "a3d_rope_split", *pre[r], xyz, fp, *rest, B, role[r].n, role[r].npad, E, H, st)


def _operands(f16, groups, x, wp, bp, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd, fused=True, pre=None, kv_pair=None):
    """Allocate and write the operands of `groups` -> (Qs, Ks, Vt, Lqp, Sp, scale, freq, extra): q rows, k rows, the value operand the
    forward reads (planes; the rows of the rows-only set), and extra = (q planes, k planes, v rows) for the backward -- (Qt, Kt, Vs) in
    the bf16 family, (None, None, Vr) in the fp16 family.  `scale` is the factor a3d_rope_merge_bwd applies to the q gradient.
    kv_pair: the (Kr, Vr) rows ops.ctx_kv_operands16 wrote for this layer (fp16 rows-only slots that no group here writes)."""
    Lqp, Sp = ceil_to(Lq, 64), ceil_to(S, 64)
    scale = float(E // H) ** -0.5 * (LOG2E if f16 else 1.0)
    freq = rope_freq(E, device)
    role = {"q": Role(q_xyz, scale, Lq, Lqp), "k": Role(k_xyz, 1.0, S, Sp), "v": Role(None, 1.0, S, Sp)}
    written = list(pre) if pre is not None else [r for _, _, roles in groups for r in roles]
    slots = alloc_operands(f16, written, B, H, Lqp, Sp, device, need_bwd)
    if kv_pair is not None:
        slots["k"], slots["v"] = Slot(kv_pair[0], None, PLANE_PARTS), Slot(kv_pair[1], None, V_ROWS)
    write_operands(f16, groups, role, slots, freq, B, E, H, device, x, wp, bp, fused, pre)
    q, k, v = (slots.get(r, Slot()) for r in "qkv")
    return q.rows, k.rows, (v.rows if v.planes is None else v.planes), Lqp, Sp, scale, freq, (q.planes, k.planes, v.rows)


def attn_operands(q_pre_ptr, ldq, k_pre_ptr, ldk, v_pre_ptr, ldv, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd=False):
    """rope + split three projected row sets into the operand formats of the bf16x3 kernels (a3d_rope_split)."""
    return _operands(False, (), None, None, None, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd, fused=False,
                     pre={"q": (q_pre_ptr, ldq), "k": (k_pre_ptr, ldk), "v": (v_pre_ptr, ldv)})


def attn_operands16(q_pre_ptr, ldq, k_pre_ptr, ldk, v_pre_ptr, ldv, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd=False):
    """attn_operands for the split-fp16 kernels (a3d_rope_split16): q carries scale * log2(e)."""
    return _operands(True, (), None, None, None, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd, fused=False,
                     pre={"q": (q_pre_ptr, ldq), "k": (k_pre_ptr, ldk), "v": (v_pre_ptr, ldv)})


def attn_operands_fused(mode, q_in, k_in, v_in, wp, bp, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd=False):
    """attn_operands with the in-projections folded in (a3d_proj_rope_split)."""
    return _operands(False, PROJ_GROUPS[mode], (q_in, k_in, v_in), wp, bp, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd)


def attn_operands_fused16(mode, q_in, k_in, v_in, wp, bp, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd=False, kv_pair=None):
    """attn_operands_fused for the split-fp16 kernels (a3d_proj_rope_split16).  kv_pair: the (Kr, Vr) rows of this layer already
    written by ctx_kv_operands16 (mode "kv", rows-only set): only the q group is written here."""
    groups = PROJ_GROUPS[mode] if kv_pair is None else PROJ_GROUPS[mode][:1]
    return _operands(True, groups, (q_in, k_in, v_in), wp, bp, q_xyz, k_xyz, B, Lq, S, E, H, device, need_bwd, kv_pair=kv_pair)


def _core_fwd_entry(f16, rows, dropping, need_bwd):
    """The forward core for fp16 / bf16 operands, value rows (the rows-only set) / planes."""
    if not f16:
        return "a3d_attn_fwd_dropout" if dropping else "a3d_attn_fwd"
    if ATTN_MODE == "fp8" and not dropping and not need_bwd:
        return "a3d_attn8_fwd"
    return "a3d_attn16_fwd_rows" if rows else "a3d_attn16_fwd"


def _core_bwd_entry(f16, dropping):
    if f16:
        return "a3d_attn16_bwd"
    return "a3d_attn_bwd_bf16_dropout" if dropping else "a3d_attn_bwd_bf16"


def _group_grad_route(roles, needs, sink, fold_q):
    """What becomes of a group's input gradient in the backward.  needs: whether (q_in, k_in, v_in) need one; sink: a GradSink takes
    the context's; fold_q: the query is the residual stream and its gradient is wanted.
    "parked": the group's rows wait in the sink's shared buffer, the gate issues both of its GEMMs; "sink": written / added into the
    sink's buffer; "fold": added into the LayerNorm's input gradient; "fresh": a tensor of its own; None: no input needs it."""
    if sink and "k" in roles:
        return "parked" if CTX_DEFER else "sink"
    if not any(needs["qkv".index(r)] for r in roles):
        return None
    return "fold" if fold_q and "q" in roles else "fresh"


REDUCE_TABLE_LAUNCHES = ["a3d_grad_reduce_table_plan", "a3d_grad_reduce_table_upload", "a3d_grad_reduce_table"]


class AttnRoute:
    """What serves one AttnBlockFn call (attn_block_plan): plain strings and numbers, nothing launched.
    family      "f16" (split-fp16 operands and kernels), "fp8" (the same operands, e4m3 forward core) or "bf16x3"
    operands    "rows" (the rows-only set) or "rows+planes"
    projection  "context" (k | v rows precomputed by ctx_kv_operands16, only q is projected), "fused" or "unfused"
    groups      the entries of PROJ_GROUPS the forward writes
    core_fwd / core_bwd   entry names (core_bwd: None when no backward can follow);  nsplit: key-range splits of both"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def f16(self):
        return self.family != "bf16x3"

    def _wgrad(self, M, N, K):
        two_stage = L.load().a3d_linear_wgrad_ws_bytes(M, N, K, 1) > 0
        return "a3d_linear_wgrad_partials" if two_stage and self.queue else "a3d_linear_wgrad_ws"

    def launches_forward(self):
        """Entry names of the forward's launches in order: projection, core, out-projection (+ residual dropout), add & LayerNorm."""
        n = len(self.groups)
        if self.projection == "unfused":
            out = ["a3d_linear_fwd"] * n + ["a3d_rope_split16" if self.f16 else "a3d_rope_split"] * 3
        else:
            out = ["a3d_proj_rope_split16" if self.f16 else "a3d_proj_rope_split"] * n
        out.append(self.core_fwd)
        if self.dropping:
            out += ["a3d_linear_fwd_drop"] if DROP_FOLD else ["a3d_linear_fwd", "a3d_dropout"]
        else:
            out.append("a3d_linear_fwd")
        return out + ["a3d_add_layernorm_fwd"]

    def launches_backward(self):
        """Entry names of the backward's launches in order: LayerNorm (+ residual dropout), out-projection dgrad and wgrad, core, then
        per group the inverse rotations, the weight gradient and the input gradient.  The switches the backward reads (CTX_DEFER,
        DROP_FOLD, DEFER_REDUCE) are read now; a flush of the reduce queue and the sink gate's launches are not the block's."""
        B, Lq, S, E = self.B, self.Lq, self.S, self.E
        if not self.need_bwd:
            return []
        if DEFER_REDUCE and L.load().a3d_add_layernorm_bwd_partials_count(B * Lq, E) > 0:
            out = ["a3d_add_layernorm_bwd_partials"] + ([] if self.queue else REDUCE_TABLE_LAUNCHES)
            out += ["a3d_dropout"] if self.dropping else []
        elif self.dropping:
            out = ["a3d_add_layernorm_bwd_drop"] if DROP_FOLD else ["a3d_add_layernorm_bwd", "a3d_dropout"]
        else:
            out = ["a3d_add_layernorm_bwd"]
        out += ["a3d_linear_fwd", self._wgrad(B * Lq, E, E), self.core_bwd]
        for _, _, roles in PROJ_GROUPS[self.mode]:
            to = _group_grad_route(roles, self.needs, self.sink, self.q_is_resid and self.needs[3])
            out += ["a3d_rope_merge_bwd"] * len(roles)
            if to != "parked":
                out.append(self._wgrad(B * (Lq if roles[0] == "q" else S), len(roles) * E, E))
                out += ["a3d_linear_fwd"] if to else []
        return out


def attn_block_plan(mode, B, Lq, S, E, H, need_bwd=True, dropping=False, kv_pair=False, sink=False, q_is_resid=False,
                    needs=(True, True, True, True), queue=False):
    """Host side of AttnBlockFn, in the manner of nn.backbone_plan: the route one block takes, decided from the shapes, the module
    switches (read now) and the library's size queries alone.  need_bwd: a backward can follow; dropping: dropout with p > 0;
    kv_pair: the caller supplies this layer's context rows (ctx_kv_applicable held); sink: a GradSink of the context's shape is
    offered; needs: which of (q_in, k_in, v_in, resid) need a gradient; queue: a ReduceQueue would accept the backward's records."""
    if kv_pair and mode != "kv":
        raise RuntimeError("AttnBlockFn: precomputed context operands need the packed k,v projection (key is value)")
    f16 = bool(kv_pair) or _use16(Lq, need_bwd)
    rows = bool(kv_pair) or (f16 and _rows_only())
    Lqp, Sp = ceil_to(Lq, 64), ceil_to(S, 64)
    core_fwd = _core_fwd_entry(f16, rows, dropping, need_bwd)
    return AttnRoute(
        mode=mode, B=B, Lq=Lq, S=S, E=E, H=H, need_bwd=bool(need_bwd), dropping=bool(dropping), needs=tuple(needs),
        q_is_resid=bool(q_is_resid), queue=bool(queue),
        family="bf16x3" if not f16 else "fp8" if core_fwd == "a3d_attn8_fwd" else "f16",
        operands="rows" if rows else "rows+planes",
        projection="context" if kv_pair else "fused" if _fused_proj(E) else "unfused",
        groups=PROJ_GROUPS[mode][:1] if kv_pair else PROJ_GROUPS[mode],
        core_fwd=core_fwd, core_bwd=_core_bwd_entry(f16, dropping) if need_bwd else None,
        nsplit=pick_nsplit(B, H, Lqp, Sp),
        # the context's gradient goes into its shared buffer (packed k,v projection of ONE input only: a single dgrad GEMM)
        sink=bool(sink and need_bwd and mode == "kv" and needs[1]))


# One launch for the k | v blocks of every attention layer that reads one context (csrc/ctx_proj.hip, a3d_ctx_kv_proj16): the two
# RelativeCrossAttentionLayers of a ghost-point pyramid level project the same context rows, and the per-layer launches read them four
# times.  A3D_CTX_KV_BATCH=0: per-layer a3d_proj_rope_split16 launches (A/B).  Read at call time.
CTX_KV_BATCH = os.environ.get("A3D_CTX_KV_BATCH", "1") not in ("0", "", "off")
CTX_KV_MAX_LAYERS = 2


def ctx_kv_applicable(value, value_xyz, mhas, H, Lq=1):
    """Whether ctx_kv_operands16 serves these layers: the rows-only split-fp16 operand set with fused projections, the E = 60 / H = 4
    model, fp32 device tensors, at most CTX_KV_MAX_LAYERS layers.  (Lq: the query count; a block whose backward would exceed the
    split-fp16 backward's query limit runs on the bf16x3 family, whichever grad mode -- the operands must suit both passes.)"""
    E = value.shape[-1]
    if not (CTX_KV_BATCH and _fused_proj(E) and _rows_only() and _use16(Lq, True) and E == 60 and H == 4):
        return False
    if not (1 <= len(mhas) <= CTX_KV_MAX_LAYERS and value.is_cuda and value.dtype == F32 and value.dim() == 3):
        return False
    if value_xyz is not None and not (value_xyz.is_cuda and value_xyz.shape[:2] == value.shape[:2]):
        return False
    return all(m.in_proj_weight.dtype == F32 and m.in_proj_weight.is_cuda and m.in_proj_weight.is_contiguous() and
               tuple(m.in_proj_weight.shape) == (3 * E, E) and m.in_proj_bias.is_contiguous() for m in mhas)


def ctx_kv_operands16(value, value_xyz, mhas, H):
    """(Kr, Vr) rows16 [B][H][Sp][32] of every layer in `mhas` (modules with in_proj_weight / in_proj_bias) from ONE pass over the
    context `value` [B][S][E]: what attn_operands_fused16 writes per layer in mode "kv" (k rows rotated by value_xyz, parts 2; v rows,
    parts 2 | 8).  Returns a list of nl (Kr, Vr) pairs."""
    L.require_gpu(value)
    value = _c(value)
    B, S, E = value.shape
    Sp = ceil_to(S, 64)
    dev = value.device
    freq = rope_freq(E, dev)
    xyz = None if value_xyz is None else _c(value_xyz.to(F32))
    pairs = [(torch.empty((B, H, Sp, 32), device=dev, dtype=torch.float16), torch.empty((B, H, Sp, 32), device=dev, dtype=torch.float16))
             for _ in mhas]
    ips = [InProj(m.in_proj_weight, m.in_proj_bias, E) for m in mhas]
    args = [a for ip, (Kr, Vr) in zip(ips, pairs) for a in (ip.wk, ip.bk, Kr.data_ptr(), Vr.data_ptr())]
    args += [None] * 4 * (CTX_KV_MAX_LAYERS - len(mhas))
    L.call("a3d_ctx_kv_proj16", value.data_ptr(), E, None if xyz is None else xyz.data_ptr(), *args, E, freq.data_ptr(), len(mhas),
           B, S, Sp, E, H, 0, L.stream())
    return pairs


class DropCtx:
    """Dropout context of ONE forward pass: `state` is a device uint64[2] snapshot {seed, offset} of the model's dropout
    generator (taken before it was advanced), `p` the probability.  Forward and backward kernels of the pass regenerate
    their masks from (state, site, element index) -- nothing is stored, no host RNG, capturable."""

    def __init__(self, state, p):
        self.state, self.p = state, float(p)


def site_id(name, sub=0):
    """Dropout site of module `name` (e.g. "traj_attention.0.layers.2"): CRC-32 of the name with the low 3 bits
    replaced by the sub-site (0 cross-attention weights, 1 cross residual, 2 self-attention weights, 3 self residual,
    4 FFN / MLP hidden, 5 FFN output).  The CPU twin (oracle/blocks.py) derives the same ids from parameter prefixes."""
    import zlib
    return ((zlib.crc32(name.encode()) & 0xFFFFFFF8) | sub) & 0xFFFFFFFF


def dropout_raw(x, drop, site, out=None):
    """y = x o keep / (1 - p) (its own backward).  x contiguous fp32; out may be x (in place)."""
    y = torch.empty_like(x) if out is None else out
    L.call("a3d_dropout", x.data_ptr(), y.data_ptr(), x.numel(), drop.state.data_ptr(), int(site), drop.p, L.stream())
    return y


class DropoutFn(torch.autograd.Function):
    """nn.Dropout in training mode on the device Philox stream (layers.py:34,58,82-84; diffusion_head.py:46,183,193)."""

    @staticmethod
    def forward(ctx, x, drop, site):
        L.require_gpu(x)
        ctx.drop, ctx.site = drop, site
        return dropout_raw(_c(x), drop, site)

    @staticmethod
    def backward(ctx, dy):
        return dropout_raw(_c(dy), ctx.drop, ctx.site), None, None


def dropout_mask(drop, site, n, bh=None, q=None):
    """Keep flags (uint8) the kernels use: flat elementwise indexing (bh None) or attention-weight row (bh, q)."""
    out = torch.empty((n,), device=drop.state.device, dtype=torch.uint8)
    L.call("a3d_dropout_mask", out.data_ptr(), n, drop.state.data_ptr(), 0xFFFFFFFF if bh is None else int(bh),
           0 if q is None else int(q), int(site), drop.p, L.stream())
    return out


def attn_core_fwd(Qs, Ks, Vt, kmask, B, H, Lq, Lqp, S, Sp, nsplit, drop=None, site=0, need_bwd=False, nograd=False):
    """Attention core on pre-formatted operands; the operand dtype selects the kernel family (fp16: attention16.hip, whose
    LSE is in log2 units; bf16: attention.hip).  A 4-d fp16 Vt is the value ROWS of the rows-only operand set.  nograd: the caller
    guarantees that no backward consumes this pass (a3d_attn16_fwd_rows then forms the low part of P only around dominant keys)."""
    dev = Qs.device
    E = H * 15
    O = torch.empty((B, Lq, E), device=dev, dtype=F32)
    LSE = torch.empty((B, H, Lqp), device=dev, dtype=F32)
    ws = torch.empty((nsplit * B * H * Lqp * 18,), device=dev, dtype=F32) if nsplit > 1 else None
    f16, dropping = Qs.dtype == torch.float16, drop is not None and drop.p > 0
    entry = _core_fwd_entry(f16, Vt.dim() == 4, dropping, need_bwd)
    args = [Qs.data_ptr(), Ks.data_ptr(), Vt.data_ptr(), None if kmask is None else kmask.data_ptr(), O.data_ptr(), LSE.data_ptr(),
            None if ws is None else ws.data_ptr(), B, H, Lq, Lqp, S, Sp, nsplit]
    if entry == "a3d_attn8_fwd":
        if Vt.dim() == 4:
            raise RuntimeError("attn_core_fwd: the fp8 mode packs its value operand from value PLANES; these operands were built "
                               "in the rows-only set (build them with ops.ATTN_MODE == 'fp8')")
        ops8 = torch.empty((L.load().a3d_attn8_operand_bytes(B, H, Sp),), device=dev, dtype=torch.uint8)
        args.insert(3, ops8.data_ptr())
    elif f16:
        args += [drop.state.data_ptr() if dropping else None, int(site), drop.p if dropping else 0.0]
        args += [1 if nograd else 0] if entry == "a3d_attn16_fwd_rows" else []
    elif dropping:
        args += [drop.state.data_ptr(), int(site), drop.p]
    L.call(entry, *args, L.stream())
    return O, LSE


def attn_core_bwd(Qs, Ks, Vt, kmask, O, dO, LSE, B, H, Lq, Lqp, S, Sp, nsplit, extra=None, drop=None, site=0):
    dev = Qs.device
    dropping = drop is not None and drop.p > 0
    D = torch.empty((B, H, Lqp), device=dev, dtype=F32)
    dQp = torch.empty((nsplit, B, H, Lqp, 16), device=dev, dtype=F32)
    dK = torch.empty((B, H, Sp, 16), device=dev, dtype=F32)
    dV = torch.empty((B, H, Sp, 16), device=dev, dtype=F32)
    km = None if kmask is None else kmask.data_ptr()
    if Qs.dtype == torch.float16:
        if extra is None or extra[2] is None:
            raise RuntimeError("attn_core_bwd: the forward wrote no value rows (it ran with need_bwd=False on the planes operand set)")
        Vr = extra[2]
        dOr = torch.empty((B, H, Lqp, 32), device=dev, dtype=torch.float16)          # row-normalised dO ln2: hi | lo
        dOp = torch.empty((L.load().a3d_attn16_bwd_pack_bytes(B, H, Lqp) // 2,), device=dev, dtype=torch.float16)
        rexp = torch.empty((B, H, Lqp), device=dev, dtype=torch.int32)
        L.call(_core_bwd_entry(True, dropping), Qs.data_ptr(), None, Ks.data_ptr(), None, Vr.data_ptr(), km, O.data_ptr(),
               dO.data_ptr(), LSE.data_ptr(), dOr.data_ptr(), dOp.data_ptr(), D.data_ptr(), rexp.data_ptr(), dQp.data_ptr(),
               dK.data_ptr(), dV.data_ptr(), B, H, Lq, Lqp, S, Sp, nsplit, drop.state.data_ptr() if dropping else None,
               int(site), drop.p if dropping else 0.0, L.stream())
        return dQp, dK, dV
    if extra is None or extra[0] is None:
        raise RuntimeError("attn_core_bwd: the forward wrote no backward operand formats (it ran with need_bwd=False)")
    Qt, Kt, Vs = extra
    dOs = torch.empty((B, H, Lqp, 32), device=dev, dtype=torch.bfloat16)
    dOt = torch.empty((B, H, 2, 16, Lqp), device=dev, dtype=torch.bfloat16)
    args = (Qs.data_ptr(), Qt.data_ptr(), Ks.data_ptr(), Kt.data_ptr(), Vs.data_ptr(), km,
            O.data_ptr(), dO.data_ptr(), LSE.data_ptr(), dOs.data_ptr(), dOt.data_ptr(), D.data_ptr(), dQp.data_ptr(),
            dK.data_ptr(), dV.data_ptr(), B, H, Lq, Lqp, S, Sp, nsplit)
    L.call(_core_bwd_entry(False, dropping), *args, *((drop.state.data_ptr(), int(site), drop.p) if dropping else ()), L.stream())
    return dQp, dK, dV


def rope_merge(dR, nsplit, xyz, freq, scale, out_ptr, ldy, B, N, Npad, E, H):
    L.call("a3d_rope_merge_bwd", dR.data_ptr(), nsplit, None if xyz is None else xyz.data_ptr(), freq.data_ptr(),
           scale, out_ptr, ldy, B, N, Npad, E, H, L.stream())


# ------------------------------------------------------------------------------------------------ fused blocks
# One gradient buffer for a tensor that several kernels consume (Act3D's context tokens of a level: two ghost-attention layers and
# two query-stream layers): each consumer's backward kernel writes (first) or accumulates (+=) into the same buffer and returns None
# to autograd -- instead of four (B, S, E) tensors that autograd sums with three 63 MB torch adds per level (9 of the step's 30
# at::add launches, 0.3 ms).  The total is handed over by a GATE node between the tensor and its consumers (attach_grad_sink):
# autograd runs the gate's backward when every consumer THAT TAKES PART in this backward pass has run -- its own dependency
# count decides, so a pass in which some consumers receive no gradient (a loss on the action only: the ghost layers of a level get
# none) still delivers the others' sum.  (Round 5's first version let "the last REGISTERED consumer" return the total and dropped
# the gradient in exactly that case; found by the 6D-head golden test.)  Consumers may run on different streams (the query
# stream's side stream): an event chain orders the writers and the gate.  A3D_CTX_SINK=0: every consumer returns its own tensor (A/B).
CTX_GRAD_SINK = os.environ.get("A3D_CTX_SINK", "1") not in ("0", "", "off")


# Deferred projection gradients (round 6).  Every attention block that reads the shared tensor X through a packed k | v projection
# owes it d X += dKV_l W_l ([B S, 2E] x [2E, E]) and owes its own weights dW_l += dKV_l^T X.  Run per block these are 2 n GEMM
# launches that each re-read X (weight gradient) or read-modify-write the shared gradient (input gradient): at the trajectory
# model's script shape 16 + 16 launches, 2.3 of the 16 ms step, moving ~1.8 GB.  Deferred, the blocks only park their dKV rows
# side by side in ONE [B S, n 2E] buffer; when the last consumer has run, the gate issues ONE input-gradient GEMM with K = n 2E
# against the stacked weights and ONE weight-gradient GEMM with N = n 2E (X and the shared gradient are touched once), then adds
# the n slices of the stacked weight gradient to the parameters' own.  A3D_CTX_DEFER=0: per-block GEMMs (A/B).
CTX_DEFER = os.environ.get("A3D_CTX_DEFER", "1") not in ("0", "", "off")


class GradSink:
    live = []                                     # the sinks of the last forward pass (tests look at them)

    def __init__(self, shape, device):
        self.shape, self.device = tuple(shape), device
        self.buf, self.event = None, None
        self.writers = 0                          # consumers that wrote during the current backward pass
        self.expected = 0                         # packed-k|v attention blocks that registered during the forward pass
        self.dkv, self.parked, self.x = None, [], None

    def park(self, x, E2):
        """-> (pointer, row stride in floats) of the next free [M, E2] slice of the shared dKV buffer; the caller fills it (on the
        current stream, ordered by begin / end like any writer) and then calls parked_done()."""
        cur = torch.cuda.current_stream(self.device)
        if self.event is not None:
            cur.wait_event(self.event)
        M = self.shape[0] * self.shape[1]
        cap = max(self.expected, len(self.parked) + 1)
        if self.dkv is None:
            self.dkv = torch.empty((M, cap * E2), device=self.device, dtype=F32)
            self.x = x
        else:
            self.dkv.record_stream(cur)
        if (len(self.parked) + 1) * E2 > self.dkv.shape[1]:
            raise RuntimeError("GradSink.park: more deferred writers than registered consumers")
        return self.dkv.data_ptr() + len(self.parked) * E2 * 4, self.dkv.shape[1]

    def parked_done(self, w_kv, gw_kv, gb_kv):
        """w_kv [E2, E]: the block's k | v weight rows (a view of in_proj_weight); gw_kv / gb_kv: the matching views of the
        parameters' gradient buffers."""
        self.parked.append((w_kv, gw_kv, gb_kv))
        return self.end()

    def _flush_parked(self):
        n = len(self.parked)
        E2, E = self.parked[0][0].shape
        M, K, ld = self.dkv.shape[0], n * E2, self.dkv.shape[1]
        wstack = torch.cat([w for w, _, _ in self.parked], dim=0)                        # [n E2, E]
        acc = self.buf is not None
        if not acc:
            self.buf = torch.empty(self.shape, device=self.device, dtype=F32)
        # d X (+)= [dKV_0 | dKV_1 | ...] [W_0; W_1; ...]
        linear_raw(self.dkv.data_ptr(), ld, wstack.data_ptr(), E, None, M, E, K, self.device, act=3 if acc else 0, transposed=True,
                   out=self.buf.view(M, E))
        # [dW_0; dW_1; ...] = [dKV_0 | dKV_1 | ...]^T X, the bias gradients alongside
        nbytes = L.load().a3d_linear_wgrad_ws_bytes(M, K, E, 1)
        q = reduce_queue(self.device) if nbytes else None
        if q is not None:
            # first stage once over the stacked rows; every block's slice of the partial tiles goes straight to its own gradient
            ws = torch.empty((nbytes // 4,), device=self.device, dtype=F32)
            ns, KE = ctypes.c_int(0), E + 1
            L.call("a3d_linear_wgrad_partials", self.dkv.data_ptr(), ld, self.x.data_ptr(), E, 1, M, K, E, ws.data_ptr(), nbytes,
                   ctypes.byref(ns), L.stream())
            for i, (_, gw, gb) in enumerate(self.parked):
                q.add(ws, ws.data_ptr() + 4 * i * E2 * KE, ns.value, K * KE, E2 * KE, KE, gw.data_ptr(), gw.stride(0), gb.data_ptr())
            self.dkv, self.parked, self.x = None, [], None
            return
        gstack = torch.zeros((K, E), device=self.device, dtype=F32)
        gbstack = torch.zeros((K,), device=self.device, dtype=F32)
        wgrad_raw(self.dkv.data_ptr(), ld, self.x.data_ptr(), E, gstack.data_ptr(), E, gbstack.data_ptr(), M, K, E, self.device)
        for i, (_, gw, gb) in enumerate(self.parked):
            gw.add_(gstack[i * E2:(i + 1) * E2])
            gb.add_(gbstack[i * E2:(i + 1) * E2])
        self.dkv, self.parked, self.x = None, [], None

    def begin(self):
        """-> (buffer, accumulate): this writer runs after the previous one, whatever stream that was on"""
        cur = torch.cuda.current_stream(self.device)
        if self.event is not None:
            cur.wait_event(self.event)
        acc = self.buf is not None
        if not acc:
            self.buf = torch.empty(self.shape, device=self.device, dtype=F32)
        else:
            self.buf.record_stream(cur)
        return self.buf, acc

    def end(self):
        """the writer's kernels are enqueued: later writers / the gate wait for them.  Always returns None (the consumer's
        gradient for the shared tensor as far as autograd is concerned)."""
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(self.device))
        self.writers += 1
        return None

    def drain(self):
        """gate backward: the total of this pass (None when no consumer wrote), ordered after the last writer"""
        cur = torch.cuda.current_stream(self.device)
        if self.event is not None:
            cur.wait_event(self.event)
        if self.parked:
            if self.buf is not None:
                self.buf.record_stream(cur)
            self.dkv.record_stream(cur)
            self._flush_parked()
        out = self.buf
        if out is not None:
            out.record_stream(cur)
        self.buf, self.event, self.writers = None, None, 0
        return out


class _SinkGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, sink):
        ctx.sink = sink
        ctx.set_materialize_grads(False)          # all consumers return None: no zero tensor is made up for them
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        total = ctx.sink.drain()
        if total is None:
            return g, None
        return (total if g is None else total + g), None


def begin_grad_sinks():
    """Called once per forward pass of the owning model: forgets the sinks of the previous pass (a buffer a backward pass left
    behind -- e.g. an exception between a writer and the gate -- is dropped with them)."""
    for sk in GradSink.live:
        sk.buf, sk.event, sk.writers = None, None, 0
        sk.dkv, sk.parked, sk.x = None, [], None
    GradSink.live = []
    ReduceQueue.current = None
    if DEFER_REDUCE and torch.cuda.is_available():
        ReduceQueue.current = ReduceQueue(torch.cuda.current_stream(), torch.device("cuda", torch.cuda.current_device()))


def attach_grad_sink(t, registry=None):
    """-> the tensor the consumers of the (B, S, E) fp32 tensor t should read: t itself, or -- when its gradient is needed -- a
    view of it behind a gate node that owns a GradSink (as ._a3d_sink); the consumers pick the sink up from there.  registry: the
    list that keeps the sink for inspection (default: GradSink.live, which begin_grad_sinks() resets per Act3D forward pass)."""
    if not (CTX_GRAD_SINK and t.is_cuda and t.requires_grad and t.dtype == F32 and torch.is_grad_enabled()):
        return t
    sk = GradSink(t.shape, t.device)
    (GradSink.live if registry is None else registry).append(sk)
    out = _SinkGateFn.apply(t, sk)
    out._a3d_sink = sk
    return out


class AttnBlockFn(torch.autograd.Function):
    """y = LayerNorm(resid + out_proj(MHA(q_in, k_in, v_in)))  with RoPE-3D on q/k from xyz.

    Mirrors MultiheadCustomAttention.forward + the post-norm residual of RelativeCrossAttentionLayer
    (layers.py:299-310) and ParallelAttentionLayer (layers.py:139-159,176-191) in the reference.
    ``mode``: a key of PROJ_GROUPS.  attn_block_plan names the launches; forward and backward dispatch on its route.
    Returns (y, attn_out) where attn_out is the pre-residual attention output (rarely needed).
    """
    @staticmethod
    def forward(ctx, q_in, k_in, v_in, resid, q_xyz, k_xyz, kmask, in_w, in_b, out_w, out_b, ln_g, ln_b, H, mode,
                drop=None, site=0, grad_mode=True, sink=None, q_is_resid=False, kv_pair=None):
        """q_is_resid: the caller passed the SAME tensor object as query and residual (decided at the call site, `q_in is resid`:
        two distinct autograd tensors that merely share storage -- a detached leaf, a view alias -- keep separate gradients).
        drop / site: DropCtx of the pass and this block's site id (attention weights: site, residual branch: site + 1;
        multihead_custom_attention.py:413, layers.py:146,181).  grad_mode: torch.is_grad_enabled() of the CALLER (grad mode is
        always off inside Function.forward, so it has to be handed in; attn_block does).  kv_pair: this layer's (Kr, Vr) rows from
        ops.ctx_kv_operands16 (the caller checked ops.ctx_kv_applicable), or None."""
        L.require_gpu(q_in, k_in, v_in, resid)
        if drop is not None and drop.p <= 0:
            drop = None
        q_in, k_in, v_in, resid = _c(q_in), _c(k_in), _c(v_in), _c(resid)
        B, Lq, E = q_in.shape
        S = k_in.shape[1]
        dev = q_in.device
        if q_xyz is not None:
            q_xyz, k_xyz = _c(q_xyz.to(F32)), _c(k_xyz.to(F32))
        if kmask is not None:
            kmask = _c(kmask.to(torch.uint8))
        # whether a backward can follow: the in-projection parameters count (they get .grad through wgrad even when no
        # input needs a gradient); under torch.no_grad() none follows whatever the parameters say
        need_bwd = bool(grad_mode) and (any(ctx.needs_input_grad) or in_w.requires_grad)
        route = attn_block_plan(mode, B, Lq, S, E, H, need_bwd, drop is not None, kv_pair is not None,
                                sink is not None and tuple(k_in.shape) == sink.shape, q_is_resid, ctx.needs_input_grad[:4])
        Qs, Ks, Vt, Lqp, Sp, scale, freq, extra = _operands(route.f16, route.groups, (q_in, k_in, v_in), in_w.data_ptr(), in_b.data_ptr(),
                                                            q_xyz, k_xyz, B, Lq, S, E, H, dev, need_bwd,
                                                            fused=route.projection != "unfused", kv_pair=kv_pair)
        nsplit = route.nsplit
        O, LSE = attn_core_fwd(Qs, Ks, Vt, kmask, B, H, Lq, Lqp, S, Sp, nsplit, drop=drop, site=site, need_bwd=need_bwd,
                               nograd=not need_bwd)
        Y = linear2d(O.view(B * Lq, E), out_w, out_b, drop=drop, site=site + 1)   # seq1 + dropout(attn_out): Y is the dropped branch
        y, mean, rstd = add_layernorm(resid.view(B * Lq, E), Y, ln_g, ln_b)
        ctx.save_for_backward(q_in, k_in, v_in, resid, Y, mean, rstd, Qs, Ks, Vt, O, LSE, *_or_empty(dev, q_xyz, k_xyz, kmask))
        ctx.params = (in_w, in_b, out_w, out_b, ln_g, ln_b)
        ctx.extra = extra
        ctx.need_bwd = need_bwd
        ctx.drop, ctx.site = drop, site
        ctx.meta = (B, Lq, S, E, H, Lqp, Sp, scale, nsplit, mode, q_xyz is not None, kmask is not None)
        # the usual post-norm layer: the query IS the residual stream -- its two gradients are summed by the dgrad kernel (in place, into
        # the LayerNorm's input gradient) instead of by an autograd add
        ctx.q_is_resid = bool(q_is_resid)
        ctx.sink = sink if route.sink else None
        if ctx.sink is not None:
            ctx.sink.expected += 1
        return y.view(B, Lq, E)

    @staticmethod
    def backward(ctx, dy):
        (q_in, k_in, v_in, resid, Y, mean, rstd, Qs, Ks, Vt, O, LSE, q_xyz, k_xyz, kmask) = ctx.saved_tensors
        in_w, in_b, out_w, out_b, ln_g, ln_b = ctx.params
        B, Lq, S, E, H, Lqp, Sp, scale, nsplit, mode, has_xyz, has_mask = ctx.meta
        dev = dy.device
        if not ctx.need_bwd:
            raise RuntimeError("AttnBlockFn.backward: the forward ran with grad_mode=False (a gradient-free pass: adaptive low part "
                               "of P, no backward operand formats); call it through ops.attn_block or pass "
                               "grad_mode=torch.is_grad_enabled()")
        (q_xyz, k_xyz), (kmask,) = _or_none(has_xyz, q_xyz, k_xyz), _or_none(has_mask, kmask)
        freq = rope_freq(E, dev)
        dy = _c(dy).view(B * Lq, E)
        if ctx.drop is None:
            dS = dYo = add_layernorm_bwd(resid.view(B * Lq, E), Y, ln_g, ln_b, mean, rstd, dy)     # = d resid = d Y
        else:                                                                                     # dYo: through the residual dropout
            dS, dYo = add_layernorm_bwd(resid.view(B * Lq, E), Y, ln_g, ln_b, mean, rstd, dy, drop=ctx.drop, site=ctx.site + 1)
        dO = dgrad2d(dYo, out_w)
        wgrad2d(dYo, O.view(B * Lq, E), out_w, out_b)
        dQp, dK, dV = attn_core_bwd(Qs, Ks, Vt, kmask, O, dO.view(B, Lq, E), LSE, B, H, Lq, Lqp, S, Sp, nsplit,
                                    extra=ctx.extra, drop=ctx.drop, site=ctx.site)
        ip = InProj(in_w, in_b, E)
        g = ip.grad
        st = L.stream()
        needs = ctx.needs_input_grad
        fold_q = ctx.q_is_resid and needs[3]                     # d_q_in is added into dS (no reader of dS / dYo is left by then)
        x, d_in = (q_in, k_in, v_in), [None, None, None]
        role = {"q": Role(q_xyz, scale, Lq, Lqp, dQp, nsplit), "k": Role(k_xyz, 1.0, S, Sp, dK), "v": Role(None, 1.0, S, Sp, dV)}
        for src, w0, roles in PROJ_GROUPS[mode]:
            w_off, b_off, cols, ld = ip.group(w0, roles)
            N = role[roles[0]].n
            to = _group_grad_route(roles, needs, ctx.sink is not None, fold_q)
            if to == "parked":
                # next to the other blocks' rows (GradSink, "deferred projection gradients"): the input- and the weight-gradient
                # GEMMs of all blocks that read this context run once, at the gate
                ptr, ldg = ctx.sink.park(x[src], ld)
            else:
                rows = torch.empty((B * N, ld), device=dev, dtype=F32)
                ptr, ldg = rows.data_ptr(), ld
            for r, c in zip(roles, cols):
                ro = role[r]
                rope_merge(ro.grad, ro.nsplit, ro.xyz, freq, ro.scale, ptr + c, ldg, B, ro.n, ro.npad, E, H)
            if to == "parked":
                blocks = ip.rows(w0, roles)
                d_in[src] = ctx.sink.parked_done(in_w[blocks], g.weight[blocks], g.bias[blocks])
                continue
            wgrad_raw(ptr, ld, x[src].data_ptr(), E, g.wq + w_off, E, g.bq + b_off, B * N, ld, E, dev, st)
            if to is None:
                continue
            if to == "sink":
                buf, acc = ctx.sink.begin()
                out = buf.view(B * N, E)
            else:
                out, acc = (dS, True) if to == "fold" else (None, False)
            d = linear_raw(ptr, ld, ip.wq + w_off, E, None, B * N, E, ld, dev, act=3 if acc else 0, transposed=True, out=out)
            if to == "sink":
                d_in[src] = ctx.sink.end()                       # None: the sink's gate node hands the total to autograd
            elif to == "fresh":
                d_in[src] = d.view(B, N, E)
        d_resid = dS.view(B, Lq, E) if needs[3] else None
        return (*d_in, d_resid) + (None,) * 17


SINGLE_QUERY = os.environ.get("A3D_SINGLE_QUERY", "1") == "1"
# key splits of the single-query kernels = workgroups per sample.  The wave-local kernels (single_query_wave.hip) hold two
# workgroups per CU and pay a fixed prologue (W_k and its transpose into LDS) + epilogue (merge of the per-lane / per-wave
# partials) per workgroup: ONE resident round of 512 workgroups with 8 tiles each instead of 1024 with 4 (A3D_SQ_WGS to A/B)
SQ_TARGET_WGS = int(os.environ.get("A3D_SQ_WGS", "512"))


def sq_nsplit(B, S):
    return max(1, min((S + 63) // 64, SQ_TARGET_WGS // B))


def sq_keys_fwd(kv_in, k_xyz, ip, qrot, freq, H, project_v, st):
    """The key-streaming pass of both single-query Functions (a3d_sq_attn_fwd) over the context kv_in [B][S][E] -> (xbar [B][H][E],
    lse [B][H], o, nsplit).  project_v: the value projection is applied inside and o [B][E] is the attention output
    (SingleQueryAttnBlockFn); else o is None and a3d_qs_post_fwd projects xbar (QueryLayerFn).  ip: the layer's InProj."""
    B, S, E = kv_in.shape
    nsplit = sq_nsplit(B, S)
    new = lambda *shape: torch.empty(shape, device=kv_in.device, dtype=F32)
    ws, xbar, lse, o = new(L.load().a3d_sq_fwd_ws_floats(B, H, E, nsplit)), new(B, H, E), new(B, H), new(B, E) if project_v else None
    wv, bv = (ip.wv, ip.bv) if project_v else (None, None)
    L.call("a3d_sq_attn_fwd", kv_in.data_ptr(), L.nz(k_xyz), ip.wk, E, ip.bk, wv, E, bv, qrot.data_ptr(), freq.data_ptr(), ws.data_ptr(),
           xbar.data_ptr(), lse.data_ptr(), L.nz(o), B, S, E, H, nsplit, st)
    return xbar, lse, o, nsplit


def sq_bwd_ws(B, H, E, nsplit, device):       # the workspace of sq_keys_bwd: dxbar [B][H][E] | cD [B][H] | weight-gradient partials
    return torch.empty((L.load().a3d_sq_bwd_ws_floats(B, H, E, nsplit),), device=device, dtype=F32)


def sq_keys_bwd(kv_in, k_xyz, ip, qrot, freq, xbar, lse, dO, ws, dX, acc, H, nsplit, st):
    """Backward of sq_keys_fwd -> dqp [nsplit][B][H][1][16], the rotated-query gradient partials; dWk / dbk are accumulated.  dO: the
    gradient of o (the value projection's gradients are accumulated too); None: the value projection is the caller's, whose
    a3d_qs_post_bwd has left dxbar | cD at the head of ws.  dX [B][S][E] is written (acc None: a3d_sq_attn_bwd; False) or added to."""
    B, S, E = kv_in.shape
    g = ip.grad
    dqp = torch.empty((nsplit, B, H, 1, 16), device=kv_in.device, dtype=F32)
    wv, dwv, dbv = (None, None, None) if dO is None else (ip.wv, g.wv, g.bv)
    L.call("a3d_sq_attn_bwd" if acc is None else "a3d_sq_attn_bwd_acc", kv_in.data_ptr(), L.nz(k_xyz), ip.wk, E, ip.bk, wv, E,
           qrot.data_ptr(), freq.data_ptr(), xbar.data_ptr(), lse.data_ptr(), L.nz(dO), ws.data_ptr(), dX.data_ptr(), dqp.data_ptr(),
           g.wk, E, g.bk, dwv, E, dbv, B, S, E, H, nsplit, *(() if acc is None else (int(acc),)), st)
    return dqp


class SingleQueryAttnBlockFn(torch.autograd.Function):
    """y = LayerNorm(resid + out_proj(MHA(q, ctx, ctx))) for ONE query per sample (Act3D's query stream, act3d.py:467-480)
    on csrc/single_query.hip: the value projection commutes with the weighted sum for a single query, the key projection
    is recomputed tile by tile -- no K / V operand tensors are written, forward or backward."""

    @staticmethod
    def forward(ctx, q_in, kv_in, resid, q_xyz, k_xyz, in_w, in_b, out_w, out_b, ln_g, ln_b, H):
        L.require_gpu(q_in, kv_in, resid)
        q_in, kv_in, resid = _c(q_in), _c(kv_in), _c(resid)
        B, _, E = q_in.shape
        S = kv_in.shape[1]
        dev = q_in.device
        if q_xyz is not None:
            q_xyz, k_xyz = _c(q_xyz.to(F32)), _c(k_xyz.to(F32))
        freq = rope_freq(E, dev)
        scale = float(E // H) ** -0.5
        ip = InProj(in_w, in_b, E)
        q_pre = linear_raw(q_in.data_ptr(), E, ip.wq, E, ip.bq, B, E, E, dev)
        qrot = torch.empty((B, H, 1, 16), device=dev, dtype=F32)
        L.call("a3d_rope_rows_f32", q_pre.data_ptr(), E, L.nz(q_xyz), freq.data_ptr(), scale, qrot.data_ptr(), B, 1, 1, E, H, L.stream())
        xbar, lse, o, nsplit = sq_keys_fwd(kv_in, k_xyz, ip, qrot, freq, H, True, L.stream())
        Y = linear2d(o, out_w, out_b)
        y, mean, rstd = add_layernorm(resid.view(B, E), Y, ln_g, ln_b)
        ctx.save_for_backward(q_in, kv_in, resid, Y, mean, rstd, qrot, xbar, lse, o, *_or_empty(dev, q_xyz, k_xyz))
        ctx.params = (in_w, in_b, out_w, out_b, ln_g, ln_b)
        ctx.meta = (B, S, E, H, scale, nsplit, q_xyz is not None)
        return y.view(B, 1, E)

    @staticmethod
    def backward(ctx, dy):
        q_in, kv_in, resid, Y, mean, rstd, qrot, xbar, lse, o, q_xyz, k_xyz = ctx.saved_tensors
        in_w, in_b, out_w, out_b, ln_g, ln_b = ctx.params
        B, S, E, H, scale, nsplit, has_xyz = ctx.meta
        dev = dy.device
        q_xyz, k_xyz = _or_none(has_xyz, q_xyz, k_xyz)
        freq = rope_freq(E, dev)
        dS = add_layernorm_bwd(resid.view(B, E), Y, ln_g, ln_b, mean, rstd, _c(dy).view(B, E))
        dO = dgrad2d(dS, out_w)
        wgrad2d(dS, o, out_w, out_b)
        ip = InProj(in_w, in_b, E)
        g = ip.grad
        ws = sq_bwd_ws(B, H, E, nsplit, dev)
        dX = torch.empty((B, S, E), device=dev, dtype=F32)
        dqp = sq_keys_bwd(kv_in, k_xyz, ip, qrot, freq, xbar, lse, dO, ws, dX, None, H, nsplit, L.stream())
        dq_pre = torch.empty((B, E), device=dev, dtype=F32)
        rope_merge(dqp, nsplit, q_xyz, freq, scale, dq_pre.data_ptr(), E, B, 1, 1, E, H)
        wgrad_raw(dq_pre.data_ptr(), E, q_in.data_ptr(), E, g.wq, E, g.bq, B, E, E, dev)
        d_q_in = dgrad2d(dq_pre, in_w[ip.rows(0, "q")]).view(B, 1, E) if ctx.needs_input_grad[0] else None
        return (d_q_in, dX if ctx.needs_input_grad[1] else None, dS.view(B, 1, E) if ctx.needs_input_grad[2] else None) + (None,) * 9


QUERY_STREAM_FUSED = os.environ.get("A3D_QS_FUSED", "1") == "1"


class QueryLayerFn(torch.autograd.Function):
    """One layer of Act3D's query stream -- RelativeCrossAttentionLayer + FeedforwardLayer on ONE query per sample
    (act3d.py:467-480, layers.py:293-351):  y = LN2(x1 + W2 relu(W1 x1)),  x1 = LN1(x + out_proj(MHA(x, ctx, ctx)))  -- as
    csrc/query_stream.hip's fused launches around the key-streaming kernels of csrc/single_query.hip: 4 launches forward
    (q projection + RoPE | keys | combine | everything after) and 4 backward, instead of 10 + 16 single-workgroup ones.
    Same arithmetic as SingleQueryAttnBlockFn followed by MLPFn (exact-f32 MFMA products; summation order differs)."""

    @staticmethod
    def forward(ctx, x, kv_in, q_xyz, k_xyz, in_w, in_b, out_w, out_b, g1, b1, w1, c1, w2, c2, g2, b2, H, sink=None):
        L.require_gpu(x, kv_in)
        x, kv_in = _c(x), _c(kv_in)
        B, _, E = x.shape
        S = kv_in.shape[1]
        dev = x.device
        if q_xyz is not None:
            q_xyz, k_xyz = _c(q_xyz.to(F32)), _c(k_xyz.to(F32))
        freq = rope_freq(E, dev)
        scale = float(E // H) ** -0.5
        ip = InProj(in_w, in_b, E)
        st = L.stream()
        qrot = torch.empty((B, H, 1, 16), device=dev, dtype=F32)
        L.call("a3d_qs_pre_fwd", x.data_ptr(), ip.wq, ip.bq, L.nz(q_xyz), freq.data_ptr(), scale, qrot.data_ptr(), B, E, H, st)
        xbar, lse, _, nsplit = sq_keys_fwd(kv_in, k_xyz, ip, qrot, freq, H, False, st)
        save = torch.empty((L.load().a3d_qs_save_floats(B, E),), device=dev, dtype=F32)
        y = torch.empty((B, 1, E), device=dev, dtype=F32)
        qp = QueryLayerFn._params(ip, out_w, out_b, g1, b1, w1, c1, w2, c2, g2, b2)
        L.call("a3d_qs_post_fwd", xbar.data_ptr(), x.data_ptr(), L.byref(qp), save.data_ptr(), y.data_ptr(), B, E, H, st)
        ctx.save_for_backward(x, kv_in, qrot, xbar, lse, save, *_or_empty(dev, q_xyz, k_xyz))
        ctx.params = (in_w, in_b, out_w, out_b, g1, b1, w1, c1, w2, c2, g2, b2)
        ctx.meta = (B, S, E, H, scale, nsplit, q_xyz is not None)
        ctx.sink = sink if (sink is not None and ctx.needs_input_grad[1] and tuple(kv_in.shape) == sink.shape) else None
        return y

    @staticmethod
    def _params(ip, out_w, out_b, g1, b1, w1, c1, w2, c2, g2, b2):
        return L.QsParams(wv=ip.wv, bv=ip.bv, wo=out_w.data_ptr(), bo=out_b.data_ptr(), g1=g1.data_ptr(), b1=b1.data_ptr(),
                          w1=w1.data_ptr(), c1=c1.data_ptr(), w2=w2.data_ptr(), c2=c2.data_ptr(), g2=g2.data_ptr(), b2=b2.data_ptr())

    @staticmethod
    def backward(ctx, dy):
        x, kv_in, qrot, xbar, lse, save, q_xyz, k_xyz = ctx.saved_tensors
        in_w, in_b, out_w, out_b, g1, b1, w1, c1, w2, c2, g2, b2 = ctx.params
        B, S, E, H, scale, nsplit, has_xyz = ctx.meta
        dev = dy.device
        q_xyz, k_xyz = _or_none(has_xyz, q_xyz, k_xyz)
        freq = rope_freq(E, dev)
        st = L.stream()
        ip = InProj(in_w, in_b, E)
        g = ip.grad
        qp = QueryLayerFn._params(ip, out_w, out_b, g1, b1, w1, c1, w2, c2, g2, b2)
        gr = L.QsGrads(dwv=g.wv, dbv=g.bv, dwo=grad_buf(out_w).data_ptr(), dbo=grad_buf(out_b).data_ptr(), dg1=grad_buf(g1).data_ptr(),
                       db1=grad_buf(b1).data_ptr(), dw1=grad_buf(w1).data_ptr(), dc1=grad_buf(c1).data_ptr(), dw2=grad_buf(w2).data_ptr(),
                       dc2=grad_buf(c2).data_ptr(), dg2=grad_buf(g2).data_ptr(), db2=grad_buf(b2).data_ptr())
        ws = sq_bwd_ws(B, H, E, nsplit, dev)                 # a3d_qs_post_bwd leaves dxbar | cD at its head for the key pass
        dx = torch.empty((B, 1, E), device=dev, dtype=F32)
        L.call("a3d_qs_post_bwd", _c(dy).data_ptr(), x.data_ptr(), xbar.data_ptr(), save.data_ptr(), L.byref(qp), L.byref(gr),
               ws.data_ptr(), ws.data_ptr() + B * H * E * 4, dx.data_ptr(), B, E, H, st)
        if ctx.sink is not None:
            dXb, acc = ctx.sink.begin()                      # the context's shared gradient buffer: written or summed into
        else:
            dXb, acc = torch.empty((B, S, E), device=dev, dtype=F32), False
        dqp = sq_keys_bwd(kv_in, k_xyz, ip, qrot, freq, xbar, lse, None, ws, dXb, acc, H, nsplit, st)
        dX = ctx.sink.end() if ctx.sink is not None else dXb
        L.call("a3d_qs_pre_bwd", dqp.data_ptr(), nsplit, L.nz(q_xyz), freq.data_ptr(), scale, x.data_ptr(), ip.wq, g.wq, g.bq,
               dx.data_ptr(), B, E, H, st)
        return (dx if ctx.needs_input_grad[0] else None, dX if ctx.needs_input_grad[1] else None) + (None,) * 16


def query_layer_applicable(query, value, E, H, hidden):
    return (QUERY_STREAM_FUSED and SINGLE_QUERY and query.is_cuda and query.shape[1] == 1 and E <= 60 and E % 12 == 0 and H <= 4 and
            H * 15 == E and hidden == E and value.dtype == F32 and query.dtype == F32)


def attn_block(q_in, k_in, v_in, resid, q_xyz, k_xyz, kmask, mha, norm, H, drop=None, site=0, sink=None, kv_pair=None):
    """mha: module with in_proj_weight/in_proj_bias/out_proj; norm: LayerNorm-like with weight/bias.

    The projection path is chosen structurally (which inputs are the same tensor), replacing the reference's
    data-dependent torch.equal checks (multihead_custom_attention.py:234-235) that force a host sync."""
    E = q_in.shape[-1]
    if (SINGLE_QUERY and k_in is v_in and q_in.shape[1] == 1 and kmask is None and E <= 60 and E % 12 == 0 and H <= 4
            and (drop is None or drop.p <= 0) and k_in.dtype == F32 and q_in.is_cuda):
        return SingleQueryAttnBlockFn.apply(q_in, k_in, resid, q_xyz, k_xyz, mha.in_proj_weight, mha.in_proj_bias,
                                            mha.out_proj.weight, mha.out_proj.bias, norm.weight, norm.bias, H)
    if k_in is v_in:
        mode = "kv"
    elif q_in is k_in:
        mode = "qk"
    else:
        mode = "none"
    return AttnBlockFn.apply(q_in, k_in, v_in, resid, q_xyz, k_xyz, kmask, mha.in_proj_weight, mha.in_proj_bias,
                             mha.out_proj.weight, mha.out_proj.bias, norm.weight, norm.bias, H, mode, drop, site,
                             torch.is_grad_enabled(), sink, q_in is resid, kv_pair)


class MLPFn(torch.autograd.Function):
    """out = W2 relu(W1 x + b1) + b2, optionally followed by LayerNorm(x + out) (FeedforwardLayer layers.py:313-332,
    ffn_12 + norm_122 layers.py:205-209; plain MLP heads act3d.py:151-166, diffusion_head.py:41-49,177-199)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, ln_g, ln_b, drop=None, site_hidden=0, site_out=None):
        """drop: DropCtx; site_hidden: the nn.Dropout between ReLU and the second Linear (layers.py:82, diffusion_head.py:46);
        site_out: the one after it (layers.py:84), None if the module has none."""
        L.require_gpu(x)
        x = _c(x)
        shp = x.shape
        K = shp[-1]
        x2 = x.view(-1, K)
        if drop is not None and drop.p <= 0:
            drop = None
        h = linear2d(x2, w1, b1, act=1, drop=drop, site=site_hidden)   # h > 0 <=> relu active AND kept: still the ReLU mask of dgrad
        o = linear2d(h, w2, b2, drop=drop if site_out is not None else None, site=site_out or 0)
        ctx.drop, ctx.sites = drop, (site_hidden, site_out)
        if ln_g is not None:
            y, mean, rstd = add_layernorm(x2, o, ln_g, ln_b)
            ctx.save_for_backward(x2, h, o, mean, rstd)
        else:
            y = o
            ctx.save_for_backward(x2, h)
        ctx.params = (w1, b1, w2, b2, ln_g, ln_b)
        return y.view(*shp[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        w1, b1, w2, b2, ln_g, ln_b = ctx.params
        dy = _c(dy)
        drop, (site_hidden, site_out) = ctx.drop, ctx.sites
        out_drop = drop if site_out is not None else None
        if ln_g is not None:
            x2, h, o, mean, rstd = ctx.saved_tensors
            if out_drop is None:
                dS = do = add_layernorm_bwd(x2, o, ln_g, ln_b, mean, rstd, dy.view(-1, dy.shape[-1]))
            else:
                dS, do = add_layernorm_bwd(x2, o, ln_g, ln_b, mean, rstd, dy.view(-1, dy.shape[-1]), drop=out_drop, site=site_out)
        else:
            x2, h = ctx.saved_tensors
            dS = None
            do = dy.view(-1, dy.shape[-1])
            if out_drop is not None:
                do = dropout_raw(do, drop, site_out)
        wgrad2d(do, h, w2, b2)
        # relu backward fused: (do W2) * (h > 0), then the 1 / (1 - p) of the kept (h > 0) elements
        dpre = dgrad2d(do, w2, mask=h, drop=drop, site=site_hidden)
        wgrad2d(dpre, x2, w1, b1)
        dx = None
        if ctx.needs_input_grad[0]:
            # dS (and `do`, which may be the same buffer) has no reader left: the input gradient is summed into it in place
            dx = dgrad2d(dpre, w1) if dS is None else dgrad2d(dpre, w1, accum_into=dS)
            dx = dx.view(*dy.shape[:-1], x2.shape[1])
        return dx, None, None, None, None, None, None, None, None, None


def mlp(x, lin1, lin2, norm=None, drop=None, site_hidden=0, site_out=None):
    return MLPFn.apply(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, None if norm is None else norm.weight,
                       None if norm is None else norm.bias, drop, site_hidden, site_out)


class LinearFn(torch.autograd.Function):
    """y = x W^T + b (instruction encoder act3d.py:170, gripper encoders diffusion_head.py:50-52, AdaLN modulation)."""

    @staticmethod
    def forward(ctx, x, w, b):
        L.require_gpu(x)
        x = _c(x)
        x2 = x.view(-1, x.shape[-1])
        y = linear2d(x2, w, b)
        ctx.save_for_backward(x2)
        ctx.params = (w, b)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        w, b = ctx.params
        dy2 = _c(dy).view(-1, dy.shape[-1])
        wgrad2d(dy2, x2, w, b)
        dx = dgrad2d(dy2, w).view(*dy.shape[:-1], x2.shape[1]) if ctx.needs_input_grad[0] else None
        return dx, None, None


def linear(x, lin):
    return LinearFn.apply(x, lin.weight, lin.bias)


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, b):
        x = _c(x)
        x2 = x.view(-1, x.shape[-1])
        y, mean, rstd = add_layernorm(x2, None, g, b)
        ctx.save_for_backward(x2, mean, rstd)
        ctx.params = (g, b)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd = ctx.saved_tensors
        g, b = ctx.params
        ds = add_layernorm_bwd(x2, None, g, b, mean, rstd, _c(dy).view(-1, dy.shape[-1]))
        return ds.view(dy.shape), None, None


# ------------------------------------------------------------------------------------------------ scene ops
def pcd_downsample(pcd, factor):
    """pcd (B, C, 3, H, W) -> (B, C*h*w, 3)   [no grad: act3d.py never differentiates w.r.t. xyz]"""
    L.require_gpu(pcd)
    pcd = _c(pcd.to(F32))
    B, Cn, _, Hh, Ww = pcd.shape
    h, w = Hh // factor, Ww // factor
    out = torch.empty((B, Cn * h * w, 3), device=pcd.device, dtype=F32)
    L.call("a3d_pcd_downsample", pcd.data_ptr(), out.data_ptr(), B, Cn, Hh, Ww, factor, L.stream())
    return out


def knn_topk(pos, xyz, k, return_dist=False):
    """indices (B, k) int64 of the k nearest scene points, ascending (distance, index)."""
    L.require_gpu(pos, xyz)
    pos, xyz = _c(pos.to(F32)).view(-1, 3), _c(xyz.to(F32))
    B, N, _ = xyz.shape
    ws = torch.empty((L.load().a3d_knn_topk_ws_bytes(B, N) // 4,), device=xyz.device, dtype=torch.int32)
    idx = torch.empty((B, k), device=xyz.device, dtype=torch.int64)
    dist = torch.empty((B, k), device=xyz.device, dtype=F32) if return_dist else None
    L.call("a3d_knn_topk", pos.data_ptr(), xyz.data_ptr(), ws.data_ptr(), idx.data_ptr(),
           None if dist is None else dist.data_ptr(), B, N, k, L.stream())
    return (idx, dist) if return_dist else idx


def traj_nn_topk(traj_xyz, xyz, k):
    """find_traj_nn (model/utils/utils.py:39-48): indices (B, k) of the k scene points closest (squared distance) to ANY of
    the trajectory points traj_xyz (B, L, 3), ascending (distance, index)."""
    L.require_gpu(traj_xyz, xyz)
    traj_xyz, xyz = _c(traj_xyz.detach().to(F32)), _c(xyz.to(F32))
    B, N, _ = xyz.shape
    ws = torch.empty((L.load().a3d_knn_topk_ws_bytes(B, N) // 4,), device=xyz.device, dtype=torch.int32)
    idx = torch.empty((B, k), device=xyz.device, dtype=torch.int64)
    L.call("a3d_traj_nn_topk", traj_xyz.data_ptr(), traj_xyz.shape[1], xyz.data_ptr(), ws.data_ptr(), idx.data_ptr(), None,
           B, N, k, L.stream())
    return idx


def gather_rows(src, idx, extra=None):
    """[src[b][idx[b]] | extra[b]] without autograd (xyz rows)."""
    src = _c(src)
    B, Npts, W = src.shape
    k = idx.shape[1] if idx is not None else Npts
    X = 0 if extra is None else extra.shape[1]
    out = torch.empty((B, k + X, W), device=src.device, dtype=F32)
    L.call("a3d_build_context", src.data_ptr(), None if idx is None else idx.data_ptr(),
           None if extra is None else _c(extra).data_ptr(), out.data_ptr(), B, Npts, k, X, W, L.stream())
    return out


class GradAccum:
    """One gradient buffer for a token map that several pyramid levels gather from (levels >= 1 share the res1 map,
    act3d.py:86): every level's backward scatters into it and only the last one hands it to autograd, instead of one
    dense map per level plus the adds that sum them."""

    def __init__(self):
        self.buf, self.pending = None, 0


# Token-sparse weight gradient of the FPN's 3x3 output convolution (csrc/fpn_sparse.hip, round 6): a map whose gradient arrives only
# through BuildContextFn's gathers gets its convolution's weight gradient from those gathers' own backward inputs (indices + context
# gradient rows) instead of a dense library kernel over the zero-filled, scattered map.  A3D_FPN_SPARSE_WGRAD=0: dense (A/B).
SPARSE_FPN_WGRAD = os.environ.get("A3D_FPN_SPARSE_WGRAD", "1") == "1"
# the same convolution's INPUT gradient on the 8 x 32-pixel tiles the gathered tokens' neighbourhoods touch (csrc/conv3x3.hip LIST
# variant) instead of the library's dense igemm_bwd; the library serves maps more than SPARSE_FPN_DGRAD_MAX of whose pixels were gathered
SPARSE_FPN_DGRAD = os.environ.get("A3D_FPN_SPARSE_DGRAD", "1") == "1"
SPARSE_FPN_DGRAD_MAX = float(os.environ.get("A3D_FPN_SPARSE_DGRAD_MAX", "0.25"))


class SparseConvCtx:
    """Shared by the FPN's output convolution of one map (nn._LayerConv3x3Fn) and the map's gather consumers (BuildContextFn):
    x: the convolution's input (bf16 channels_last, 64 channels), ncam: cameras per sample (the token index of a sample runs over
    (camera, h, w)); dw: the weight gradient [3][3][64 co][64 ci] the gathers' backward passes have accumulated so far (None: none
    yet); dense: some consumer read the map densely (idx None) -- its gradient is not in dw, the convolution falls back to the
    library's dense weight gradient."""
    __slots__ = ("x", "ncam", "dw", "dense", "mask", "ntok")

    def __init__(self, ncam):
        self.x, self.ncam, self.dw, self.dense = None, ncam, None, False
        # mask: one byte per 8 x 32-pixel tile of the map, set by the gathers' backward passes for the tiles the 3x3 neighbourhoods of
        # their tokens touch (a3d_conv3x3_mark_tiles) -- the convolution's input gradient is then computed on those tiles only
        # (a3d_conv3x3_dgrad_tiles); ntok: tokens marked so far (the static coverage bound the convolution decides by)
        self.mask, self.ntok = None, 0


class TokenMap:
    """One level's visual tokens (B, ncam*h*w, ld) plus the bias that is still OWED to the rows a level gathers: the FPN's 3x3
    output convolution runs bias-free on the bf16 path (nn.FeaturePyramidNetwork.forward(defer_output_bias=True)) and
    BuildContextFn adds `row_bias` to the gathered rows.  An explicit pair instead of an attribute on the tensor: any tensor
    op (.float(), .detach(), slicing, save / load) would silently drop an attribute and run the model on bias-free features."""
    __slots__ = ("tokens", "row_bias", "conv_ctx")

    def __init__(self, tokens, row_bias=None, conv_ctx=None):
        self.tokens, self.row_bias, self.conv_ctx = tokens, row_bias, conv_ctx      # conv_ctx: SparseConvCtx of the producing convolution or None

    @staticmethod
    def of(x):
        return x if isinstance(x, TokenMap) else TokenMap(x, None)

    def detach(self):
        return TokenMap(self.tokens.detach(), self.row_bias)

    def leaf(self):
        """detached leaf of the tokens that records a gradient (engine._split_backward); the bias keeps its own graph, the
        convolution context travels along (the leaf's gradient goes back through the same convolution)"""
        return TokenMap(self.tokens.detach().requires_grad_(self.tokens.requires_grad), self.row_bias, self.conv_ctx)

    def with_bias(self):
        """the tokens with the owed bias added (what the reference's feature map holds, act3d.py:352), fp32"""
        if self.row_bias is None:
            return self.tokens
        E = self.row_bias.numel()
        return self.tokens[..., :E].float() + self.row_bias.float()


class BuildContextFn(torch.autograd.Function):
    """ctx tokens = [feat[b][idx[b]] | extra[b]]  (act3d.py:247-260).  feat (B, Npts, E) fp32, or bf16 (the FPN's
    channels-last output read in place: no fp32 copy of the map, the gradient goes back as one bf16 map); extra (B, X, E)."""

    @staticmethod
    def forward(ctx, feat, idx, extra, accum=None, bias=None, conv_ctx=None):
        """bias: fp32 Parameter (E,) added to the gathered rows of a bf16 map (the deferred bias of the FPN's 3x3 output
        convolution, nn.FeaturePyramidNetwork.forward(defer_output_bias=True)); its gradient -- the column sums of d(ctx)
        over the gathered rows -- is accumulated into bias.grad by the backward.  conv_ctx: SparseConvCtx of the convolution that
        produced the map: the backward then also accumulates that convolution's WEIGHT gradient from (idx, d ctx rows)."""
        L.require_gpu(feat)
        feat, extra = _c(feat), _c(extra)
        B, Npts, ldf = feat.shape
        E = extra.shape[2]                                # bf16 maps may carry pad channels (ldf = 64 for E = 60)
        k = idx.shape[1] if idx is not None else Npts
        X = extra.shape[1]
        out = torch.empty((B, k + X, E), device=feat.device, dtype=F32)
        bf = feat.dtype == torch.bfloat16
        if bias is not None and (not bf or bias.numel() != E or bias.dtype != F32):
            raise ValueError("BuildContextFn: a deferred row bias needs a bf16 token map and an fp32 bias of %d entries" % E)
        if bf:
            L.call("a3d_build_context_bf16", feat.data_ptr(), ldf, None if idx is None else idx.data_ptr(), extra.data_ptr(),
                   None if bias is None else bias.data_ptr(), out.data_ptr(), B, Npts, k, X, E, L.stream())
        else:
            if ldf != E:
                raise ValueError("fp32 token rows must have exactly the context width (%d vs %d)" % (ldf, E))
            L.call("a3d_build_context", feat.data_ptr(), None if idx is None else idx.data_ptr(), extra.data_ptr(),
                   out.data_ptr(), B, Npts, k, X, E, L.stream())
        ctx.idx = idx
        ctx.accum = accum
        ctx.bias = bias
        ctx.conv_ctx = conv_ctx if (bf and ctx.needs_input_grad[0]) else None
        if ctx.conv_ctx is not None and idx is None:
            ctx.conv_ctx.dense = True                  # a dense reader: its gradient is not covered by the token-sparse path
        if accum is not None:
            accum.pending += 1
        ctx.meta = (B, Npts, k, X, E, bf, ldf)
        return out

    @staticmethod
    def backward(ctx, dctx):
        B, Npts, k, X, E, bf, ldf = ctx.meta
        dctx = _c(dctx)
        idx, accum = ctx.idx, ctx.accum
        dfeat = dextra = None
        accumulate = 0
        if ctx.bias is not None and ctx.bias.requires_grad:
            ws = torch.empty((L.load().a3d_colsum_rows_ws_floats(B, k, E),), device=dctx.device, dtype=F32)
            gb = grad_buf(ctx.bias)
            q = reduce_queue(dctx.device)
            if q is not None:
                L.call("a3d_colsum_rows_partials", dctx.data_ptr(), B, k + X, k, E, E, ws.data_ptr(), L.stream())
                q.add(ws, ws.data_ptr(), ws.numel() // E, E, E, E, gb.data_ptr(), E, None)
            else:
                L.call("a3d_colsum_rows", dctx.data_ptr(), B, k + X, k, E, E, gb.data_ptr(), E, ws.data_ptr(), L.stream())
        cc = ctx.conv_ctx
        if (cc is not None and not cc.dense and idx is not None and SPARSE_FPN_WGRAD and cc.x is not None and cc.x.shape[1] == 64
                and cc.ncam * cc.x.shape[2] * cc.x.shape[3] == Npts and E <= 64):
            # the producing convolution's weight gradient, straight from this gather's indices and gradient rows
            acc = cc.dw is not None
            if not acc:
                cc.dw = torch.empty((3, 3, 64, 64), device=dctx.device, dtype=F32)
            ws = torch.empty((L.load().a3d_conv3x3_wgrad_tokens_ws_floats(),), device=dctx.device, dtype=F32)
            L.call("a3d_conv3x3_wgrad_tokens", cc.x.data_ptr(), idx.data_ptr(), dctx.data_ptr(), k + X, E, ws.data_ptr(),
                   cc.dw.data_ptr(), 1 if acc else 0, B, k, cc.ncam, cc.x.shape[2], cc.x.shape[3], L.stream())
            if SPARSE_FPN_DGRAD and cc.mask is not None:
                L.call("a3d_conv3x3_mark_tiles", idx.data_ptr(), B, k, cc.ncam, cc.x.shape[2], cc.x.shape[3], cc.mask.data_ptr(), L.stream())
                cc.ntok += B * k
        if ctx.needs_input_grad[0]:
            dt = torch.bfloat16 if bf else F32
            if accum is not None and accum.buf is None and accum.pending == 1:
                accum.pending, accum = 0, None         # the map's only consumer: no shared buffer needed
            if accum is not None:
                if accum.buf is None:
                    accum.buf = torch.zeros((B, Npts, ldf), device=dctx.device, dtype=dt)
                dfeat, accumulate = accum.buf, 1
            else:
                dense = idx is None and ldf == E
                dfeat = (torch.empty if dense else torch.zeros)((B, Npts, ldf), device=dctx.device, dtype=dt)
        if ctx.needs_input_grad[2]:
            dextra = torch.empty((B, X, E), device=dctx.device, dtype=F32)
        iptr = None if idx is None else idx.data_ptr()
        fptr = None if dfeat is None else dfeat.data_ptr()
        eptr = None if dextra is None else dextra.data_ptr()
        if bf:
            L.call("a3d_build_context_bwd_bf16", dctx.data_ptr(), iptr, fptr, ldf, eptr, B, Npts, k, X, E, accumulate, L.stream())
        else:
            L.call("a3d_build_context_bwd", dctx.data_ptr(), iptr, fptr, eptr, B, Npts, k, X, E, accumulate, L.stream())
        if accum is not None:
            accum.pending -= 1
            if accum.pending > 0:
                dfeat = None                    # a later backward of the same map returns the shared buffer
            else:
                accum.buf = None
        return dfeat, None, dextra, None, None, None


# ------------------------------------------------------------------------------------------------ heads / losses
class MaskLogitsFn(torch.autograd.Function):
    """logits[b, n] = <q[b], F[b, n]>   (act3d.py:493-494)"""

    @staticmethod
    def forward(ctx, q, Fm):
        q, Fm = _c(q), _c(Fm)
        B, Ng, E = Fm.shape
        out = torch.empty((B, Ng), device=Fm.device, dtype=F32)
        L.call("a3d_mask_logits_fwd", q.data_ptr(), Fm.data_ptr(), out.data_ptr(), B, Ng, E, L.stream())
        ctx.save_for_backward(q, Fm)
        return out

    @staticmethod
    def backward(ctx, dlog):
        q, Fm = ctx.saved_tensors
        B, Ng, E = Fm.shape
        dF = torch.empty_like(Fm)
        dq = torch.empty_like(q)
        L.call("a3d_mask_logits_bwd", q.data_ptr(), Fm.data_ptr(), _c(dlog).data_ptr(), dF.data_ptr(), dq.data_ptr(), B,
               Ng, E, 0, L.stream())
        return dq, dF


def argmax_gather(logits, ghost):
    """top_idx (B,) int64 = first maximum; position (B, 3) = ghost[b, top_idx]."""
    logits, ghost = _c(logits), _c(ghost)
    B, Ng = logits.shape
    top = torch.empty((B,), device=logits.device, dtype=torch.int64)
    pos = torch.empty((B, 3), device=logits.device, dtype=F32)
    L.call("a3d_argmax_gather", logits.data_ptr(), ghost.data_ptr(), top.data_ptr(), pos.data_ptr(), B, Ng, L.stream())
    return top, pos


class SoftCEFn(torch.autograd.Function):
    """coeff * mean_b CE(logits[b], softmax(-|ghost - gt| / spread))   (main_keypose.py:382-405)"""

    @staticmethod
    def forward(ctx, logits, ghost, gt, spread, label_smoothing, coeff):
        logits, ghost, gt = _c(logits), _c(ghost), _c(gt.to(F32))
        B, Ng = logits.shape
        loss_b = torch.empty((B,), device=logits.device, dtype=F32)
        loss = torch.empty((), device=logits.device, dtype=F32)
        dlog = torch.empty_like(logits)
        L.call("a3d_soft_ce_loss", ghost.data_ptr(), gt.data_ptr(), logits.data_ptr(), loss_b.data_ptr(),
               loss.data_ptr(), dlog.data_ptr(), B, Ng, spread, label_smoothing, coeff, L.stream())
        ctx.save_for_backward(dlog)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlog,) = ctx.saved_tensors
        out = torch.empty_like(dlog)
        L.call("a3d_scale_by_scalar", dlog.data_ptr(), _c(g).data_ptr(), out.data_ptr(), dlog.numel(), L.stream())
        return out, None, None, None, None, None


class ElemLossFn(torch.autograd.Function):
    """coeff * mean((p - t)^2) [kind 0] or coeff * mean(|p - t|) [kind 1]"""

    @staticmethod
    def forward(ctx, pred, target, kind, coeff):
        pred, target = _c(pred), _c(target.to(F32))
        loss = torch.empty((), device=pred.device, dtype=F32)
        grad = torch.empty_like(pred)
        L.call("a3d_elem_loss", pred.data_ptr(), target.data_ptr(), pred.numel(), kind, coeff, loss.data_ptr(),
               grad.data_ptr(), L.stream())
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        out = torch.empty_like(grad)
        L.call("a3d_scale_by_scalar", grad.data_ptr(), _c(g).data_ptr(), out.data_ptr(), grad.numel(), L.stream())
        return out, None, None, None


class SymQuatLossFn(torch.autograd.Function):
    """coeff * mean_b min(mse(q_b, g_b), mse(q_b, -g_b)): symmetric_rotation_loss of main_keypose.py:370-376"""

    @staticmethod
    def forward(ctx, pred, target, coeff):
        pred, target = _c(pred), _c(target.to(F32))
        loss = torch.empty((), device=pred.device, dtype=F32)
        grad = torch.empty_like(pred)
        L.call("a3d_sym_quat_loss", pred.data_ptr(), target.data_ptr(), 4, coeff, loss.data_ptr(), grad.data_ptr(),
               pred.shape[0], L.stream())
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        out = torch.empty_like(grad)
        L.call("a3d_scale_by_scalar", grad.data_ptr(), _c(g).data_ptr(), out.data_ptr(), grad.numel(), L.stream())
        return out, None, None


class QuatSigmoidFn(torch.autograd.Function):
    """pred (B,5) -> normalise_quat(pred[:, :4]), sigmoid(pred[:, 4:])   (act3d.py:526-533)"""

    @staticmethod
    def forward(ctx, pred):
        pred = _c(pred)
        B = pred.shape[0]
        rot = torch.empty((B, 4), device=pred.device, dtype=F32)
        grip = torch.empty((B, 1), device=pred.device, dtype=F32)
        L.call("a3d_quat_sigmoid_fwd", pred.data_ptr(), rot.data_ptr(), grip.data_ptr(), B, L.stream())
        ctx.save_for_backward(pred)
        return rot, grip

    @staticmethod
    def backward(ctx, drot, dgrip):
        (pred,) = ctx.saved_tensors
        dp = torch.empty_like(pred)
        drot = None if drot is None else _c(drot)        # bound to locals: both stay alive until the launch is enqueued
        dgrip = None if dgrip is None else _c(dgrip)
        L.call("a3d_quat_sigmoid_bwd", pred.data_ptr(), None if drot is None else drot.data_ptr(),
               None if dgrip is None else dgrip.data_ptr(), dp.data_ptr(), pred.shape[0], L.stream())
        return dp


class Ortho6dSigmoidFn(torch.autograd.Function):
    """pred (B,7) -> compute_rotation_matrix_from_ortho6d(pred[:, :6]) (B,3,3), sigmoid(pred[:, 6:])   (act3d.py:529-533)"""

    @staticmethod
    def forward(ctx, pred):
        pred = _c(pred)
        B = pred.shape[0]
        rot = torch.empty((B, 3, 3), device=pred.device, dtype=F32)
        grip = torch.empty((B, 1), device=pred.device, dtype=F32)
        L.call("a3d_ortho6d_sigmoid_fwd", pred.data_ptr(), rot.data_ptr(), grip.data_ptr(), B, L.stream())
        ctx.save_for_backward(pred)
        return rot, grip

    @staticmethod
    def backward(ctx, drot, dgrip):
        (pred,) = ctx.saved_tensors
        dp = torch.empty_like(pred)
        drot = None if drot is None else _c(drot)
        dgrip = None if dgrip is None else _c(dgrip)
        L.call("a3d_ortho6d_sigmoid_bwd", pred.data_ptr(), None if drot is None else drot.data_ptr(),
               None if dgrip is None else dgrip.data_ptr(), dp.data_ptr(), pred.shape[0], L.stream())
        return dp


class SelectRowFn(torch.autograd.Function):
    """x (B, N, W), idx (B,) int64 -> x[b, idx[b]] (B, W): the top ghost point's offset / feature row (act3d.py:513-522)."""

    @staticmethod
    def forward(ctx, x, idx):
        L.require_gpu(x, idx)
        x, idx = _c(x), _c(idx)
        B, N, W = x.shape
        y = torch.empty((B, W), device=x.device, dtype=F32)
        L.call("a3d_select_row_fwd", x.data_ptr(), idx.data_ptr(), y.data_ptr(), B, N, W, L.stream())
        ctx.idx, ctx.shape = idx, (B, N, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, N, W = ctx.shape
        dy = _c(dy)
        dx = torch.empty((B, N, W), device=dy.device, dtype=F32)
        L.call("a3d_select_row_bwd", dy.data_ptr(), ctx.idx.data_ptr(), dx.data_ptr(), B, N, W, L.stream())
        return dx, None


def sample_ghost_points(state, bounds, anchor, radius, B, Ng, level, max_attempts=64):
    """Device Philox sampler (a-3 of SURVEY §8a).  state: uint64[2] device tensor {seed, offset}."""
    out = torch.empty((B, Ng, 3), device=state.device, dtype=F32)
    L.call("a3d_sample_ghost_points", state.data_ptr(), bounds.data_ptr(),
           None if anchor is None else _c(anchor.to(F32)).data_ptr(), float(radius), out.data_ptr(), B, Ng, level,
           max_attempts, L.stream())
    return out


# ------------------------------------------------------------------------------------------------ diffusion pieces
class AdaLNFn(torch.autograd.Function):
    """x * (1 + scale) + shift with (scale, shift) = chunk(mod, 2)   (layers.py:281-290)"""

    @staticmethod
    def forward(ctx, x, mod):
        x, mod = _c(x), _c(mod)
        B, Ln, E = x.shape
        y = torch.empty_like(x)
        L.call("a3d_adaln_fwd", x.data_ptr(), mod.data_ptr(), y.data_ptr(), B, Ln, E, L.stream())
        ctx.save_for_backward(x, mod)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mod = ctx.saved_tensors
        B, Ln, E = x.shape
        dx = torch.empty_like(x)
        dmod = torch.empty_like(mod)
        L.call("a3d_adaln_bwd", x.data_ptr(), mod.data_ptr(), _c(dy).data_ptr(), dx.data_ptr(), dmod.data_ptr(), B, Ln,
               E, L.stream())
        return dx, dmod


class SiLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        y = torch.empty_like(x)
        L.call("a3d_silu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), L.stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        L.call("a3d_silu_bwd", x.data_ptr(), _c(dy).data_ptr(), dx.data_ptr(), x.numel(), L.stream())
        return dx


def sinusoidal_emb(x, E):
    x = _c(x.to(F32)).view(-1)
    out = torch.empty((x.numel(), E), device=x.device, dtype=F32)
    L.call("a3d_sinusoidal_emb", x.data_ptr(), out.data_ptr(), x.numel(), E, L.stream())
    return out


class AddRowsFn(torch.autograd.Function):
    """x (B, L, E) + r (L, E) broadcast over the batch; r's gradient (the batch sum) is computed only when it needs one."""

    @staticmethod
    def forward(ctx, x, r):
        x, r = _c(x), _c(r)
        B, Ln, E = x.shape
        y = torch.empty_like(x)
        L.call("a3d_add_rows", x.data_ptr(), r.data_ptr(), y.data_ptr(), B, Ln, E, L.stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        dr = None
        if ctx.needs_input_grad[1]:
            dy = _c(dy)
            B, Ln, E = dy.shape
            dr = torch.empty((Ln, E), device=dy.device, dtype=F32)
            L.call("a3d_add_rows_bwd", dy.data_ptr(), dr.data_ptr(), B, Ln, E, L.stream())
        return dy, dr


class TrajUpdateFn(torch.autograd.Function):
    """cat(traj[..., :3] + upd[..., :3], upd[..., 3:])   (diffusion_head.py:268-272).  `traj` needs a gradient only when it
    is a previous iteration's prediction (multi-round / multi-scale heads): d traj = [dy_xyz | 0]."""

    @staticmethod
    def forward(ctx, traj, upd):
        traj, upd = _c(traj), _c(upd)
        out = torch.empty_like(upd)
        L.call("a3d_traj_update", traj.data_ptr(), upd.data_ptr(), out.data_ptr(), upd.numel() // upd.shape[-1],
               upd.shape[-1], 3, L.stream())
        return out

    @staticmethod
    def backward(ctx, dy):
        dtraj = None
        if ctx.needs_input_grad[0]:
            dtraj = torch.zeros_like(dy)
            dtraj[..., :3] = dy[..., :3]
        return dtraj, dy


def ddpm_add_noise(x0, noise, t, acp_pos, acp_rot):
    x0, noise = _c(x0), _c(noise)
    B, Ln, D = x0.shape
    out = torch.empty_like(x0)
    L.call("a3d_ddpm_add_noise", x0.data_ptr(), noise.data_ptr(), _c(t.long()).data_ptr(), acp_pos.data_ptr(),
           acp_rot.data_ptr(), out.data_ptr(), B, Ln, D, 3, L.stream())
    return out


def ddpm_step(model_out, sample, noise, cond_data, cond_mask_u8, coef_pos, coef_rot, t, out=None):
    out = torch.empty_like(sample) if out is None else out
    L.call("a3d_ddpm_step", model_out.data_ptr(), sample.data_ptr(), None if noise is None else noise.data_ptr(),
           cond_data.data_ptr(), cond_mask_u8.data_ptr(), coef_pos.data_ptr(), coef_rot.data_ptr(), out.data_ptr(),
           sample.numel() // sample.shape[-1], sample.shape[-1], 3, int(t), L.stream())
    return out


def ddpm_step_sched(model_out, sample, noise, cond_data, cond_mask_u8, coef_pos, coef_rot, row, terminal, out=None, hist=None,
                    kappa_pos=None, kappa_rot=None):
    """ddpm_step on [K][3] tables indexed by step position (diffusion.SamplerSchedule): row = the step's position, terminal = the
    step returns the in-painted network output.  hist / kappa_pos / kappa_rot (all three): the history term of a multistep
    schedule (a3d_ddpm_step_hist) -- hist, the shape of sample, is read where kappa[row] != 0 and updated in place."""
    out = torch.empty_like(sample) if out is None else out
    args = (model_out.data_ptr(), sample.data_ptr(), None if noise is None else noise.data_ptr(),
            cond_data.data_ptr(), cond_mask_u8.data_ptr(), coef_pos.data_ptr(), coef_rot.data_ptr(), out.data_ptr(),
            sample.numel() // sample.shape[-1], sample.shape[-1], 3, int(row), int(bool(terminal)))
    if hist is None and kappa_pos is None and kappa_rot is None:
        L.call("a3d_ddpm_step_sched", *args, L.stream())
    else:
        assert hist is None or (hist.shape == sample.shape and hist.is_contiguous() and hist.dtype == torch.float32)
        L.call("a3d_ddpm_step_hist", *args, *(None if x is None else x.data_ptr() for x in (hist, kappa_pos, kappa_rot)), L.stream())
    return out


# ------------------------------------------------------------------------------------------------ inference K/V cache
# The (k, v) group and the q group of mode "kv" in the bf16 family, forward only: the cache holds K rows and V planes, the query rows only.
def kv_cache_build(k_in, k_xyz, mha, H):
    """Step-invariant K/V operands of one cross-attention layer (context projected, rotated, split) -- computed once per
    trajectory batch instead of once per denoise step (SURVEY §0 "re-encodes ... every step", §8f-2)."""
    k_in = _c(k_in)
    B, S, E = k_in.shape
    k_xyz = None if k_xyz is None else _c(k_xyz.to(F32))
    _, Ks, Vt, _, Sp, _, _, _ = _operands(False, PROJ_GROUPS["kv"][1:], (None, k_in, k_in), mha.in_proj_weight.data_ptr(),
                                          mha.in_proj_bias.data_ptr(), None, k_xyz, B, S, S, E, H, k_in.device, False,
                                          fused=_fused_proj(E))
    return {"Ks": Ks, "Vt": Vt, "S": S, "Sp": Sp}


def ctx_kv_cache16(ctx, xyz, mha, H):
    """Step-invariant context operands of one cross-attention layer of the fused sampler (csrc/denoise.hip) -> (Kf [B][H][Sp][32] fp16
    hi | lo rows, rotated by xyz; Vt [B][H][2][16][Sp] fp16 hi / lo planes with the ones channel): the (k, v) group of mode "kv" through
    write_operands.  dn_cross reads K rows + V planes whatever the training side uses, so neither _rows_only() nor ATTN_MODE is asked."""
    ctx, xyz = _c(ctx), _c(xyz.to(F32))
    B, S, E = ctx.shape
    Sp, dev = ceil_to(S, 64), ctx.device
    Kf, Vt = (torch.empty(shape, device=dev, dtype=torch.float16) for shape in ((B, H, Sp, 32), (B, H, 2, 16, Sp)))
    write_operands(True, PROJ_GROUPS["kv"][1:], {"k": Role(xyz, 1.0, S, Sp), "v": Role(None, 1.0, S, Sp)},
                   {"k": Slot(Kf, None, PLANE_PARTS), "v": Slot(None, Vt, V_PLANES)}, rope_freq(E, dev), B, E, H, dev, (None, ctx, ctx),
                   mha.in_proj_weight.data_ptr(), mha.in_proj_bias.data_ptr(), fused=_fused_proj(E))
    return Kf, Vt


@torch.no_grad()
def attn_block_cached(q_in, resid, q_xyz, cache, mha, norm, H):
    """Inference-only cross-attention block against a prebuilt K/V cache: q-proj + RoPE + attention + out-proj + add&LN."""
    q_in, resid = _c(q_in), _c(resid)
    B, Lq, E = q_in.shape
    q_xyz = None if q_xyz is None else _c(q_xyz.to(F32))
    Qs, _, _, Lqp, _, _, _, _ = _operands(False, PROJ_GROUPS["kv"][:1], (q_in, None, None), mha.in_proj_weight.data_ptr(),
                                          mha.in_proj_bias.data_ptr(), q_xyz, None, B, Lq, cache["S"], E, H, q_in.device, False,
                                          fused=_fused_proj(E))
    nsplit = pick_nsplit(B, H, Lqp, cache["Sp"])
    O_, _ = attn_core_fwd(Qs, cache["Ks"], cache["Vt"], None, B, H, Lq, Lqp, cache["S"], cache["Sp"], nsplit)
    Y = linear2d(O_.view(B * Lq, E), mha.out_proj.weight, mha.out_proj.bias)
    y, _, _ = add_layernorm(resid.view(B * Lq, E), Y, norm.weight, norm.bias)
    return y.view(B, Lq, E)
