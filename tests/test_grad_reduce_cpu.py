"""Host side of the deferred gradient reductions: the queries (partial counts, workspace sizes), the argument checks of the new
entries (they return before anything is launched) and the table builder (destination grouping and order).  No GPU needed."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib(a3d):
    return a3d.lib.load()


def test_layernorm_partial_count(lib):
    cnt = lib.a3d_add_layernorm_bwd_partials_count
    assert cnt(21312, 60) == 167                           # the ghost-token rows of the bench shape: 128 rows per workgroup
    for M in (1, 3, 4, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 21312, 1 << 20, 1 << 30):
        for E in (4, 12, 60, 64):
            n = cnt(M, E)
            rows = -(-(-(-M // 256)) // 64) * 64           # whole 64-row passes, at most 256 workgroups
            assert 1 <= n <= 256 and n == -(-M // rows)
            assert (n - 1) * rows < M <= n * rows          # contiguous blocks that cover the rows, none empty
    for M, E in ((0, 60), (-5, 60), (100, 0), (100, 62), (100, 68), (100, 120), (100, 128), (100, 512)):
        assert cnt(M, E) == 0                              # not served: the caller keeps the other kernels


def test_wgrad_partials_follow_the_two_stage_plan(a3d, lib):
    L = a3d.lib
    ns = ctypes.c_int(-1)
    fake = 0x1000                                          # never dereferenced: every call below fails its checks first
    assert lib.a3d_linear_wgrad_ws_bytes(1000, 60, 60, 1) == 0
    with pytest.raises(RuntimeError, match="one-stage"):
        L.call("a3d_linear_wgrad_partials", fake, 60, fake, 60, 1, 1000, 60, 60, fake, 1 << 30, ctypes.byref(ns), None)
    need = lib.a3d_linear_wgrad_ws_bytes(21312, 60, 60, 1)
    assert need > 0 and need % (4 * 60 * 61) == 0
    assert need // (4 * 60 * 61) == 333                    # the slab count of the bench shape's ghost-stream linears
    with pytest.raises(RuntimeError, match="workspace too small"):
        L.call("a3d_linear_wgrad_partials", fake, 60, fake, 60, 1, 21312, 60, 60, fake, need - 4, ctypes.byref(ns), None)
    for bad in [(None, 60, fake, 60, 1, 21312, 60, 60, fake, need, ctypes.byref(ns), None),
                (fake, 60, fake, 60, 1, 21312, 60, 60, None, need, ctypes.byref(ns), None),
                (fake, 60, fake, 60, 1, 21312, 60, 60, fake, need, None, None),
                (fake, 60, fake, 60, 1, 0, 60, 60, fake, need, ctypes.byref(ns), None),
                (fake, 60, fake, 60, 1, 21312, 0, 60, fake, need, ctypes.byref(ns), None)]:
        with pytest.raises(RuntimeError, match="bad argument"):
            L.call("a3d_linear_wgrad_partials", *bad)
    assert ns.value == -1


def test_other_entries_reject_bad_arguments(a3d):
    L = a3d.lib
    fake = 0x1000
    with pytest.raises(RuntimeError, match="a3d_add_layernorm_bwd_partials"):        # E = 120 is not this entry's
        L.call("a3d_add_layernorm_bwd_partials", fake, None, fake, fake, fake, fake, fake, fake, 100, 120, None)
    with pytest.raises(RuntimeError, match="a3d_add_layernorm_bwd_partials"):        # no record buffer
        L.call("a3d_add_layernorm_bwd_partials", fake, None, fake, fake, fake, fake, fake, None, 100, 60, None)
    with pytest.raises(RuntimeError, match="a3d_add_layernorm_bwd_partials"):        # rows that are not 16-byte aligned
        L.call("a3d_add_layernorm_bwd_partials", fake + 4, None, fake, fake, fake, fake, fake, fake, 100, 60, None)
    with pytest.raises(RuntimeError, match="a3d_colsum_rows_partials"):
        L.call("a3d_colsum_rows_partials", fake, 2, 10, 11, 60, 60, fake, None)       # k > S
    with pytest.raises(RuntimeError, match="a3d_grad_reduce_table"):
        L.call("a3d_grad_reduce_table", None, 1, 1, None)
    with pytest.raises(RuntimeError, match="a3d_grad_reduce_table"):
        L.call("a3d_grad_reduce_table", fake, 1, 0, None)


def _rec(partial=0x1000, nsplit=3, slab=100, count=100, row_len=10, dst=0x9000, stride=10, bias=None):
    return (partial, nsplit, slab, count, row_len, dst, stride, bias)


def test_table_builder_groups_destinations_in_order(a3d):
    O = a3d.ops
    recs = [_rec(0x100, dst=0xA000), _rec(0x200, count=60 * 61, slab=60 * 61, row_len=61, dst=0xB000, stride=60, bias=0xC000),
            _rec(0x300, nsplit=7, dst=0xA000), _rec(0x400, dst=0xD000), _rec(0x500, nsplit=1, dst=0xA000),
            _rec(0x600, count=60 * 61, slab=2 * 60 * 61, row_len=61, dst=0xB000, stride=60, bias=0xC000),
            _rec(0x700, dst=0xB000)]                      # the same pointer as a differently shaped destination: its own group
    t = O.build_reduce_table(recs)
    assert len(t) == len(recs)
    got = [(r.partial, r.dst, r.group_len, r.nsplit) for r in t]
    assert got == [(0x100, 0xA000, 3, 3), (0x300, 0xA000, 0, 7), (0x500, 0xA000, 0, 1),       # groups by first appearance,
                   (0x200, 0xB000, 2, 3), (0x600, 0xB000, 0, 3),                              # members in append order
                   (0x400, 0xD000, 1, 3), (0x700, 0xB000, 1, 3)]
    assert t[3].bias == 0xC000 and t[4].slab_stride == 2 * 60 * 61 and t[0].bias is None
    nwg = ctypes.c_int(0)
    a3d.lib.call("a3d_grad_reduce_table_plan", t, len(t), ctypes.byref(nwg))
    assert nwg.value == 2 + 58 + 2 + 2                     # 64-output chunks per GROUP: 100 -> 2, 60 * 61 -> 58


def test_table_plan_rejects_malformed_tables(a3d):
    O, L = a3d.ops, a3d.lib
    nwg = ctypes.c_int(0)

    def plan(t, n=None):
        L.call("a3d_grad_reduce_table_plan", t, len(t) if n is None else n, ctypes.byref(nwg))

    good = [_rec(0x100), _rec(0x200), _rec(0x300, dst=0xB000)]
    plan(O.build_reduce_table(good))
    for field, value in (("group_len", 0), ("group_len", 4), ("dst", None), ("count", 0), ("row_len", 0), ("dst_stride", 9)):
        t = O.build_reduce_table(good)
        setattr(t[0], field, value)
        with pytest.raises(RuntimeError, match="group leader"):
            plan(t)
    for field, value in (("partial", None), ("nsplit", 0), ("slab_stride", 99), ("count", 90), ("row_len", 5), ("dst", 0xF000),
                         ("bias", 0xF000), ("dst_stride", 20), ("group_len", 1)):
        t = O.build_reduce_table(good)
        setattr(t[1], field, value)
        with pytest.raises(RuntimeError, match="does not match its group leader"):
            plan(t)
    with pytest.raises(RuntimeError, match="bad argument"):
        plan(O.build_reduce_table(good), 0)
    t = O.build_reduce_table([_rec(count=61, slab=61, row_len=61, stride=0, bias=0xC000)])
    with pytest.raises(RuntimeError, match="group leader"):           # 60 weight columns in a row stride of 0
        plan(t)
    plan(O.build_reduce_table([_rec(count=5, slab=5, row_len=1, stride=0, bias=0xC000)]))     # bias only: no weight column at all


def test_queue_takes_nothing_outside_a_backward_pass(a3d):
    O = a3d.ops
    assert O.reduce_queue("cpu") is None or O.ReduceQueue.current is not None
    q = O.ReduceQueue()                                    # no stream: as when the forward ran without a GPU
    assert q.accepts("cpu") is False and q.records == []
    q.flush()                                              # nothing pending: no launch, no error
    assert O.ReduceQueue.flushes >= 0
