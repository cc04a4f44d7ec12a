"""a3d_ctx_kv_proj16 (csrc/ctx_proj.hip) rejects what it does not serve on the host, before any launch, with the library's error code
and an error string naming the entry point (tests/test_ctx_kv_proj_gpu.py runs the accepted calls).  No device needed."""
import ctypes

from conftest import load_pkg


def test_ctx_kv_proj_argument_validation_without_gpu():
    a3d = load_pkg()
    lib = a3d.lib.load()
    d = ctypes.c_void_p(64)                                                          # 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(68)                                                        # 4-byte aligned only

    def args(X=d, ldx=60, W0=d, K0=d, V0=d, W1=d, K1=d, V1=d, ldw=60, nl=2, B=1, N=10, Npad=64, E=60, H=4, nsplit=0, xyz=None,
             freq=None):
        return (X, ldx, xyz, W0, None, K0, V0, W1, None, K1, V1, ldw, freq, nl, B, N, Npad, E, H, nsplit, None)

    def refused(**kw):
        assert lib.a3d_ctx_kv_proj16(*args(**kw)) == -22, kw
        assert b"a3d_ctx_kv_proj16" in lib.a3d_last_error_string(), (kw, lib.a3d_last_error_string())

    refused(nl=0)
    refused(nl=3)
    refused(E=120, H=8)                                                              # the other model's width
    refused(E=30, H=2)
    refused(E=61)                                                                    # E != 15 H
    refused(H=5)
    refused(Npad=72)                                                                 # Npad % 64
    refused(Npad=0)                                                                  # Npad < N
    refused(N=0)
    refused(B=0)
    refused(K0=None)                                                                 # null outputs
    refused(V0=None)
    refused(K1=None)
    refused(V1=None)
    refused(W0=None)
    refused(W1=None)
    refused(X=None)
    refused(X=odd)                                                                   # X not 16-byte aligned
    refused(K0=odd)                                                                  # outputs are written as 16-byte segments
    refused(ldx=62)                                                                  # ldx % 4
    refused(ldx=56)                                                                  # ldx < E
    refused(ldw=59)
    refused(xyz=d)                                                                   # xyz without freq
    refused(nsplit=-1)
    # the default split count is at least one workgroup per sample, whatever the geometry
    assert lib.a3d_ctx_kv_proj16_splits(64, 4160) >= 1
    assert lib.a3d_ctx_kv_proj16_splits(0, 0) == 1
