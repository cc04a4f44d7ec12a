"""Host-side argument checks of the conv3 + bn3 + residual route (no GPU: nothing is launched)."""
import ctypes

from conftest import load_pkg


def test_conv3_residual_and_gram_entry_points_validate_arguments_without_gpu():
    a3d = load_pkg()
    a3d.build()
    lib = a3d.lib.load()
    dummy = ctypes.c_void_p(64)                                                      # aligned, never dereferenced
    assert lib.a3d_conv1x1_bn_residual_serves(64, 256) == 1 and lib.a3d_conv1x1_bn_residual_serves(128, 512) == 1
    for K, N in [(64, 64), (256, 512), (64, 320)]:
        assert lib.a3d_conv1x1_bn_residual_serves(K, N) == 0
        assert lib.a3d_conv1x1_bn_residual_fwd(dummy, dummy, None, None, 0, dummy, dummy, dummy, None, None, 1, 0, dummy, 16, K, N, None) == -22
        assert b"a3d_conv1x1_bn_residual_fwd" in lib.a3d_last_error_string()
    args = (dummy, dummy, None, None, 0, dummy, dummy)
    assert lib.a3d_conv1x1_bn_residual_fwd(*args, None, None, None, 1, 0, dummy, 16, 64, 256, None) == -22       # no residual
    assert lib.a3d_conv1x1_bn_residual_fwd(*args, dummy, dummy, None, 1, 0, dummy, 16, 64, 256, None) == -22     # res_scale without res_shift
    assert lib.a3d_conv1x1_bn_residual_fwd(*args, ctypes.c_void_p(72), None, None, 1, 0, dummy, 16, 64, 256, None) == -22   # alignment
    assert lib.a3d_conv1x1_bn_residual_fwd(dummy, dummy, None, None, 0, None, dummy, dummy, None, None, 1, 0, dummy, 16, 64, 256, None) == -22
    # the statistics-only call of a3d_conv1x1_bn_fwd (y NULL): only with partial sums, only on the two conv3 shapes
    assert lib.a3d_conv1x1_bn_fwd(dummy, dummy, None, None, 0, None, None, 128, 64, 256, None) == -22
    assert lib.a3d_conv1x1_bn_fwd(dummy, dummy, None, None, 0, None, dummy, 128, 64, 64, None) == -22
    # Gram slabs: chunks of 8192 / K rows, at most 512 (K = 64) / 256 (K = 128) slabs, other widths not served
    assert lib.a3d_bn_gram_nslab(130, 64) == 2 and lib.a3d_bn_gram_nslab(1 << 20, 64) == 512
    assert lib.a3d_bn_gram_nslab(4096, 128) == 64 and lib.a3d_bn_gram_nslab(1 << 18, 128) == 256
    assert lib.a3d_bn_gram_nslab(1000, 256) == 0 and lib.a3d_bn_gram_nslab(0, 64) == 0
    assert lib.a3d_bn_gram(dummy, None, None, 0, dummy, dummy, 1000, 256, 1, None) == -22                    # K not served
    assert lib.a3d_bn_gram(dummy, None, None, 0, dummy, dummy, 1000, 64, 3, None) == -22                     # nslab != a3d_bn_gram_nslab
    assert lib.a3d_bn_gram(dummy, dummy, None, 1, dummy, dummy, 130, 64, 2, None) == -22                     # scale without shift
    assert b"a3d_bn_gram" in lib.a3d_last_error_string()
    assert lib.a3d_bn_gram_stats(dummy, dummy, 2, dummy, 64, 254, dummy, dummy, None) == -22                 # N % 4
    assert lib.a3d_bn_gram_stats(dummy, dummy, 0, dummy, 64, 256, dummy, dummy, None) == -22                 # no slabs
    assert lib.a3d_bn_gram_stats(dummy, dummy, 2, dummy, 64, 256, None, dummy, None) == -22                  # no scratch
