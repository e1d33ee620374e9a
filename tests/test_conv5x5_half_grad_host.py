"""csrc/conv5x5_half_grad.hip without a GPU: the host arithmetic of its C ABI, and what the compiler made of its kernels."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_supported_and_scratch_sizes():
    from sbmc_amd import _lib
    L = _lib.lib()
    for ok in (L.sbmc_conv5x5_half_dgrad_supported, L.sbmc_conv5x5_half_wgrad_supported):
        assert ok(1, 720, 1280, 100, 441) == 1 and ok(1, 5, 5, 1, 1) == 1
        assert ok(1, 4, 720, 27, 100) == 0 and ok(1, 720, 4, 27, 100) == 0 and ok(1, 9, 9, 0, 8) == 0
        assert ok(1, 8, 80000000, 27, 8) == 0                  # a row beyond 31 bits of byte offset
    assert L.sbmc_conv5x5_half_dgrad_supported(1, 8, 2000000, 27, 8) == 0   # 37 patch rows beyond 31 bits; one row is not
    assert L.sbmc_conv5x5_half_wgrad_supported(1, 8, 2000000, 27, 8) == 1
    # per range: [ky 5][128][64] partial sums per (tap column, 128-channel output tile, 64-channel input tile) + 128 bias
    # sums per output tile; 5 x 5 input: one row stage, one range
    per_range = lambda cin, cout: (-(-cout // 128) * -(-cin // 64) * 5 * 5 * 128 * 64 + -(-cout // 128) * 128) * 4
    assert L.sbmc_conv5x5_half_wgrad_scratch_bytes(1, 5, 5, 100, 441) == per_range(100, 441)
    many = L.sbmc_conv5x5_half_wgrad_scratch_bytes(1, 720, 1280, 100, 100)
    assert many % per_range(100, 100) == 0 and many // per_range(100, 100) >= 2
    assert L.sbmc_conv5x5_half_wgrad_scratch_bytes(1, 4, 9, 100, 100) == 0


def test_null_pointers_are_refused_without_a_launch():
    from sbmc_amd import _lib
    L = _lib.lib()
    assert L.sbmc_conv5x5_half_wgrad_bias(None, 16, None, 32, None, 675, 25, 5, 1, None, None, 1, 9, 9, 27, 8, None) == -1
    assert L.sbmc_conv5x5_half_dgrad_adj_nhwc(None, 16, None, None, 1.0, None, 32, 1, 9, 9, 27, 8, None) == -1
    assert L.sbmc_conv5x5_half_pack_adj_nchw_f32(None, None, 0.0, None, 16, 1, 8, 25, None) == -1
    assert L.sbmc_conv5x5_half_pack_adj_nchw_f16(None, None, 0.0, None, 16, 1, 8, 25, None) == -1
    assert L.sbmc_conv5x5_half_unpack_nhwc_f32(None, 32, None, 1, 27, 81, None) == -1
    assert L.sbmc_conv5x5_half_pack_adj_nchw_f32(None, None, 0.0, None, 16, 0, 8, 25, None) == 0     # an empty problem
    assert L.sbmc_conv5x5_half_unpack_nhwc_f32(None, 32, None, 1, 27, 0, None) == 0


@pytest.mark.slow
def test_half_gradient_kernels_do_not_spill():
    """dgrad: the half forward's budget, one wave per SIMD, 256 accumulators, 133 632 bytes of dynamic LDS; wgrad: 160
    accumulators + 40 held operand registers within 256, two waves per SIMD, 44 032 bytes of dynamic LDS a workgroup."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.resources(os.path.join(ROOT, "sbmc_amd", "csrc", "conv5x5_half_grad.hip"))
    for r in rows:
        assert r["scratch"] == 0 and r["spill"] == 0, r
    main = {k: [r for r in rows if k in r["name"]] for k in ("conv5_half_dgrad_kernel", "conv5_half_wgrad_kernel")}
    assert [len(v) for v in main.values()] == [1, 1], rows
    dgrad, wgrad = main["conv5_half_dgrad_kernel"][0], main["conv5_half_wgrad_kernel"][0]
    assert dgrad["occupancy"] == 1 and wgrad["occupancy"] == 2, (dgrad, wgrad)
    assert dgrad["lds"] + (2 * 4 * 724 + 2 * 1280) * 16 <= 160 * 1024, dgrad
    assert 2 * (wgrad["lds"] + (2 * 4 * 128 + 6 * 4 * 72) * 16) <= 160 * 1024, wgrad
