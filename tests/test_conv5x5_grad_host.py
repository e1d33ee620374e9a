"""csrc/conv5x5_grad.hip without a GPU: the host arithmetic of its C ABI, and what the compiler made of its kernels."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_supported_and_scratch_sizes():
    from sbmc_amd import _lib
    L = _lib.lib()
    for ok in (L.sbmc_conv5x5_dgrad_supported, L.sbmc_conv5x5_wgrad_supported):
        assert ok(1, 720, 1280, 100, 441) == 1 and ok(1, 5, 5, 1, 1) == 1
        assert ok(1, 4, 720, 27, 100) == 0 and ok(1, 720, 4, 27, 100) == 0 and ok(1, 9, 9, 0, 8) == 0
        assert ok(1, 8, 40000000, 27, 8) == 0                  # a row beyond 31 bits of byte offset
    assert L.sbmc_conv5x5_dgrad_supported(1, 8, 2000000, 27, 8) == 0        # 21 patch rows beyond 31 bits; one row is not
    assert L.sbmc_conv5x5_wgrad_supported(1, 8, 2000000, 27, 8) == 1
    # per range: [ky 5][128][64] partial sums per (tap column, 128-channel output tile, 64-channel input tile) + 128 bias
    # sums per output tile; 5 x 5 input: one row stage, one range
    per_range = lambda cin, cout: (-(-cout // 128) * -(-cin // 64) * 5 * 5 * 128 * 64 + -(-cout // 128) * 128) * 4
    assert L.sbmc_conv5x5_wgrad_scratch_bytes(1, 5, 5, 100, 441) == per_range(100, 441)
    many = L.sbmc_conv5x5_wgrad_scratch_bytes(1, 720, 1280, 100, 100)
    assert many % per_range(100, 100) == 0 and many // per_range(100, 100) >= 2
    assert L.sbmc_conv5x5_wgrad_scratch_bytes(1, 4, 9, 100, 100) == 0
    assert L.sbmc_conv5x5_wgrad_bias_f32(None, 16, None, None, 32, None, None, 675, 25, 5, 1, None, None, 1, 9, 9, 27, 8, None) == -1
    assert L.sbmc_conv5x5_dgrad_adj_nhwc_f32(None, 16, None, None, None, 1.0, None, 32, 1, 9, 9, 27, 8, None, None) == -1


@pytest.mark.slow
def test_gradient_kernels_do_not_spill():
    """dgrad: the forward's budget, one wave per SIMD on the whole register file; wgrad: 160 accumulator registers and 80 KB of
    LDS, two workgroups per CU."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.resources(os.path.join(ROOT, "sbmc_amd", "csrc", "conv5x5_grad.hip"))
    for r in rows:
        assert r["scratch"] == 0 and r["spill"] == 0, r
    occ = {k: [r["occupancy"] for r in rows if k in r["name"]] for k in ("conv5_dgrad_kernel", "conv5_wgrad_kernel")}
    assert occ == {"conv5_dgrad_kernel": [1], "conv5_wgrad_kernel": [2]}, rows
