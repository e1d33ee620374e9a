"""csrc/conv5x5_half.hip without a GPU: the host arithmetic of its C ABI, and what the compiler made of the kernel."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shapes_strides_and_sizes():
    from sbmc_amd import _lib
    L = _lib.lib()
    assert [L.sbmc_conv5x5_padded_channels(c) for c in (0, 1, 16, 27, 100, 441)] == [0, 16, 16, 32, 112, 448]
    assert L.sbmc_conv5x5_half_supported(1, 720, 1280, 27, 100) == 1 and L.sbmc_conv5x5_half_supported(1, 5, 5, 1, 1) == 1
    assert L.sbmc_conv5x5_half_supported(2, 720, 1280, 100, 441) == 1
    assert L.sbmc_conv5x5_half_supported(1, 4, 720, 27, 100) == 0 and L.sbmc_conv5x5_half_supported(1, 720, 4, 27, 100) == 0
    assert L.sbmc_conv5x5_half_supported(1, 9, 9, 0, 8) == 0 and L.sbmc_conv5x5_half_supported(1, 9, 9, 8, 0) == 0
    assert L.sbmc_conv5x5_half_supported(0, 9, 9, 8, 8) == 0
    assert L.sbmc_conv5x5_half_supported(1, 8, 2000000, 441, 441) == 0      # a patch row beyond 31 bits of byte offset
    # K rounded up to 16, N to the 128-channel tile; a stage = 5 taps x 2 octets x 128 entries of 16 bytes
    assert L.sbmc_conv5x5_half_weights_bytes(100, 441) == 4 * 7 * 5 * 20480
    assert L.sbmc_conv5x5_half_weights_bytes(100, 0) == 0 and L.sbmc_conv5x5_half_weights_bytes(0, 8) == 0


def test_null_pointers_are_refused_without_a_launch():
    from sbmc_amd import _lib
    L = _lib.lib()
    assert L.sbmc_conv5x5_half_bias_act_nhwc(None, 32, None, None, None, 112, 1, 9, 9, 27, 100, 0.0, None) == -1
    assert L.sbmc_conv5x5_half_prepare_weights(None, 675, 25, 5, 1, 27, 100, None, None) == -1
    assert L.sbmc_conv5x5_half_pack_nchw_f32(None, None, 32, 1, 27, 81, None) == -1
    assert L.sbmc_conv5x5_half_pack_nchw_f16(None, None, 32, 1, 27, 81, None) == -1
    assert L.sbmc_conv5x5_half_unpack_nhwc(None, 112, None, 1, 100, 25, None) == -1


@pytest.mark.slow
def test_conv5_half_kernel_does_not_spill():
    """One wave per SIMD on the whole register file, 256 of it accumulators: a spill goes to scratch inside the MFMA
    stream.  133 632 bytes of dynamic LDS (two patch buffers + two weight stages) on top of what the file declares."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = kernel_resources.resources(os.path.join(ROOT, "sbmc_amd", "csrc", "conv5x5_half.hip"))
    main = [r for r in rows if "conv5_half_kernel" in r["name"]]
    assert len(main) == 1 and len(rows) == 5, rows
    for r in rows:
        assert r["scratch"] == 0 and r["spill"] == 0, r
        assert r["lds"] <= 160 * 1024, r
    assert main[0]["occupancy"] == 1 and main[0]["agprs"] == 256, main
    assert main[0]["lds"] + (2 * 4 * 724 + 2 * 1280) * 16 <= 160 * 1024, main
