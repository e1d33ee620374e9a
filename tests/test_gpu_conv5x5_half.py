"""The half 5 x 5 valid convolution (csrc/conv5x5_half.hip) behind KPCN's chains under torch.autocast(float16): a layer
against float64 of the SAME half inputs and half-rounded weights (the contract of tests/test_gpu_conv3x3_half.py: one half
rounding of the result + fp32 summation noise), a chain and the whole model against the library's half run."""
import ctypes

import pytest
import torch as th
import torch.nn.functional as F

from helpers import KernelApplyFP64, float64_twin, no_worse_than
from sbmc_amd import KPCN, _lib
from sbmc_amd import functions as funcs
from sbmc_amd import modules as ops

pytestmark = pytest.mark.gpu

HALF_ULP = 2.0 ** -11


def _dev():
    if not th.cuda.is_available():
        pytest.skip("needs a GPU")
    return th.device("cuda")


def _check_half(a, ref, what):
    """|a - ref| <= one half rounding of ref (+ fp32 summation noise relative to the tensor's scale)"""
    a, ref = a.detach().cpu().double(), ref.double()
    err = (a - ref).abs()
    print("%s: worst %.3e of scale" % (what, (err.max() / ref.abs().max()).item()))
    bad = err > HALF_ULP * 1.01 * ref.abs() + 1e-5 * ref.abs().max()
    assert not bad.any(), "%s: %d / %d beyond one half rounding, worst %.3e of scale" % (
        what, int(bad.sum()), ref.numel(), (err.max() / ref.abs().max()).item())


def _layer(b, cin, cout, h, w, dtype, seed=0):
    g = th.Generator(device="cpu").manual_seed(seed + b * 1000 + cin + cout + h * w)
    x = th.randn(b, cin, h, w, generator=g).to(dtype)
    wt = th.randn(cout, cin, 5, 5, generator=g) * (2.0 / (25 * cin)) ** 0.5
    bias = th.randn(cout, generator=g) * 0.5
    ref = F.conv2d(x.half().double(), wt.half().double(), bias.double())
    return x, wt, bias, ref


@pytest.mark.parametrize("b,cin,cout,h,w,dtype", [
    (1, 27, 100, 36, 20, th.float32),    # exactly one 32 x 16 tile, the first layer: planar fp32 in, a partial granule
    (2, 100, 100, 37, 21, th.float16),   # one pixel more each way, batch: ragged tiles, seven granules (a half chunk last)
    (1, 100, 441, 52, 20, th.float16),   # one and a half tiles; four output-channel tiles, the last one ragged
    (1, 6, 8, 9, 9, th.float32),         # an output smaller than a tile, less than one granule
    (1, 100, 25, 5, 5, th.float16),      # a single output pixel
])
def test_single_layer_matches_float64(b, cin, cout, h, w, dtype):
    dev = _dev()
    x, wt, bias, ref = _layer(b, cin, cout, h, w, dtype)
    for act, fn in ((0, lambda v: v), (1, th.relu)):
        y = funcs.conv5x5_chain_half(x.to(dev), [(wt.to(dev), bias.to(dev), act, 0.0)])
        assert y.dtype == th.float16 and y.shape == (b, cout, h - 4, w - 4) and y.is_contiguous()
        _check_half(y, fn(ref), "conv5x5 half %s act %d" % ((b, cin, cout, h, w), act))


def test_padding_channels_stay_zero_through_the_raw_abi():
    dev = _dev()
    L = _lib.lib()
    b, cin, cout, h, w = 1, 27, 100, 37, 21
    x, wt, bias, ref = _layer(b, cin, cout, h, w, th.float32, seed=5)
    x, wt, bias = x.to(dev), wt.to(dev), bias.to(dev) + 1.0           # (a bias that would show in a padding channel)
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    ldx, ldy = L.sbmc_conv5x5_padded_channels(cin), L.sbmc_conv5x5_padded_channels(cout)
    xb = th.full((b, h, w, ldx), 7.0, dtype=th.float16, device=dev)
    yb = th.full((b, h - 4, w - 4, ldy), 7.0, dtype=th.float16, device=dev)
    wp = th.empty(L.sbmc_conv5x5_half_weights_bytes(cin, cout), dtype=th.uint8, device=dev)
    assert L.sbmc_conv5x5_half_pack_nchw_f32(p(x), p(xb), ldx, b, cin, h * w, None) == 0
    assert L.sbmc_conv5x5_half_prepare_weights(p(wt), *wt.stride(), cin, cout, p(wp), None) == 0
    assert L.sbmc_conv5x5_half_bias_act_nhwc(p(xb), ldx, p(wp), p(bias), p(yb), ldy, b, h, w, cin, cout, 1.0, None) == 0
    th.cuda.synchronize()
    assert (xb[..., cin:] == 0).all() and th.equal(xb[..., :cin], x.half().permute(0, 2, 3, 1))
    assert (yb[..., cout:] == 0).all()
    _check_half(yb[..., :cout].permute(0, 3, 1, 2), ref + 1.0, "raw ABI")
    for bad in (dict(h=4), dict(ldx=16), dict(ldy=104)):
        a = dict(h=h, ldx=ldx, ldy=ldy)
        a.update(bad)
        assert L.sbmc_conv5x5_half_bias_act_nhwc(p(xb), a["ldx"], p(wp), p(bias), p(yb), a["ldy"], b, a["h"], w, cin, cout,
                                                 1.0, None) == -1, bad


def test_chain_under_autocast_against_the_library(monkeypatch):
    dev = _dev()
    th.manual_seed(11)
    make = lambda: ops.ConvChain(27, 441, ksize=5, width=100, depth=3, pad=False, weight_norm=False, activation="relu")
    net = make().to(dev)
    for q in net.parameters():
        if q.dim() == 1:
            q.data.normal_(0.0, 0.1)
    x = th.randn(1, 27, 29, 33, device=dev)
    with th.no_grad():
        truth = float64_twin(net, make)(x.cpu().double())
        with th.autocast("cuda", dtype=th.float16):
            monkeypatch.setenv("SBMC_CONV5X5_HALF", "0")
            lib = net(x)
            monkeypatch.setenv("SBMC_CONV5X5_HALF", "1")
            y = net(x)
    assert y.dtype == th.float16 and y.shape == (1, 441, 17, 21) and y.is_contiguous()
    no_worse_than(y, lib, truth, rtol=2.0 ** -10, slack=2.0, what="chain")


def test_kpcn_dispatch_under_autocast(monkeypatch):
    """no_grad + float16 autocast runs on the kernel (the library convolution raises); SBMC_CONV5X5_HALF = 0 and gradients
    wanted leave everything where it was."""
    dev = _dev()
    th.manual_seed(4)
    model = KPCN(27, ksize=5).to(dev)
    for name, q in model.named_parameters():
        if name.endswith("bias"):
            q.data.normal_(0.0, 0.1)
    data = {k: th.randn(1, 27, 53, 53, device=dev) for k in ("kpcn_diffuse_in", "kpcn_specular_in")}
    data.update({k: th.rand(1, 3, 53, 53, device=dev) for k in ("kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo")})
    m64 = float64_twin(model, lambda: KPCN(27, ksize=5))
    m64.kernel_apply = KernelApplyFP64()
    with th.no_grad():
        r64 = m64({k: v.cpu().double() for k, v in data.items()})
    with th.autocast("cuda", dtype=th.float16):
        monkeypatch.setenv("SBMC_CONV5X5_HALF", "0")
        with th.no_grad():
            lib = model(data)
        lib_grad = model(data)
        monkeypatch.setenv("SBMC_CONV5X5_HALF", "1")
        res_grad = model(data)
        for k in lib_grad:
            assert th.equal(res_grad[k], lib_grad[k]), k

        def refuse(*a, **kw):
            raise AssertionError("the library convolution ran")
        monkeypatch.setattr(F, "conv2d", refuse)
        monkeypatch.setattr(th.nn.Conv2d, "forward", refuse)
        with th.no_grad():
            res = model(data)
            monkeypatch.setenv("SBMC_CONV5X5_HALF", "0")
            with pytest.raises(AssertionError, match="library convolution"):
                model(data)
    # a `.half()` chain with a half input is not autocast's case (half parameters): the library, as before, to the bit
    monkeypatch.undo()
    th.manual_seed(7)
    net = ops.ConvChain(27, 25, ksize=5, width=100, depth=2, pad=False, weight_norm=False, activation="relu").to(dev).half()
    xh = th.randn(1, 27, 21, 21, device=dev).half()
    with th.no_grad():
        monkeypatch.setenv("SBMC_CONV5X5_HALF", "0")
        lib_half = net(xh)
        monkeypatch.setenv("SBMC_CONV5X5_HALF", "1")
        assert th.equal(net(xh), lib_half)
    # (the chain test's margin: both sides round every layer's result to half, 2^-11 each, before the fp32 splat)
    for k in ("radiance", "diffuse", "specular"):
        no_worse_than(res[k], lib[k], r64[k], rtol=2.0 ** -10, slack=2.0, what=k)
