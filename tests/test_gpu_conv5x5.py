"""The split-precision 5 x 5 valid convolution (csrc/conv5x5.hip) behind KPCN's chains at inference, against torch's
float64 convolution on the CPU.  The fp32 library convolution (MIOpen) is the yardstick, as in test_gpu_conv3x3.py: ours
must be no further from float64 than twice its error."""
import ctypes

import pytest
import torch as th
import torch.nn.functional as F

from helpers import KernelApplyFP64, float64_twin, no_worse_than
from sbmc_amd import KPCN, _lib
from sbmc_amd import functions as funcs
from sbmc_amd import modules as ops

pytestmark = pytest.mark.gpu


def _dev():
    if not th.cuda.is_available():
        pytest.skip("needs a GPU")
    return th.device("cuda")


def _err(a, ref):
    return (a.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def _single_layer(b, cin, cout, h, w, xs=1.0, ws=0.05):
    """One layer, linear and with ReLU, against float64; the bound of tests/test_gpu_conv3x3.py."""
    dev = _dev()
    g = th.Generator(device="cpu").manual_seed(b * 1000 + cin + cout + h * w)
    x = th.randn(b, cin, h, w, generator=g) * xs
    wt = th.randn(cout, cin, 5, 5, generator=g) * ws
    bias = th.randn(cout, generator=g) * (xs * ws * (25 * cin) ** 0.5)         # (of the size of the sums it joins)
    ref = F.conv2d(x.double(), wt.double(), bias.double())
    xg, wg, bg = x.to(dev), wt.to(dev), bias.to(dev)
    lib = F.conv2d(xg, wg, bg)
    for act, fn in ((0, lambda v: v), (1, th.relu)):
        y = funcs.conv5x5_chain(xg, [(wg, bg, act, 0.0)])
        assert y.shape == (b, cout, h - 4, w - 4) and y.is_contiguous()
        e, yard = _err(y, fn(ref)), _err(fn(lib), fn(ref))
        print("conv5x5 %s act %d: %.3e of the largest value (fp32 library: %.3e)" % ((b, cin, cout, h, w), act, e, yard))
        assert e <= max(2.0 * yard, 2e-7), "act %d: %.3e of the largest value (fp32 library: %.3e)" % (act, e, yard)


@pytest.mark.parametrize("b,cin,cout,h,w", [
    (1, 27, 100, 20, 20),         # exactly one 16 x 16 tile; a partial reduction granule; padded output channels
    (2, 100, 100, 21, 37),        # ragged tiles in both directions, several tiles, batch, seven reduction chunks
    (1, 100, 441, 24, 20),        # four output-channel tiles, the last one ragged
    (1, 6, 8, 9, 9),              # an output smaller than a tile; the fixtures' channel counts
    (1, 100, 25, 5, 5),           # a single output pixel
])
def test_single_layer_matches_float64(b, cin, cout, h, w):
    _single_layer(b, cin, cout, h, w)


@pytest.mark.parametrize("xs,ws", [(1e-9, 1.0), (3e4, 1e-6), (1.0, 1e3)])
def test_scales_follow_the_tensors(xs, ws):
    _single_layer(2, 100, 100, 21, 37, xs, ws)


def test_chain_hands_magnitudes_and_zero_padding_on(monkeypatch):
    dev = _dev()
    th.manual_seed(11)
    make = lambda: ops.ConvChain(27, 441, ksize=5, width=100, depth=3, pad=False, weight_norm=False, activation="relu")
    net = make().to(dev)
    for p in net.parameters():
        if p.dim() == 1:
            p.data.normal_(0.0, 0.1)
    x = th.randn(1, 27, 29, 33, device=dev)
    with th.no_grad():
        truth = float64_twin(net, make)(x.cpu().double())
        monkeypatch.setenv("SBMC_CONV5X5", "0")
        ref32 = net(x)
        monkeypatch.setenv("SBMC_CONV5X5", "1")
        y = net(x)
    assert y.shape == (1, 441, 17, 21) and y.is_contiguous()
    no_worse_than(y, ref32, truth, rtol=1e-5, slack=2.0, what="chain")


@pytest.mark.parametrize("grad", [False, True])
def test_kpcn_dispatch(monkeypatch, grad):
    """Inference runs on the kernel (the library convolution raises); with gradients wanted nothing changes, to the bit."""
    dev = _dev()
    th.manual_seed(4)
    model = KPCN(27, ksize=5).to(dev)
    for name, p in model.named_parameters():
        if name.endswith("bias"):
            p.data.normal_(0.0, 0.1)
    data = {k: th.randn(1, 27, 53, 53, device=dev) for k in ("kpcn_diffuse_in", "kpcn_specular_in")}
    data.update({k: th.rand(1, 3, 53, 53, device=dev) for k in ("kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo")})
    with th.set_grad_enabled(grad):
        monkeypatch.setenv("SBMC_CONV5X5", "0")
        ref32 = model(data)
        monkeypatch.setenv("SBMC_CONV5X5", "1")
        if grad:
            res = model(data)
            for k in ref32:
                assert th.equal(res[k], ref32[k]), k
            res["radiance"].sum().backward()
            assert all(p.grad is not None for p in model.parameters())
            return
        m64 = float64_twin(model, lambda: KPCN(27, ksize=5))
        m64.kernel_apply = KernelApplyFP64()
        r64 = m64({k: v.cpu().double() for k, v in data.items()})

        def refuse(*a, **kw):
            raise AssertionError("the library convolution ran")
        monkeypatch.setattr(F, "conv2d", refuse)
        monkeypatch.setattr(th.nn.Conv2d, "forward", refuse)
        res = model(data)
    for k in ("radiance", "diffuse", "specular"):
        no_worse_than(res[k], ref32[k], r64[k], what=k)


def test_abi_rejects_what_the_kernel_does_not_take():
    dev = _dev()
    L = _lib.lib()
    assert L.sbmc_conv5x5_supported(1, 5, 5, 1, 1) == 1 and L.sbmc_conv5x5_supported(2, 720, 1280, 100, 441) == 1
    assert L.sbmc_conv5x5_supported(1, 4, 9, 27, 100) == 0 and L.sbmc_conv5x5_supported(1, 9, 4, 27, 100) == 0
    assert L.sbmc_conv5x5_supported(1, 8, 2000000, 441, 441) == 0       # a patch row beyond 31 bits of byte offset
    assert L.sbmc_conv5x5_supported(1, 9, 9, 0, 8) == 0 and L.sbmc_conv5x5_weights_bytes(0, 8) == 0
    assert [L.sbmc_conv5x5_padded_channels(c) for c in (0, 1, 27, 100, 441)] == [0, 16, 32, 112, 448]
    x = th.zeros(1, 9, 9, 32, device=dev)
    y = th.zeros(1, 5, 5, 16, device=dev)
    bias, xmax = th.zeros(8, device=dev), th.zeros(1, dtype=th.int32, device=dev)
    wt = th.randn(8, 27, 5, 5, device=dev)
    wp = th.zeros(L.sbmc_conv5x5_weights_bytes(27, 8), dtype=th.uint8, device=dev)
    p = lambda t_, off=0: ctypes.c_void_p(t_.data_ptr() + off)
    assert L.sbmc_conv5x5_prepare_weights_f32(p(wt), 675, 25, 5, 1, wt.numel(), 27, 8, p(wp), None) == 0

    def launch(xp=p(x), wpp=p(wp), yp=p(y), h=9, w=9, ldx=32, ldy=16):
        return L.sbmc_conv5x5_bias_act_nhwc_f32(xp, ldx, p(xmax), wpp, p(bias), yp, ldy, 1, h, w, 27, 8, 0.0, None, None)
    for bad in (dict(h=4), dict(w=4), dict(xp=p(x, 4)), dict(wpp=p(wp, 8)), dict(yp=p(y, 4)), dict(xp=None),
                dict(ldx=16), dict(ldy=24), dict(w=2000000)):
        assert launch(**bad) == -1, bad
    assert launch() == 0                                               # (the same call with nothing wrong: zeros in, zeros out)
    assert y.abs().max().item() == 0.0
