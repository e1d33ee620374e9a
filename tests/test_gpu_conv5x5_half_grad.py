"""The gradients of the half 5 x 5 valid convolution (csrc/conv5x5_half_grad.hip) behind KPCN's chains in training under
torch.autocast(float16): a layer against float64 autograd of the SAME half-rounded operands, a chain against its layers
stacked by autograd, and the model's dispatch."""
import pytest
import torch as th
import torch.nn.functional as F

from helpers import close_sum
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
    """tests/test_gpu_conv5x5_half.py's contract: one half rounding of ref + 1e-5 of the tensor's scale"""
    a, ref = a.detach().cpu().double(), ref.double()
    err = (a - ref).abs()
    print("%s: worst %.3e of scale" % (what, (err.max() / ref.abs().max()).item()))
    bad = err > HALF_ULP * 1.01 * ref.abs() + 1e-5 * ref.abs().max()
    assert not bad.any(), "%s: %d / %d beyond one half rounding, worst %.3e of scale" % (
        what, int(bad.sum()), ref.numel(), (err.max() / ref.abs().max()).item())


def _grads64(x, wt, bias, cot, mask=None):
    """float64 (gx, gw, gb) of the convolution for the cotangent `cot`; mask: act' of the layer below, applied to gx"""
    leaves = [t.double().requires_grad_() for t in (x, wt, bias)]
    gx, gw, gb = th.autograd.grad(F.conv2d(*leaves), leaves, cot.double())
    return (gx if mask is None else gx * mask), gw, gb


@pytest.mark.parametrize("b,cin,cout,h,w,relu_below", [
    (1, 27, 100, 36, 20, False),     # one dgrad tile, partial granules on both sides
    (2, 100, 100, 37, 21, False),    # ragged tiles, batch
    (2, 100, 100, 37, 21, True),     # ... with ReLU below the layer: the adjoint from a given saved activation
    (1, 100, 441, 24, 20, False),    # 28 reduction granules for dgrad; four output-channel tiles for wgrad, the last ragged
    (1, 6, 8, 9, 9, False),          # a gz smaller than a tile
    (1, 100, 25, 5, 5, False),       # one gz pixel: every dgrad output is a border pixel
    (1, 16, 16, 40, 150, False),     # more row stages than one wgrad range holds
])
def test_single_layer_gradients_match_float64(b, cin, cout, h, w, relu_below):
    dev = _dev()
    L = _lib.lib()
    if (cin, cout) == (16, 16):
        one_range = (5 * 5 * 128 * 64 + 128) * 4         # a tile of partial sums per tap column + the bias sums
        assert L.sbmc_conv5x5_half_wgrad_scratch_bytes(b, h, w, cin, cout) > one_range
    gen = th.Generator(device="cpu").manual_seed(b * 1000 + cin + cout + h * w)
    x = th.randn(b, cin, h, w, generator=gen).half()
    if relu_below:
        x = th.relu(x)                                   # the saved activation of a ReLU layer: act' = x > 0, exactly
    wt = th.randn(cout, cin, 5, 5, generator=gen) * (2.0 / (25 * cin)) ** 0.5
    bias = th.randn(cout, generator=gen) * 0.5
    cot = th.randn(b, cout, h - 4, w - 4, generator=gen).half()
    what = "%s relu_below=%s" % ((b, cin, cout, h, w), relu_below)
    mask = (x > 0).double() if relu_below else None
    gx64, gw64, gb64 = _grads64(x, wt.half(), bias, cot, mask)
    _, gwabs, gbabs = _grads64(x.abs(), wt.half(), bias, cot.abs())
    if relu_below:
        # through the raw entry points: the layer's saved half input is the activation whose adjoint the epilogue applies
        p = _lib.ptr
        ldx, ldg = L.sbmc_conv5x5_padded_channels(cin), L.sbmc_conv5x5_padded_channels(cout)
        xb = th.empty(b, h, w, ldx, dtype=th.float16, device=dev)
        gz = th.empty(b, h - 4, w - 4, ldg, dtype=th.float16, device=dev)
        gxb = th.full((b, h, w, ldx), 7.0, dtype=th.float16, device=dev)
        xd, cd, wd = x.to(dev), cot.to(dev), wt.to(dev)
        wp = th.empty(L.sbmc_conv5x5_half_weights_bytes(cout, cin), dtype=th.uint8, device=dev)
        gw, gb = th.empty(cout, cin, 5, 5, device=dev), th.empty(cout, device=dev)
        scratch = th.empty(L.sbmc_conv5x5_half_wgrad_scratch_bytes(b, h, w, cin, cout), dtype=th.uint8, device=dev)
        assert L.sbmc_conv5x5_half_pack_nchw_f16(p(xd), p(xb), ldx, b, cin, h * w, None) == 0
        assert L.sbmc_conv5x5_half_pack_nchw_f16(p(cd), p(gz), ldg, b, cout, (h - 4) * (w - 4), None) == 0
        assert L.sbmc_conv5x5_half_prepare_weights(p(wd), 25, cin * 25, 5, 1, cout, cin, p(wp), None) == 0
        assert L.sbmc_conv5x5_half_dgrad_adj_nhwc(p(gz), ldg, p(wp), p(xb), 0.0, p(gxb), ldx, b, h, w, cin, cout, None) == 0
        assert L.sbmc_conv5x5_half_wgrad_bias(p(gz), ldg, p(xb), ldx, p(gw), *gw.stride(), p(gb), p(scratch), b, h, w, cin, cout,
                                              None) == 0
        th.cuda.synchronize()
        assert (gxb[..., cin:] == 0).all()               # the padding channels are written, as zeros
        gx = gxb[..., :cin].permute(0, 3, 1, 2)
    else:
        leaves = [t.to(dev).requires_grad_() for t in (x, wt, bias)]
        y = funcs.Conv5x5ChainTrainHalf.apply(leaves[0], ((0, 0.0),), leaves[1], leaves[2])
        gx, gw, gb = th.autograd.grad(y, leaves, cot.to(dev))
        assert gx.dtype == th.float16 and gw.dtype == th.float32 and gb.dtype == th.float32
    _check_half(gx, gx64, "gx " + what)
    close_sum(gw, gw64, gwabs, rtol=1e-5, what="gw " + what)
    close_sum(gb, gb64, gbabs, rtol=1e-5, what="gb " + what)


@pytest.mark.parametrize("act,slope", [(1, 0.0), (2, 0.1)])
def test_chain_equals_its_layers_stacked_by_autograd(monkeypatch, act, slope):
    """27 -> 100 -> 100 -> 441 on 1 x 27 x 17 x 21.  ReLU: bit for bit (both apply g {0, 1} before one half rounding);
    LeakyReLU: within one half rounding + 1e-5 of scale.  (Two half values that differ at all differ by a whole ulp, up to
    2^-10 of the value: that bound asks for all but equal results, and the data-gradient epilogue gives them -- it rounds
    the sum to half before the slope, as the layered form does.)"""
    dev = _dev()
    gen = th.Generator(device="cpu").manual_seed(7 + act)
    chans = [27, 100, 100, 441]
    x = th.randn(1, 27, 17, 21, generator=gen).to(dev)
    params = []
    for cin, cout in zip(chans[:-1], chans[1:]):
        params += [(th.randn(cout, cin, 5, 5, generator=gen) * (2.0 / (25 * cin)) ** 0.5).to(dev).requires_grad_(),
                   (th.randn(cout, generator=gen) * 0.1).to(dev).requires_grad_()]
    cot = th.randn(1, 441, 5, 9, generator=gen).half().to(dev)
    acts = ((act, slope),) * 3

    xg = x.clone().requires_grad_()
    y = funcs.Conv5x5ChainTrainHalf.apply(xg, acts, *params)
    chain = th.autograd.grad(y, [xg] + params, cot)
    with th.no_grad():
        infer = funcs.conv5x5_chain_half(x, [(params[2 * i], params[2 * i + 1], act, slope) for i in range(3)])
    assert y.dtype == th.float16 and th.equal(y, infer)
    assert chain[0].dtype == th.float32                    # gx has x's dtype

    xl = x.clone().requires_grad_()
    z = xl
    for i in range(3):
        z = funcs.Conv5x5ChainTrainHalf.apply(z, acts[i:i + 1], params[2 * i], params[2 * i + 1])
    assert th.equal(z, y)
    layered = th.autograd.grad(z, [xl] + params, cot)
    for k, (a, r) in enumerate(zip(chain, layered)):
        if act == 1:
            assert th.equal(a, r), k
        else:
            _check_half(a, r.cpu(), "leaky %d" % k)

    # nothing wanted from x: the first layer's data gradient does not run
    y = funcs.Conv5x5ChainTrainHalf.apply(x, acts, *params)
    calls = []
    real = _lib.lib().sbmc_conv5x5_half_dgrad_adj_nhwc
    monkeypatch.setattr(_lib.lib(), "sbmc_conv5x5_half_dgrad_adj_nhwc", lambda *a: calls.append(a[8]) or real(*a))
    y.backward(cot)
    monkeypatch.undo()
    assert calls == [9, 13] and x.grad is None            # (the input heights of layers 2 and 1)
    for k, q in enumerate(params):
        assert th.equal(q.grad, chain[1 + k]), k


def _refuse(*a, **kw):
    raise AssertionError("the library convolution ran")


def test_kpcn_trains_under_autocast_without_the_library(monkeypatch):
    dev = _dev()
    th.manual_seed(4)
    model = KPCN(27, ksize=5).to(dev)
    for name, q in model.named_parameters():
        if name.endswith("bias"):
            q.data.normal_(0.0, 0.1)
    data = {k: th.randn(1, 27, 53, 53, device=dev) for k in ("kpcn_diffuse_in", "kpcn_specular_in")}
    data.update({k: th.rand(1, 3, 53, 53, device=dev) for k in ("kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo")})
    monkeypatch.setenv("SBMC_CONV5X5_TRAIN", "1")
    monkeypatch.setattr(F, "conv2d", _refuse)
    monkeypatch.setattr(th.nn.Conv2d, "forward", _refuse)
    with th.autocast("cuda", dtype=th.float16):
        with th.no_grad():
            infer = model(data)
        res = model(data)
        for k in infer:
            assert th.equal(res[k], infer[k]), k
    res["radiance"].float().sum().backward()
    for name, q in model.named_parameters():
        assert q.grad is not None and q.grad.dtype == th.float32, name
        assert th.isfinite(q.grad).all() and q.grad.abs().max().item() > 0, name
    with th.autocast("cuda", dtype=th.bfloat16):
        with pytest.raises(AssertionError, match="library convolution"):
            model(data)
