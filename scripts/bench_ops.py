#!/usr/bin/env python
"""Micro-benchmark of the boundary-level operators and the fused splat update (counterpart of the
reference's scripts/profile/kernel_weighting.py:29-59 and scatter2gather.py:29-57, which only
print a profiler table).  Prints one JSON line per (operator, shape) with the time, the
algorithmic HBM bytes and the fraction of the 8 TB/s roofline.

    python scripts/bench_ops.py [--reps 20]
"""
import argparse
import json
import os
import sys

import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sbmc_amd import functions as F, modules  # noqa: E402

PEAK = 8000.0          # GB/s, HBM3E spec
MFMA_PEAK = 157.3      # TFLOP/s, dense fp32 MFMA


def timeit(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    th.cuda.synchronize()
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="", help="kpcn: only KPCN's 5 x 5 convolutions; kpcn_half: only their half form; "
                                                "kpcn_half_grad: only the half form's gradients")
    args = ap.parse_args()
    dev = th.device("cuda")
    if args.only == "kpcn":
        return kpcn_convs(dev, args.reps)
    if args.only == "kpcn_half":
        return kpcn_half_convs(dev, args.reps)
    if args.only == "kpcn_half_grad":
        return kpcn_half_grad_convs(dev, args.reps)
    shapes = [("profile-script shape (bs4,c3,128x128,k21)", 4, 3, 128, 128, 21),
              ("720p (bs1,c3,1280x720,k21)", 1, 3, 720, 1280, 21)]
    for label, bs, c, h, w, k in shapes:
        px = bs * h * w
        data = th.rand(bs, c, h, w, device=dev)
        wts = th.randn(bs, k, k, h, w, device=dev)
        go = th.randn(bs, c, h, w, device=dev)
        gs = th.randn(bs, h, w, device=dev)
        out, sw = th.empty_like(data), th.empty(bs, h, w, device=dev)
        dd, dw, s2g = th.empty_like(data), th.empty_like(wts), th.empty_like(wts)
        from sbmc_amd import halide_ops as ops
        rows = [
            ("scatter2gather", lambda: ops.scatter2gather_cuda_float32(wts, s2g), 8 * k * k),
            ("kernel_weighting fwd", lambda: ops.kernel_weighting_cuda_float32(data, wts, out, sw),
             4 * k * k + 4 * (2 * c + 1)),
            ("kernel_weighting bwd", lambda: ops.kernel_weighting_grad_cuda_float32(
                data, wts, sw, go, gs, dd, dw), 8 * k * k + 4 * (4 * c + 1)),
        ]
        upd = modules.ProgressiveKernelApply(splat=True)
        kern = wts.view(bs, k * k, h, w)
        st = upd(data, kern, None, None, None)
        st = tuple(t.detach() for t in st)
        rows.append(("fused splat update fwd (with running state)",
                     lambda: upd(data, kern, *st), 4 * k * k + 4 * c + 8 * (c + 2)))
        kg = kern.clone().requires_grad_()
        dg = data.clone().requires_grad_()

        def fused_fb():
            kg.grad = None
            dg.grad = None
            r = upd(dg, kg, *st)
            th.autograd.backward(r, [go, gs.unsqueeze(1), gs.unsqueeze(1)])
        rows.append(("fused splat update fwd+bwd", fused_fb, 12 * k * k + 116))
        gupd = modules.ProgressiveKernelApply(splat=False)
        gst = tuple(t.detach() for t in gupd(data, kern, None, None, None))

        def gather_fb():
            kg.grad = None
            dg.grad = None
            r = gupd(dg, kg, *gst)
            th.autograd.backward(r, [go, gs.unsqueeze(1), gs.unsqueeze(1)])
        rows.append(("fused gather update fwd+bwd (splat=False)", gather_fb, 16 * k * k + 116))
        for name, fn, bpp in rows:
            ms = timeit(fn, args.reps)
            gbps = px * bpp / (ms * 1e-3) / 1e9
            print(json.dumps({"op": name, "shape": label, "ms": round(ms, 4),
                              "alg_bytes": px * bpp, "GBps": round(gbps, 1),
                              "roofline_frac": round(gbps / PEAK, 4)}))
        del data, wts, go, gs, out, sw, dd, dw, s2g, kern, kg, dg, st, gst
        th.cuda.empty_cache()
    cnn_glue(dev, args.reps)
    kpcn_convs(dev, args.reps)
    kpcn_half_convs(dev, args.reps)


def cnn_glue(dev, reps):
    """The kernels around the kernel-predicting CNN at 1280x720, 8 samples: fused 1x1 layers (fp32
    MFMA; flop = 2*cin*cout per output pixel and product), bias/activation passes and the U-net's
    upsample + concat (HBM-bound)."""
    hw, B = 1280 * 720, 8
    label = "720p, 8 samples"

    def emit(name, fn, flop=None, nbytes=None):
        ms = timeit(fn, reps)
        rec = {"op": name, "shape": label, "ms": round(ms, 4)}
        if flop is not None:
            rec.update(TFLOPs=round(flop / (ms * 1e-3) / 1e12, 1),
                       frac_of_fp32_mfma_peak=round(flop / (ms * 1e-3) / 1e12 / MFMA_PEAK, 4))
        if nbytes is not None:
            rec.update(alg_bytes=nbytes, GBps=round(nbytes / (ms * 1e-3) / 1e9, 1),
                       roofline_frac=round(nbytes / (ms * 1e-3) / 1e9 / PEAK, 4))
        print(json.dumps(rec))

    for cin, cout, act in ((128, 128, 1), (128, 441, 0)):
        x = th.randn(B, cin, hw, device=dev, requires_grad=True)
        w = (th.randn(cout, cin, device=dev) / cin ** 0.5).requires_grad_()
        bias = th.randn(cout, device=dev, requires_grad=True)
        emit("pointwise layer %d->%d fwd (GEMM + bias + act)" % (cin, cout),
             lambda: F.PointwiseLayer.apply(x.detach(), w.detach(), bias.detach(), None, 1, act, 0.0),
             flop=2.0 * cin * cout * B * hw, nbytes=4.0 * B * hw * (cin + cout))
        y = F.PointwiseLayer.apply(x, w, bias, None, 1, act, 0.0)
        g = th.randn_like(y)
        emit("pointwise layer %d->%d bwd (gx + gw + gbias)" % (cin, cout),
             lambda: th.autograd.grad(y, [x, w, bias], g, retain_graph=True),
             flop=4.0 * cin * cout * B * hw, nbytes=4.0 * B * hw * (2 * cin + (2 if act else 1) * cout))
        del x, y, g
        th.cuda.empty_cache()
    y0 = th.randn(1, 128, 720, 1280, device=dev)
    bias = th.randn(128, device=dev, requires_grad=True)
    emit("bias_act fwd [1,128,720,1280] (in place)", lambda: F.BiasAct.apply(y0, bias.detach(), 1, 0.0),
         nbytes=8.0 * y0.numel())
    yy = F.BiasAct.apply(y0.clone().requires_grad_() * 1.0, bias, 1, 0.0)
    g = th.randn_like(yy)
    emit("bias_act bwd [1,128,720,1280]", lambda: th.autograd.grad(yy, [bias], g, retain_graph=True),
         nbytes=12.0 * y0.numel())
    coarse = th.randn(1, 256, 360, 640, device=dev, requires_grad=True)
    left = th.randn(1, 128, 720, 1280, device=dev, requires_grad=True)
    emit("upsample x2 + concat fwd (256 + 128 channels at 720p)",
         lambda: F.UpsampleCat.apply(coarse.detach(), left.detach()),
         nbytes=4.0 * (coarse.numel() + 2 * left.numel() + 4 * coarse.numel()))
    out = F.UpsampleCat.apply(coarse, left)
    g = th.randn_like(out)
    emit("upsample x2 + concat bwd (gather adjoint)",
         lambda: th.autograd.grad(out, [coarse], g, retain_graph=True),
         nbytes=4.0 * (4 * coarse.numel() + coarse.numel()))


F16_PEAK = 2500.0      # TFLOP/s, dense f16 MFMA


def kpcn_convs(dev, reps):
    """KPCN's nine 5 x 5 valid convolutions at 1280x720 (27 -> 100 (x 8) -> 441, the frame 4 pixels smaller per layer):
    csrc/conv5x5.hip (bias + ReLU in its epilogue) against the library convolution + bias + ReLU it replaces, ALTERNATING
    in one process -- median and range over the repetitions -- and the whole KPCN(27) forward under no_grad with
    SBMC_CONV5X5 = 0 / 1; per layer also the data and the weight (+ bias) gradient of csrc/conv5x5_grad.hip against
    torch.autograd.grad of F.conv2d, and the whole forward + backward with SBMC_CONV5X5_TRAIN = 0 / 1.  f16 rate: the three f16 products per term the kernel issues on its padded shape (16 on the
    reduction side, 128 on the output side, whole 16 x 16 tiles) against the dense f16 peak."""
    import torch.nn.functional as nnf
    from sbmc_amd import KPCN, _lib
    L = _lib.lib()
    reps = max(3, min(reps, 10))

    def stats(ts):
        ts = sorted(ts)
        return dict(ms=round(ts[len(ts) // 2], 4), ms_min=round(ts[0], 4), ms_max=round(ts[-1], 4))

    def alternate(fns):
        """[name -> fn] timed in turn, `reps` rounds after one warm-up round -> {name: [ms]}"""
        out = {k: [] for k in fns}
        for r in range(reps + 1):
            for k, fn in fns.items():
                a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                th.cuda.synchronize()
                if r:
                    out[k].append(a.elapsed_time(b))
        return out

    H, W = 720, 1280
    stream = _lib.current_stream(dev)
    for i, (cin, cout) in enumerate([(27, 100)] + [(100, 100)] * 7 + [(100, 441)]):
        h, w = H - 4 * i, W - 4 * i
        x = th.randn(1, cin, h, w, device=dev)
        wt = th.randn(cout, cin, 5, 5, device=dev) * (2.0 / (25 * cin)) ** 0.5
        bias = th.randn(cout, device=dev) * 0.1
        ldx, ldy = L.sbmc_conv5x5_padded_channels(cin), L.sbmc_conv5x5_padded_channels(cout)
        xb = th.empty(1, h, w, ldx, device=dev)
        _lib.check(L.sbmc_conv5x5_pack_nchw_f32(_lib.ptr(x), _lib.ptr(xb), ldx, 1, cin, h * w, stream), "pack")
        xmax = F.Conv3x3NHWC._absmax(x)
        wp = th.empty(L.sbmc_conv5x5_weights_bytes(cin, cout), dtype=th.uint8, device=dev)
        s = wt.stride()
        _lib.check(L.sbmc_conv5x5_prepare_weights_f32(_lib.ptr(wt), s[0], s[1], s[2], s[3], wt.numel(), cin, cout,
                                                      _lib.ptr(wp), stream), "prepare")
        yb = th.empty(1, h - 4, w - 4, ldy, device=dev)
        amax = th.zeros(1, dtype=th.int32, device=dev)
        ours = lambda: _lib.check(L.sbmc_conv5x5_bias_act_nhwc_f32(
            _lib.ptr(xb), ldx, _lib.ptr(xmax), _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(yb), ldy, 1, h, w, cin, cout, 0.0,
            _lib.ptr(amax), stream), "conv5x5")
        res = alternate({"conv5x5.hip": ours, "library": lambda: nnf.relu_(nnf.conv2d(x, wt, bias))})
        px = (h - 4) * (w - 4)
        issued = 6.0 * 25 * ldx * (-(-cout // 128) * 128) * (-(-(h - 4) // 16) * 16) * (-(-(w - 4) // 16) * 16)
        for k, ts in res.items():
            rec = {"op": "KPCN layer %d: 5x5 valid %d->%d + bias + ReLU, %s" % (i, cin, cout, k), "shape": "%dx%d" % (w, h)}
            rec.update(stats(ts))
            rec["true_TFLOPs"] = round(2.0 * 25 * cin * cout * px / (rec["ms"] * 1e-3) / 1e12, 1)
            if k == "conv5x5.hip":
                rec["f16_product_TFLOPs"] = round(issued / (rec["ms"] * 1e-3) / 1e12, 1)
                rec["frac_of_f16_peak"] = round(issued / (rec["ms"] * 1e-3) / 1e12 / F16_PEAK, 4)
            print(json.dumps(rec))
        # the gradients (csrc/conv5x5_grad.hip) against the library's: torch.autograd.grad of F.conv2d on the same tensors
        gz = th.randn(1, cout, h - 4, w - 4, device=dev)
        gzb = th.empty(1, h - 4, w - 4, ldy, device=dev)
        _lib.check(L.sbmc_conv5x5_pack_nchw_f32(_lib.ptr(gz), _lib.ptr(gzb), ldy, 1, cout, px, stream), "pack")
        gmax = F.Conv3x3NHWC._absmax(gz)
        wps = th.empty(L.sbmc_conv5x5_weights_bytes(cout, cin), dtype=th.uint8, device=dev)
        _lib.check(L.sbmc_conv5x5_prepare_weights_f32(_lib.ptr(wt), s[1], s[0], s[2], s[3], wt.numel(), cout, cin,
                                                      _lib.ptr(wps), stream), "prepare")
        gxb, gw, gb = th.empty_like(xb), th.empty_like(wt), th.empty_like(bias)
        scratch = th.empty(L.sbmc_conv5x5_wgrad_scratch_bytes(1, h, w, cin, cout), dtype=th.uint8, device=dev)
        xr, wr = x.clone().requires_grad_(), wt.clone().requires_grad_()
        yl = nnf.conv2d(xr, wr)
        res = alternate({
            "dgrad, conv5x5_grad.hip": lambda: _lib.check(L.sbmc_conv5x5_dgrad_adj_nhwc_f32(
                _lib.ptr(gzb), ldy, _lib.ptr(gmax), _lib.ptr(wps), _lib.ptr(xb), 0.0, _lib.ptr(gxb), ldx, 1, h, w, cin, cout,
                _lib.ptr(amax), stream), "dgrad"),
            "dgrad, library": lambda: th.autograd.grad(yl, xr, gz, retain_graph=True),
            "wgrad + bias, conv5x5_grad.hip": lambda: _lib.check(L.sbmc_conv5x5_wgrad_bias_f32(
                _lib.ptr(gzb), ldy, _lib.ptr(gmax), _lib.ptr(xb), ldx, _lib.ptr(xmax), _lib.ptr(gw), s[0], s[1], s[2], s[3],
                _lib.ptr(gb), _lib.ptr(scratch), 1, h, w, cin, cout, stream), "wgrad"),
            "wgrad, library": lambda: th.autograd.grad(yl, wr, gz, retain_graph=True)})
        for k, ts in res.items():
            rec = {"op": "KPCN layer %d: 5x5 valid %d->%d %s" % (i, cin, cout, k), "shape": "%dx%d" % (w, h)}
            rec.update(stats(ts))
            rec["true_TFLOPs"] = round(2.0 * 25 * cin * cout * px / (rec["ms"] * 1e-3) / 1e12, 1)
            print(json.dumps(rec))
        del x, xb, yb, wp, gz, gzb, wps, gxb, scratch, xr, wr, yl
        th.cuda.empty_cache()
    model = KPCN(27).to(dev)
    data = {k: th.randn(1, 27, H, W, device=dev) for k in ("kpcn_diffuse_in", "kpcn_specular_in")}
    data.update({k: th.rand(1, 3, H, W, device=dev) for k in ("kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo")})

    def forward(flag):
        def run():
            os.environ["SBMC_CONV5X5"] = flag
            with th.no_grad():
                model(data)
        return run
    before = os.environ.get("SBMC_CONV5X5")
    res = alternate({"SBMC_CONV5X5=1": forward("1"), "SBMC_CONV5X5=0": forward("0")})
    os.environ.pop("SBMC_CONV5X5")
    if before is not None:
        os.environ["SBMC_CONV5X5"] = before
    for k, ts in res.items():
        rec = {"op": "KPCN(27) forward, no_grad, %s" % k, "shape": "%dx%d" % (W, H)}
        rec.update(stats(ts))
        print(json.dumps(rec))

    def train(flag):
        def run():
            os.environ["SBMC_CONV5X5_TRAIN"] = flag
            model.zero_grad(set_to_none=True)
            model(data)["radiance"].sum().backward()
        return run
    before = os.environ.get("SBMC_CONV5X5_TRAIN")
    res = alternate({"SBMC_CONV5X5_TRAIN=1": train("1"), "SBMC_CONV5X5_TRAIN=0": train("0")})
    os.environ.pop("SBMC_CONV5X5_TRAIN")
    if before is not None:
        os.environ["SBMC_CONV5X5_TRAIN"] = before
    for k, ts in res.items():
        rec = {"op": "KPCN(27) forward + radiance.sum().backward(), %s" % k, "shape": "%dx%d" % (W, H)}
        rec.update(stats(ts))
        print(json.dumps(rec))


def kpcn_half_convs(dev, reps):
    """KPCN's three 5 x 5 layer shapes at 1280x720 on HALF activations: csrc/conv5x5_half.hip (bias + ReLU in its epilogue,
    half in, half out) against F.conv2d + bias + ReLU on half tensors, ALTERNATING in one process; next to each, the fp32
    kernel's figure of profiles/conv5x5_bench_ops.jsonl; and the whole KPCN(27) forward under no_grad +
    torch.autocast(float16) with SBMC_CONV5X5_HALF = 0 / 1.  f16 rate: the one product per term the kernel issues on its
    padded shape (16 on the reduction side, 128 on the output side, whole 32 x 16 tiles) against the dense f16 peak."""
    import torch.nn.functional as nnf
    from sbmc_amd import KPCN, _lib
    L = _lib.lib()
    reps = max(3, min(reps, 10))

    WARM, PER = 3, 5

    def timed(fns, per=PER):
        """[name -> fn] in turn: WARM warm-up rounds, then `reps` samples of `per` launches between two events each"""
        out = {k: [] for k in fns}
        for r in range(reps + WARM):
            for k, fn in fns.items():
                a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per):
                    fn()
                b.record()
                th.cuda.synchronize()
                if r >= WARM:
                    out[k].append(a.elapsed_time(b) / per)
        return {k: dict(ms=round(sorted(ts)[len(ts) // 2], 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
                for k, ts in out.items()}

    fp32 = {}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv5x5_bench_ops.jsonl")
    if os.path.exists(path):
        for line in open(path):
            rec = json.loads(line)
            if rec["op"].endswith("ReLU, conv5x5.hip"):
                fp32[rec["op"].split(":")[0]] = rec["ms"]
    H, W = 720, 1280
    stream = _lib.current_stream(dev)
    for i, cin, cout in ((0, 27, 100), (1, 100, 100), (8, 100, 441)):
        h, w = H - 4 * i, W - 4 * i
        x = th.randn(1, cin, h, w, device=dev).half()
        wt = th.randn(cout, cin, 5, 5, device=dev) * (2.0 / (25 * cin)) ** 0.5
        bias = th.randn(cout, device=dev) * 0.1
        wh, bh = wt.half(), bias.half()
        ldx, ldy = L.sbmc_conv5x5_padded_channels(cin), L.sbmc_conv5x5_padded_channels(cout)
        xb = th.empty(1, h, w, ldx, dtype=th.float16, device=dev)
        _lib.check(L.sbmc_conv5x5_half_pack_nchw_f16(_lib.ptr(x), _lib.ptr(xb), ldx, 1, cin, h * w, stream), "pack")
        wp = th.empty(L.sbmc_conv5x5_half_weights_bytes(cin, cout), dtype=th.uint8, device=dev)
        s = wt.stride()
        _lib.check(L.sbmc_conv5x5_half_prepare_weights(_lib.ptr(wt), s[0], s[1], s[2], s[3], cin, cout, _lib.ptr(wp), stream),
                   "prepare")
        yb = th.empty(1, h - 4, w - 4, ldy, dtype=th.float16, device=dev)
        ours = lambda: _lib.check(L.sbmc_conv5x5_half_bias_act_nhwc(
            _lib.ptr(xb), ldx, _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(yb), ldy, 1, h, w, cin, cout, 0.0, stream), "conv5x5_half")
        res = timed({"conv5x5_half.hip": ours, "library (half)": lambda: nnf.relu_(nnf.conv2d(x, wh, bh))})
        px = (h - 4) * (w - 4)
        issued = 2.0 * 25 * ldx * (-(-cout // 128) * 128) * (-(-(h - 4) // 32) * 32) * (-(-(w - 4) // 16) * 16)
        for k, st in res.items():
            rec = {"op": "KPCN layer %d: 5x5 valid %d->%d + bias + ReLU, %s" % (i, cin, cout, k), "shape": "%dx%d" % (w, h)}
            rec.update(st)
            rec["true_TFLOPs"] = round(2.0 * 25 * cin * cout * px / (rec["ms"] * 1e-3) / 1e12, 1)
            if k == "conv5x5_half.hip":
                rec["f16_product_TFLOPs"] = round(issued / (rec["ms"] * 1e-3) / 1e12, 1)
                rec["frac_of_f16_peak"] = round(issued / (rec["ms"] * 1e-3) / 1e12 / F16_PEAK, 4)
                if "KPCN layer %d" % i in fp32:
                    rec["fp32_kernel_ms_recorded"] = fp32["KPCN layer %d" % i]
            print(json.dumps(rec))
        del x, xb, yb, wp
        th.cuda.empty_cache()
    model = KPCN(27).to(dev)
    data = {k: th.randn(1, 27, H, W, device=dev) for k in ("kpcn_diffuse_in", "kpcn_specular_in")}
    data.update({k: th.rand(1, 3, H, W, device=dev) for k in ("kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo")})

    def forward(flag):
        def run():
            os.environ["SBMC_CONV5X5_HALF"] = flag
            with th.no_grad(), th.autocast("cuda", dtype=th.float16):
                model(data)
        return run
    before = os.environ.get("SBMC_CONV5X5_HALF")
    res = timed({"SBMC_CONV5X5_HALF=1": forward("1"), "SBMC_CONV5X5_HALF=0": forward("0")}, per=1)
    os.environ.pop("SBMC_CONV5X5_HALF")
    if before is not None:
        os.environ["SBMC_CONV5X5_HALF"] = before
    for k, st in res.items():
        rec = {"op": "KPCN(27) forward, no_grad, autocast(float16), %s" % k, "shape": "%dx%d" % (W, H)}
        rec.update(st)
        print(json.dumps(rec))


def kpcn_half_grad_convs(dev, reps):
    """The gradients of KPCN's three 5 x 5 layer shapes at 1280x720 on HALF activations: the data gradient and the weight +
    bias gradient of csrc/conv5x5_half_grad.hip against torch.autograd.grad of F.conv2d on half tensors (the library's half
    backward: what SBMC_CONV5X5_TRAIN = 0 runs under autocast), ALTERNATING in one process; next to each, the fp32
    kernel's figure of profiles/conv5x5_grad_bench_ops.jsonl; and the whole KPCN(27) forward + backward under
    torch.autocast(float16) with SBMC_CONV5X5_TRAIN = 0 / 1.  f16 rate: the one product per term the kernels issue on their
    padded shapes (dgrad: 16 gz channels, 128 x channels, whole 32 x 16 tiles; wgrad: 128 x 64 channel tiles, 25 taps, 32-pixel
    row stages) against the dense f16 peak."""
    import torch.nn.functional as nnf
    from sbmc_amd import KPCN, _lib
    L = _lib.lib()
    reps = max(3, min(reps, 10))
    WARM = 2

    def timed(fns):
        """[name -> fn] in turn: WARM warm-up rounds, then `reps` samples of one launch between two events each"""
        out = {k: [] for k in fns}
        for r in range(reps + WARM):
            for k, fn in fns.items():
                a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                th.cuda.synchronize()
                if r >= WARM:
                    out[k].append(a.elapsed_time(b))
        return {k: dict(ms=round(sorted(ts)[len(ts) // 2], 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
                for k, ts in out.items()}

    fp32 = {}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv5x5_grad_bench_ops.jsonl")
    if os.path.exists(path):
        for line in open(path):
            rec = json.loads(line)
            if rec["op"].endswith("conv5x5_grad.hip"):
                fp32[rec["op"].replace("conv5x5_grad.hip", "conv5x5_half_grad.hip")] = rec["ms"]
    H, W = 720, 1280
    stream = _lib.current_stream(dev)
    for i, cin, cout in ((0, 27, 100), (1, 100, 100), (8, 100, 441)):
        h, w = H - 4 * i, W - 4 * i
        px = (h - 4) * (w - 4)
        x = th.randn(1, cin, h, w, device=dev).half()
        wt = th.randn(cout, cin, 5, 5, device=dev) * (2.0 / (25 * cin)) ** 0.5
        gz = th.randn(1, cout, h - 4, w - 4, device=dev).half()
        ldx, ldg = L.sbmc_conv5x5_padded_channels(cin), L.sbmc_conv5x5_padded_channels(cout)
        xb = th.empty(1, h, w, ldx, dtype=th.float16, device=dev)
        gzb = th.empty(1, h - 4, w - 4, ldg, dtype=th.float16, device=dev)
        _lib.check(L.sbmc_conv5x5_half_pack_nchw_f16(_lib.ptr(x), _lib.ptr(xb), ldx, 1, cin, h * w, stream), "pack")
        _lib.check(L.sbmc_conv5x5_half_pack_nchw_f16(_lib.ptr(gz), _lib.ptr(gzb), ldg, 1, cout, px, stream), "pack")
        s = wt.stride()
        wps = th.empty(L.sbmc_conv5x5_half_weights_bytes(cout, cin), dtype=th.uint8, device=dev)
        _lib.check(L.sbmc_conv5x5_half_prepare_weights(_lib.ptr(wt), s[1], s[0], s[2], s[3], cout, cin, _lib.ptr(wps), stream),
                   "prepare")
        gxb, gw, gb = th.empty_like(xb), th.empty_like(wt), th.empty(cout, device=dev)
        scratch = th.empty(L.sbmc_conv5x5_half_wgrad_scratch_bytes(1, h, w, cin, cout), dtype=th.uint8, device=dev)
        xr, wr = x.clone().requires_grad_(), wt.half().requires_grad_()
        yl = nnf.conv2d(xr, wr)
        res = timed({
            "dgrad, conv5x5_half_grad.hip": lambda: _lib.check(L.sbmc_conv5x5_half_dgrad_adj_nhwc(
                _lib.ptr(gzb), ldg, _lib.ptr(wps), _lib.ptr(xb), 0.0, _lib.ptr(gxb), ldx, 1, h, w, cin, cout, stream), "dgrad"),
            "dgrad, library (half)": lambda: th.autograd.grad(yl, xr, gz, retain_graph=True),
            "wgrad + bias, conv5x5_half_grad.hip": lambda: _lib.check(L.sbmc_conv5x5_half_wgrad_bias(
                _lib.ptr(gzb), ldg, _lib.ptr(xb), ldx, _lib.ptr(gw), s[0], s[1], s[2], s[3], _lib.ptr(gb), _lib.ptr(scratch),
                1, h, w, cin, cout, stream), "wgrad"),
            "wgrad, library (half)": lambda: th.autograd.grad(yl, wr, gz, retain_graph=True)})
        issued = {
            "dgrad": 2.0 * 25 * ldg * (-(-cin // 128) * 128) * (-(-h // 32) * 32) * (-(-w // 16) * 16),
            "wgrad": 2.0 * 25 * (-(-cout // 128) * 128) * (-(-cin // 64) * 64) * (h - 4) * (-(-(w - 4) // 32) * 32)}
        for k, st in res.items():
            rec = {"op": "KPCN layer %d: 5x5 valid %d->%d %s" % (i, cin, cout, k), "shape": "%dx%d" % (w, h)}
            rec.update(st)
            rec["true_TFLOPs"] = round(2.0 * 25 * cin * cout * px / (rec["ms"] * 1e-3) / 1e12, 1)
            if k.endswith("conv5x5_half_grad.hip"):
                n = issued[k[:5]]
                rec["f16_product_TFLOPs"] = round(n / (rec["ms"] * 1e-3) / 1e12, 1)
                rec["frac_of_f16_peak"] = round(n / (rec["ms"] * 1e-3) / 1e12 / F16_PEAK, 4)
                rec["ratio_to_library"] = round(res[k[:5] + ", library (half)"]["ms"] / rec["ms"], 2)
                if rec["op"] in fp32:
                    rec["fp32_kernel_ms_recorded"] = fp32[rec["op"]]
            print(json.dumps(rec), flush=True)
        del x, xb, gz, gzb, wps, gxb, scratch, xr, wr, yl
        th.cuda.empty_cache()
    model = KPCN(27).to(dev)
    data = {k: th.randn(1, 27, H, W, device=dev) for k in ("kpcn_diffuse_in", "kpcn_specular_in")}
    data.update({k: th.rand(1, 3, H, W, device=dev) for k in ("kpcn_diffuse_buffer", "kpcn_specular_buffer", "kpcn_albedo")})

    def train(flag):
        def run():
            os.environ["SBMC_CONV5X5_TRAIN"] = flag
            model.zero_grad(set_to_none=True)
            with th.autocast("cuda", dtype=th.float16):
                out = model(data)["radiance"]
            out.float().sum().backward()
        return run
    before = os.environ.get("SBMC_CONV5X5_TRAIN")
    res = timed({"SBMC_CONV5X5_TRAIN=1": train("1"), "SBMC_CONV5X5_TRAIN=0": train("0")})
    os.environ.pop("SBMC_CONV5X5_TRAIN")
    if before is not None:
        os.environ["SBMC_CONV5X5_TRAIN"] = before
    for k, st in res.items():
        rec = {"op": "KPCN(27) forward + radiance.sum().backward(), autocast(float16), %s" % k, "shape": "%dx%d" % (W, H)}
        rec.update(st)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
