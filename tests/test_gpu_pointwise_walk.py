"""The persistent 1 x 1 kernels' MULTI-TILE walks against float64 (csrc/pointwise.hip, pointwise_chain.hip, pointwise_chain_bwd.hip).

Every per-sample 1 x 1 kernel launches about one workgroup per CU and walks 64-pixel tiles at a grid stride.  What is delicate in
them exists from a workgroup's SECOND tile on: LDS-DMA requests for the tile after next waited for with hand-counted
`s_waitcnt vmcnt(N)`, the double-buffered per-pixel maxima, the running sample mean and magnitude words, the weight / bias / context
partial sums a workgroup keeps in registers across its tiles.  The other float64 tests' shapes give a 256-CU part one tile per
workgroup; the shapes here follow the device's CU count (walk_shape) so that every workgroup walks first, steady, steady and last
tiles, workgroups end at different iterations, and ragged edge tiles fall in the middle of walks -- at tens of MB per tensor.

Every test asserts that precondition (_check_walk) on the device it runs on, against the grid the C ABI reports where it
reports one.  Bounds: the project's 1e-5 of each tensor's scale against float64; words and sign bits exact; the half kernels at
the bounds of tests/test_gpu_ops.py (test_pointwise_half_training)."""
import pytest
import torch as th

from test_gpu_pointwise_chain import _chain64, _make, _pack_signs, _pair_gz64, _sign_bits
from test_gpu_pointwise_scaled import _backward64, _layer64, _word

pytestmark = pytest.mark.gpu

PLANES = 16          # image groups of a launch: 16 ragged edge tiles spread over a walk of 4.5 rounds
SLOPE = 0.01


def _cus():
    """the attribute the launch code reads (hipDeviceAttributeMultiprocessorCount)"""
    return th.cuda.get_device_properties(0).multi_processor_count


# The grids, from the launch code (units: a pixel tile of one image group -- its S samples are walked one after the other
# where something per-pixel is shared between them):
#   min(units, CUs)                     the chains (sbmc_pointwise_chain_fwd_f32), the wide forward (sbmc_pointwise_wide_fwd_f32),
#                                       pw_bwd_grid (every sbmc_pointwise_bwd_*, sbmc_pointwise_gw_wide_*, sbmc_pointwise_wide_bwd_f32),
#                                       the pair backward (sbmc_pointwise_chain_bwd_groups)
#   CUs / (8 nrt) * (8 nrt)             the split forward (pw_fwd_launch, fp32 in): nrt = ceil(cout / 128) workgroups share a
#     against ceil(units / 8) * 8 nrt   unit, so grid / nrt workgroups WALK
#   2 CUs / (8 nrt) * (8 nrt), same cap the all-half forward, on tiles of 128 pixels
def grid_persistent(units):
    return min(units, _cus())


def walkers_split_forward(units, cout, per_cu=1):
    nrt = (cout + 127) // 128
    unit = 8 * nrt
    grid = per_cu * _cus() // unit * unit
    grid = max(min(grid, (units + 7) // 8 * unit), unit)
    return grid // nrt


def walk_shape(walkers, tile=64, planes=PLANES, rounds=4.5):
    """-> (planes, hw): planes x ceil(hw / tile) units are at least `rounds` x `walkers` (the number of workgroups that walk,
    at the size of grid the shape itself produces) and no multiple of it; hw % tile == 20: every plane ends in a ragged tile.
    (tools/fuzz_pointwise_chain.py --walk draws its shapes here too.)"""
    assert walkers > 1, "one workgroup walks everything: no remainder to leave"
    if planes % walkers == 0:
        planes += 1                                     # (a handful of CUs: every multiple of `planes` is one of the grid)
    tpp = -int(-rounds * walkers // planes)
    while (planes * tpp) % walkers == 0:
        tpp += 1
    return planes, tile * (tpp - 1) + 20


def _check_walk(units, walkers, tpp, what, interleave=1):
    """The precondition of every test here: each workgroup walks at least 4 units, some walk one more (they end at different
    iterations), and the plane's ragged last tile is met in the middle of some walk (neither a first nor a last tile).
    interleave: the tiles of that many images alternate in the walk's order (units = tiles)."""
    lo = units // walkers
    assert 2 * units >= 9 * walkers and units % walkers != 0 and lo >= 4, \
        "%s: %d units over %d workgroups is no multi-tile walk on this device (%d CUs)" % (what, units, walkers, _cus())
    edges = [(interleave * (j * tpp + tpp - 1) + k) // walkers for j in range(units // tpp // interleave) for k in range(interleave)]
    assert any(1 <= e < lo - 1 for e in edges), "%s: no ragged tile in mid-walk (%s)" % (what, edges)
    print("%s: %d units over %d workgroups: %d-%d per workgroup" % (what, units, walkers, lo, lo + 1))


def _rel(a, ref, what):
    """max |a - ref| / max |ref| against float64, printed before it is held to a bound"""
    assert a.shape == ref.shape, (what, tuple(a.shape), tuple(ref.shape))
    assert th.isfinite(a).all(), what + ": not every element was written"
    e = (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)
    print("  %s: %.3e of scale" % (what, e))
    return e


def _nan(*shape, **kw):
    return th.full(shape, float("nan"), device="cuda", **kw)


# ---------------------------------------------------------------------------------------------
# the chain forward: the six launch forms by what is stored behind the next tile's requests (wait_rows() in
# csrc/pointwise_chain.hip: nyounger = 16 if layer 1 is stored + 1 with its sign words + 16 with three layers -- the last
# layer of a two-layer chain IS layer 1, so its inference form waits with vmcnt(16) as the three-layer one does)
CHAIN_CASES = [
    # s, cin, couts, t_mode, acts, mean, store_mid, signs, spread
    (1, 128, (128, 128), 0, (2, 2), False, False, False, 1.0),           # NL = 2 inference
    (2, 64, (128, 128), 1, (1, 0), True, False, False, 1e-4),            #   KP 64, per-image context, mean
    (2, 128, (128, 128, 128), 2, (1, 1, 0), True, False, False, 1.0),    # NL = 3 inference: vmcnt(16)
    (2, 93, (128, 128, 128), 1, (1, 1, 0), False, False, False, 1e-4),   #   KP 96 ragged, S > 1 without the mean
    (1, 32, (128, 128, 128), 0, (2, 0, 1), False, False, False, 1.0),    #   KP 32
    (1, 32, (128, 128), 0, (1, 2), False, True, False, 1.0),             # NL = 2 stored, no signs: vmcnt(16)
    (2, 128, (128, 128), 2, (2, 2), False, True, True, 1.0),             # NL = 2 stored, signs: vmcnt(17) (the regressor's pair)
    (2, 64, (96, 128), 1, (1, 1), True, True, True, 1.0),                #   KP 64, mean
    (2, 96, (128, 128, 128), 0, (1, 2, 0), True, True, False, 1.0),      # NL = 3 stored, no signs: vmcnt(32); S from the mean alone
    (2, 128, (128, 128, 128), 2, (1, 1, 0), True, True, True, 1.0),      # NL = 3 stored, signs: vmcnt(33) (a later embedding)
    (1, 93, (128, 128, 128), 1, (1, 1, 0), False, True, True, 1.0),      #   the first embedding: 93 features
    (1, 32, (25, 40, 17), 0, (2, 1, 2), False, True, True, 1.0),         #   narrow ragged layers
]


@pytest.mark.parametrize("s,cin,couts,t_mode,acts,mean,store_mid,want_signs,spread", CHAIN_CASES)
def test_chain_forward_walk_vs_float64(s, cin, couts, t_mode, acts, mean, store_mid, want_signs, spread):
    """sbmc_pointwise_chain_fwd_f32 with 4-5 units per workgroup: stored layers, sign words (bit for bit y > 0), magnitude
    words (max |y| exactly), the sample mean against float64 at 1e-5 of each tensor's scale; two launches bit-equal.
    Every count of wait_rows() runs in steady state here.  (Measured once: with the primed wait REMOVED these cases still pass on
    an MI355X -- at this size the rows land a tile ahead anyway; a weak count shows only under the 1280 x 720 test's store
    traffic.  What fails here and not at the small shapes: the running mean not reset between units, the maxima's double buffer
    not flipped at S = 1 -- anything wrong in what a workgroup carries from one unit to the next.)"""
    from sbmc_amd import functions as funcs
    dev = th.device("cuda")
    planes, hw = walk_shape(_cus())
    b = planes * s
    S = s if (t_mode or mean) else 1               # (the launch's: samples walked together)
    tpp = (hw + 63) // 64
    units = tpp * (b // S)
    _check_walk(units, grid_persistent(units), tpp, "chain forward")
    x, t, layers = _make(b, s, cin, couts, hw, t_mode, acts, spread, dev, 1000 * cin + hw)
    ref = _chain64(x, t, s, layers)
    run = lambda: funcs.pointwise_chain_forward(x, t, s, layers, store_mid=store_mid, want_signs=want_signs, mean=mean)
    ys, signs, amaxes, ymean = run()
    ys2, signs2, amaxes2, ymean2 = run()
    th.cuda.synchronize()
    tail = th.tensor([-1] * ((hw + 31) // 32 - 1) + [(1 << (hw % 32)) - 1], dtype=th.int32, device=dev)   # (bits within the plane)
    for l, r in enumerate(ref):
        if not (l + 1 == len(ref) or store_mid):
            assert ys[l] is None
            continue
        assert _rel(ys[l], r, "y%d" % l) <= 1e-5
        assert amaxes[l].item() == _word(ys[l]).item(), "magnitude word %d is not max |y|" % l
        assert th.equal(ys[l], ys2[l]) and amaxes[l].item() == amaxes2[l].item()
        assert (signs[l] is not None) == (want_signs and acts[l] != 0)
        if signs[l] is not None:
            assert th.equal(_sign_bits(signs[l], hw), ys[l] > 0)
            assert th.equal(signs[l] & tail, signs2[l] & tail)
    if mean:
        assert _rel(ymean, ref[-1].view(b // s, s, couts[-1], hw).mean(1), "mean") <= 1e-5
        assert th.equal(ymean, ymean2)


# ---------------------------------------------------------------------------------------------
# single-layer forwards
@pytest.mark.parametrize("s,cin,cout,t_mode,act,mean", [
    (1, 128, 128, 0, 2, False),          # signs, no mean
    (2, 96, 128, 1, 1, True),            # per-image context, signs and the sample mean
    (2, 128, 128, 2, 0, False),          # per-pixel context, linear: no signs
    (2, 64, 128, 0, 0, True),            # S from the mean alone
    (1, 128, 441, 0, 0, False),          # the logits layer: nrt = 4 workgroups per unit
])
def test_scaled_forward_walk_vs_float64(s, cin, cout, t_mode, act, mean):
    """sbmc_pointwise_fwd_scaled_f32, two planes (xmax) and three: y, sign words, magnitude word, mean."""
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    S = s if (t_mode or mean) else 1
    # (the number of workgroups that walk depends on the units only below 8 of them: take it at any large count)
    planes, hw = walk_shape(walkers_split_forward(1 << 20, cout))
    b = planes * S
    tpp = (hw + 63) // 64
    units = tpp * (b // S)
    _check_walk(units, walkers_split_forward(units, cout), tpp, "split forward")
    th.manual_seed(cout + hw)
    x = th.randn(b, cin, hw, device=dev)
    w = th.randn(cout, cin, device=dev) / cin ** 0.5
    bias = th.randn(cout, device=dev)
    t = None if t_mode == 0 else th.randn(*((b // S, cout) if t_mode == 1 else (b // S, cout, hw)), device=dev)
    ref, _ = _layer64(x, w, bias, t, S, act, SLOPE)
    wpr = (hw + 31) // 32
    for scaled in (True, False):
        what = "scaled" if scaled else "three planes"
        y = _nan(b, cout, hw)
        signs = th.zeros(b, cout, wpr, dtype=th.int32, device=dev) if act != 0 else None
        ymean = _nan(b // S, cout, hw) if mean else None
        amax = th.zeros(1, dtype=th.int32, device=dev)
        _lib.check(L.sbmc_pointwise_fwd_scaled_f32(
            _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(t), _lib.ptr(y), _lib.ptr(signs), _lib.ptr(ymean), S if mean else 1,
            _lib.ptr(_word(x)) if scaled else None, _lib.ptr(amax), b, S, cin, cout, hw, t_mode, act, SLOPE,
            _lib.current_stream(dev)), "fwd_scaled")
        assert _rel(y, ref, what + " y") <= 1e-5
        assert amax.item() == _word(y).item(), what + ": magnitude word is not max |y|"
        if mean:
            m = ref.view(b // S, S, cout, hw).mean(1)
            assert _rel(ymean, m, what + " mean") * m.abs().max().item() <= 1e-5 * ref.abs().max().item()
        if signs is not None:
            assert th.equal(_sign_bits(signs, hw), y > 0), what


@pytest.mark.parametrize("s,cin,cout,t_mode,act,mean", [
    (1, 128, 128, 0, 1, False),
    (2, 96, 128, 2, 2, False),           # per-pixel context; the walk is in plain tile order (S plays no part in it)
    (2, 128, 128, 0, 1, True),           # sbmc_pointwise_fwd_mean_f16: the samples of a tile one after the other
    (2, 128, 96, 1, 2, True),
])
def test_half_forward_walk_vs_float64(s, cin, cout, t_mode, act, mean):
    """sbmc_pointwise_fwd_f16 / _mean_f16 (all half: the f16 matrix pipe, weights rounded to half; 2 workgroups per CU on
    128-pixel tiles) against float64 of the ROUNDED values, at test_pointwise_half_training's bound: one half rounding of
    the output's scale + 1e-3.  The mean is the mean of the values as stored (pw_fwd_h_kernel), rounded to half once."""
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    planes, hw = walk_shape(walkers_split_forward(1 << 20, cout, per_cu=2), tile=128)
    b = planes * (s if mean else 1)
    tpp = (hw + 127) // 128
    units = tpp * b // (s if mean else 1)
    _check_walk(units, walkers_split_forward(units, cout, per_cu=2), tpp, "half forward", interleave=1 if (mean or not t_mode) else s)
    th.manual_seed(cout + hw + t_mode)
    x = th.randn(b, cin, hw, device=dev).half()
    w = th.randn(cout, cin, device=dev) / cin ** 0.5
    bias = th.randn(cout, device=dev)
    t = None if t_mode == 0 else th.randn(*((b // s, cout) if t_mode == 1 else (b // s, cout, hw)), device=dev)
    ref, _ = _layer64(x, w.half(), bias, t, s, act, SLOPE)
    y = _nan(b, cout, hw, dtype=th.float16)
    if mean:
        ymean = _nan(b // s, cout, hw, dtype=th.float16)
        _lib.check(L.sbmc_pointwise_fwd_mean_f16(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(t), _lib.ptr(y), _lib.ptr(ymean), s,
                                                 b, s, cin, cout, hw, t_mode, act, SLOPE, _lib.current_stream(dev)), "fwd_mean_f16")
    else:
        _lib.check(L.sbmc_pointwise_fwd_f16(_lib.ptr(x), 1, _lib.ptr(w), _lib.ptr(bias), _lib.ptr(t), _lib.ptr(y), b, s, cin, cout, hw,
                                            t_mode, act, SLOPE, _lib.current_stream(dev)), "fwd_f16")
    scale = ref.abs().max().item()
    assert _rel(y, ref, "y") * scale <= 2.0 ** -10 * scale + 1e-3
    if mean:
        m = y.double().view(b // s, s, cout, hw).mean(1)
        assert _rel(ymean, m, "mean") * m.abs().max().item() <= 2.0 ** -10 * scale + 1e-3


def test_wide_forward_walk_vs_float64():
    """sbmc_pointwise_wide_fwd_f32 with b > 1 and a ragged plane: edge tiles in mid-walk (the 1200-unit case of
    tests/test_gpu_pointwise_chain.py has two planes of whole tiles)."""
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    b, hw = walk_shape(_cus())
    cin, cout, act = 96, 441, 2
    tpp = (hw + 63) // 64
    _check_walk(tpp * b, grid_persistent(tpp * b), tpp, "wide forward")
    th.manual_seed(hw)
    x = th.randn(b, cin, hw, device=dev)
    w = th.randn(cout, cin, device=dev) / cin ** 0.5
    bias = th.randn(cout, device=dev)
    assert L.sbmc_pointwise_wide_fwd_supported(cin, cout, hw)
    y = _nan(b, cout, hw)
    amax = th.zeros(1, dtype=th.int32, device=dev)
    _lib.check(L.sbmc_pointwise_wide_fwd_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(amax), b, cin, cout, hw,
                                             act, SLOPE, _lib.current_stream(dev)), "wide_fwd")
    assert _rel(y, _chain64(x, None, 1, [(w, bias, act, SLOPE)])[0], "y") <= 1e-5
    assert amax.item() == _word(y).item()


# ---------------------------------------------------------------------------------------------
# backwards: float64 with the forward's own decisions; the partial sums a workgroup keeps over its 4-5 units
def _layer_inputs(b, s, cin, cout, hw, t_mode, seed):
    dev = th.device("cuda")
    th.manual_seed(seed)
    x = th.randn(b, cin, hw, device=dev)
    w = th.randn(cout, cin, device=dev) / cin ** 0.5
    bias = th.randn(cout, device=dev)
    t = None if t_mode == 0 else th.randn(*((b // s, cout) if t_mode == 1 else (b // s, cout, hw)), device=dev)
    return x, w, bias, t


@pytest.mark.parametrize("s,cin,cout,t_mode,act,gm,dx", [
    (1, 128, 128, 0, 2, False, True),
    (2, 128, 128, 0, 0, True, True),     # an embedding's last (linear) layer with the mean's gradient
    (2, 128, 128, 2, 1, False, True),    # per-pixel context gradient
    (2, 96, 128, 1, 1, False, False),    # the first embedding's first layer: no data gradient, per-image context gradient
    (2, 64, 96, 0, 2, True, True),
])
def test_scaled_backward_walk_vs_float64(s, cin, cout, t_mode, act, gm, dx):
    """sbmc_pointwise_bwd_scaled_f32, two planes (the RAW kernel: vmcnt(16) behind its 16 gx stores) and three: gx and its
    word, the summed gw / gbias partials, gt per image and per pixel, every row of the NaN-filled partial buffers written."""
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    S = s if (t_mode or gm) else 1
    planes, hw = walk_shape(_cus())
    b = planes * S
    tpp = (hw + 63) // 64
    groups = L.sbmc_pointwise_bwd_groups(b, S, 1 if (gm and t_mode == 0) else t_mode, hw)        # (as functions.py)
    _check_walk(tpp * (b // S), groups, tpp, "backward")
    x, w, bias, t = _layer_inputs(b, S, cin, cout, hw, t_mode, cin + cout + hw)
    gy = th.randn(b, cout, hw, device=dev)
    gmean = th.randn(b // S, cout, hw, device=dev) if gm else None
    # the forward on the GPU for the sign bits the backward reads
    y = th.empty(b, cout, hw, device=dev)
    signs = th.zeros(b, cout, (hw + 31) // 32, dtype=th.int32, device=dev)
    _lib.check(L.sbmc_pointwise_fwd_scaled_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(t), _lib.ptr(y), _lib.ptr(signs), None, 1,
                                               _lib.ptr(_word(x)), None, b, S, cin, cout, hw, t_mode, act, SLOPE,
                                               _lib.current_stream(dev)), "fwd")
    gx64, gw64, gb64, gt64 = _backward64(x, w, y > 0, gy, gmean, S, t_mode, act, SLOPE)
    nb = b // S if t_mode == 1 else 1
    for scaled in (True, False):
        what = "scaled" if scaled else "three planes"
        gx = _nan(b, cin, hw) if dx else None
        gwp, gbp = _nan(groups, cout, cin), _nan(groups, nb, cout)
        gt = _nan(b // S, cout, hw) if t_mode == 2 else None
        # (the three-plane kernels with a context / mean gradient keep no running maximum)
        want_word = dx and (scaled or not (gm or t_mode == 2))
        gxmax = th.zeros(1, dtype=th.int32, device=dev) if want_word else None
        _lib.check(L.sbmc_pointwise_bwd_scaled_f32(
            _lib.ptr(gy), _lib.ptr(signs) if act != 0 else None, _lib.ptr(x), _lib.ptr(w), _lib.ptr(gx), _lib.ptr(gwp), _lib.ptr(gbp),
            _lib.ptr(gt), _lib.ptr(gmean), S, _lib.ptr(_word(gy)) if scaled else None,
            _lib.ptr(_word(gmean)) if (scaled and gm) else None, _lib.ptr(_word(x)) if scaled else None, _lib.ptr(gxmax),
            b, S, cin, cout, hw, t_mode, act, SLOPE, _lib.current_stream(dev)), "bwd_scaled")
        if dx:
            assert _rel(gx, gx64, what + " gx") <= 1e-5
            if want_word:
                assert gxmax.item() == _word(gx).item(), what
        assert th.isfinite(gwp).all() and th.isfinite(gbp).all(), what + ": a row of the partial sums was not written"
        assert _rel(gwp.double().sum(0), gw64, what + " gw") <= 1e-5
        per_image = gbp.double().sum(0)
        assert _rel(per_image.sum(0), gb64, what + " gbias") <= 1e-5
        if t_mode == 1:
            assert _rel(per_image, gt64, what + " gt per image") <= 1e-5
        if t_mode == 2:
            assert _rel(gt, gt64, what + " gt per pixel") <= 1e-5


@pytest.mark.parametrize("s,cin,cout,t_mode,act,gm", [
    (2, 128, 128, 0, 1, True),           # (relu and S = 2: gz is formed exactly on either side)
    (2, 96, 128, 2, 2, False),
])
def test_half_backward_walk_vs_float64(s, cin, cout, t_mode, act, gm):
    """sbmc_pointwise_bwd_f16 (all half, the f16 matrix pipe) against float64 on exactly the values the kernel sees, as
    test_pointwise_half_training: gz = gy act'(y) in fp32, rounded to half once for the products, the weights rounded to half
    for gx; gx to one half rounding of its scale (+ 1e-6), gw / gbias to helpers.close_sum's bound with that test's
    allowance, the per-pixel context gradient (fp32) to 1e-5."""
    from helpers import close_sum
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    S = s if (t_mode or gm) else 1
    planes, hw = walk_shape(_cus())
    b = planes * S
    tpp = (hw + 63) // 64
    groups = L.sbmc_pointwise_bwd_groups(b, S, 1 if (gm and t_mode == 0) else t_mode, hw)
    _check_walk(tpp * (b // S), groups, tpp, "half backward")
    x, w, bias, t = _layer_inputs(b, S, cin, cout, hw, t_mode, cin + hw)
    x = x.half()
    y = _layer64(x, w.half(), bias, t, S, act, SLOPE)[0].half()                  # (what a half forward stored: its decisions)
    gy = th.randn(b, cout, hw, device=dev).half()
    gmean = th.randn(b // S, cout, hw, device=dev).half() if gm else None
    gx = _nan(b, cin, hw, dtype=th.float16)
    gwp, gbp = _nan(groups, cout, cin), _nan(groups, 1, cout)
    gt = _nan(b // S, cout, hw) if t_mode == 2 else None
    _lib.check(L.sbmc_pointwise_bwd_f16(_lib.ptr(gy), _lib.ptr(y), _lib.ptr(x), 1, _lib.ptr(w), _lib.ptr(gx), _lib.ptr(gwp), _lib.ptr(gbp),
                                        _lib.ptr(gt), _lib.ptr(gmean), S, b, S, cin, cout, hw, t_mode, act, SLOPE,
                                        _lib.current_stream(dev)), "bwd_f16")
    g = gy.float()
    if gm:
        g = g + gmean.float().repeat_interleave(S, 0) / S
    gz = th.where(y > 0, g, g * (SLOPE if act == 2 else 0.0))
    gzq, xd = gz.half().double(), x.double()
    gxr = th.einsum("oc,bop->bcp", w.half().double(), gzq)
    assert _rel(gx, gxr, "gx") * gxr.abs().max().item() <= 2.0 ** -10 * gxr.abs().max().item() + 1e-6
    assert th.isfinite(gwp).all() and th.isfinite(gbp).all(), "a row of the partial sums was not written"
    close_sum(gwp.double().sum(0), th.einsum("bop,bcp->oc", gzq, xd), th.einsum("bop,bcp->oc", gzq.abs(), xd.abs()), what="gw",
              extra=(8 * 2.0 ** -11 * gzq.abs().max() * xd.abs().max()).item())
    close_sum(gbp.double().sum((0, 1)), gz.double().sum((0, 2)), gz.double().abs().sum((0, 2)), what="gbias")
    if t_mode == 2:
        assert _rel(gt, gz.double().view(b // S, S, cout, hw).sum(1), "gt per pixel") <= 1e-5


def _wide_inputs(b, cin, cout, hw):
    dev = th.device("cuda")
    th.manual_seed(b * 31 + cout)
    gz = th.randn(b, cout, hw, device=dev) * 1e-3
    gz[:, :, ::7] *= 30.0                              # a wide spread of magnitudes, as logit gradients have
    x = th.randn(b, cin, hw, device=dev).relu_()
    w = th.randn(cout, cin, device=dev) / cin ** 0.5
    return gz, x, w


def test_wide_weight_gradient_walk_vs_float64():
    """sbmc_pointwise_gw_wide_f32 (pw_gw_wide_kernel): the 441-channel layer's gw / gbias partial sums."""
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    b, hw = walk_shape(_cus())
    cin, cout = 128, 441
    tpp = (hw + 63) // 64
    groups = L.sbmc_pointwise_gw_wide_groups(b, hw)
    _check_walk(tpp * b, groups, tpp, "wide weight gradient")
    gz, x, _ = _wide_inputs(b, cin, cout, hw)
    gwp, gbp = _nan(groups, cout, cin), _nan(groups, cout)
    _lib.check(L.sbmc_pointwise_gw_wide_f32(_lib.ptr(gz), _lib.ptr(x), _lib.ptr(gwp), _lib.ptr(gbp), b, cin, cout, hw,
                                            _lib.current_stream(dev)), "gw_wide")
    assert th.isfinite(gwp).all() and th.isfinite(gbp).all(), "a row of the partial sums was not written"
    assert _rel(gwp.double().sum(0), th.einsum("bop,bkp->ok", gz.double(), x.double()), "gw") <= 1e-5
    assert _rel(gbp.double().sum(0), gz.double().sum((0, 2)), "gbias") <= 1e-5


@pytest.mark.parametrize("loose", [1.0, 37.0])
@pytest.mark.parametrize("cin,cout", [(128, 441), (96, 200)])
def test_wide_backward_walk_vs_float64(cin, cout, loose):
    """sbmc_pointwise_wide_bwd_f32 (pw_wide_bwd2_kernel: vmcnt(4) / vmcnt(NX + 4 + 16) behind its x requests and gx stores),
    4 and 2 row tiles, the gradient's word tight and a bound: gx and its word, summed gw / gbias partials."""
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    b, hw = walk_shape(_cus())
    tpp = (hw + 63) // 64
    groups = L.sbmc_pointwise_gw_wide_groups(b, hw)
    _check_walk(tpp * b, groups, tpp, "wide backward")
    gz, x, w = _wide_inputs(b, cin, cout, hw)
    gwp, gbp, gx = _nan(groups, cout, cin), _nan(groups, cout), _nan(b, cin, hw)
    ws = th.empty(L.sbmc_pointwise_wide_bwd_ws_bytes(), dtype=th.uint8, device=dev)
    gxmax = th.zeros(1, dtype=th.int32, device=dev)
    gword = (gz.abs().max() * loose).reshape(1).view(th.int32).clone()
    _lib.check(L.sbmc_pointwise_wide_bwd_f32(_lib.ptr(gz), _lib.ptr(x), _lib.ptr(w), _lib.ptr(gx), _lib.ptr(gwp), _lib.ptr(gbp), _lib.ptr(ws),
                                             _lib.ptr(gword), _lib.ptr(_word(x)), _lib.ptr(gxmax), b, cin, cout, hw,
                                             _lib.current_stream(dev)), "wide_bwd")
    assert _rel(gx, th.matmul(w.double().t(), gz.double()), "gx") <= 1e-5
    assert gxmax.item() == _word(gx).item()
    assert th.isfinite(gwp).all() and th.isfinite(gbp).all(), "a row of the partial sums was not written"
    assert _rel(gwp.double().sum(0), th.einsum("bop,bkp->ok", gz.double(), x.double()), "gw") <= 1e-5
    assert _rel(gbp.double().sum(0), gz.double().sum((0, 2)), "gbias") <= 1e-5


@pytest.mark.parametrize("loose", [1.0, 23.0])
@pytest.mark.parametrize("s,cin,t_mode,act1,act0,dx", [
    (2, 128, 2, 2, 2, True),             # the regressor's first two layers: per-pixel context gradient
    (2, 93, 1, 1, 1, False),             # the first embedding: no data gradient, per-image context gradient
    (1, 64, 0, 0, 1, True),              # the upper layer linear
])
def test_chain_pair_backward_walk_vs_float64(s, cin, t_mode, act1, act0, dx, loose):
    """sbmc_pointwise_chain_bwd_f32 (pw_chain_bwd_kernel) through the ABI as test_chain_pair_backward_vs_float64: gx and its
    word, both layers' summed gw / gbias partials, the context gradient, against float64 with the forward's decisions."""
    from sbmc_amd import _lib
    L = _lib.lib()
    dev = th.device("cuda")
    S = s if t_mode else 1
    planes, hw = walk_shape(_cus())
    b = planes * S
    tpp = (hw + 63) // 64
    groups = L.sbmc_pointwise_chain_bwd_groups(b, S, t_mode, hw)
    _check_walk(tpp * (b // S), groups, tpp, "pair backward")
    x, t, layers = _make(b, S, cin, (128, 128), hw, t_mode, (act0, act1), 1.0, dev, b * 7 + hw)
    (w0, b0, _, sl0), (w1, b1, _, sl1) = layers
    y = _chain64(x, t, S, layers)
    y0, bits = y[0].float(), y[1].float() > 0          # what the forward stored (its decisions: y0 > 0), its sign bits
    signs1 = _pack_signs(bits)
    del y
    th.manual_seed(3)
    gy = th.randn(b, 128, hw, device=dev) * 1e-2
    gy[:, :, ::5] *= 20.0
    nb = b // S if t_mode == 1 else 1
    gx = _nan(b, cin, hw) if dx else None
    gwp1, gbp1, gwp0, gbp0 = _nan(groups, 128, 128), _nan(groups, 128), _nan(groups, 128, cin), _nan(groups, nb, 128)
    gt = _nan(b // S, 128, hw) if t_mode == 2 else None
    words = [(_word(v).view(th.float32) * loose).view(th.int32) for v in (gy, y0, x)]
    gxmax = th.zeros(1, dtype=th.int32, device=dev) if dx else None
    _lib.check(L.sbmc_pointwise_chain_bwd_f32(
        _lib.ptr(gy), _lib.ptr(signs1) if act1 else None, _lib.ptr(y0), _lib.ptr(w1), _lib.ptr(x), _lib.ptr(w0), _lib.ptr(gx),
        _lib.ptr(gwp1), _lib.ptr(gbp1), _lib.ptr(gwp0), _lib.ptr(gbp0), _lib.ptr(gt), _lib.ptr(words[0]), _lib.ptr(words[1]),
        _lib.ptr(words[2]), _lib.ptr(gxmax), b, S, cin, hw, t_mode, act1, sl1, act0, sl0, _lib.current_stream(dev)), "chain_bwd")
    gz1, gz0 = _pair_gz64(gy, bits, y0 > 0, w1, act1, sl1, act0, sl0)
    y0d, xd = y0.double(), x.double()
    for p in (gwp1, gbp1, gwp0, gbp0):
        assert th.isfinite(p).all(), "a row of the partial sums was not written"
    assert _rel(gwp1.double().sum(0), th.einsum("bop,bkp->ok", gz1, y0d), "gw1") <= 1e-5
    assert _rel(gbp1.double().sum(0), gz1.sum((0, 2)), "gb1") <= 1e-5
    assert _rel(gwp0.double().sum(0), th.einsum("bop,bkp->ok", gz0, xd), "gw0") <= 1e-5
    assert _rel(gbp0.double().sum((0, 1)), gz0.sum((0, 2)), "gb0") <= 1e-5
    if t_mode == 1:
        assert _rel(gbp0.double().sum(0), gz0.view(b // S, S, 128, hw).sum((1, 3)), "gt per image") <= 1e-5
    elif t_mode == 2:
        assert _rel(gt, gz0.view(b // S, S, 128, hw).sum(1), "gt per pixel") <= 1e-5
    if dx:
        assert _rel(gx, th.einsum("ok,bop->bkp", w0.double(), gz0), "gx") <= 1e-5
        assert gxmax.item() == _word(gx).item()
