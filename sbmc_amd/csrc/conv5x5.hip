// 5 x 5 convolution of a channels-last fp32 image, stride 1, NO padding ("valid": the output is 4 pixels smaller each
// way) -- every convolution of KPCN's two chains (reference sbmc/models.py:221-291: ConvChain(27, k^2, ksize=5,
// width=100, depth=9, pad=False)) -- at fp32 accuracy on the f16 matrix pipe, with bias + activation in the epilogue.
//
// The arithmetic is csrc/conv3x3.hip's: both operands are scaled by a power of two taken from their tensor's largest
// magnitude and split into two f16 planes (common.hpp: f16_split_pair, pow2_scale_of), three exact products per term,
//     x w = (hx hw + hx lw + lx hw) / (cx cw),
// accumulated in fp32 by v_mfma_f32_32x32x16_f16.  The plan is not: the 3 x 3 kernel keeps a whole 32-channel patch in
// two buffers and three weight stages in LDS, which for a 20 x 20 patch and five taps per kernel row is 222 KB.
//
// CHANNELS.  KPCN's counts (27, 100, 441 / 25) fit no tile, so the kernel never sees ragged channels: every tensor
// lives in a channels-last buffer [n][h][w][ld] whose channel stride ld is the count rounded up to 16 (100 -> 112), with
// EXACT ZEROS in the padding channels; the prepared weights are zero-padded to match (16 on the reduction side, the
// 128-channel output tile on the other).  A padding output channel has zero weights and no bias: the epilogue writes
// act(0) = 0 there, which is what the next layer needs to read.  100 -> 100 runs as K = 112 x N = 128: 1.43 x the
// matrix products of the unpadded shape (30 % wasted).
//
// Implicit GEMM, A = pixels x (tap, cin) from the image, B = (tap, cin) x cout from the weights:
//   * a workgroup (4 waves, one per SIMD) owns 16 x 16 output pixels x 128 output channels; a wave 8 x 16 pixels x 64
//     channels = 4 x 2 accumulators of 32 x 32, twice: hx hw in one set, the two cross products in another (256 of the
//     wave's 512 registers), so that the large sum is rounded once per term, not three times;
//   * the reduction runs in CHUNKS of 16 input channels; the 20 x 20 patch of a chunk is fetched once for all 25
//     taps (fp32, 64 contiguous bytes per pixel), split in registers and kept in LDS as [plane][octet][pixel] 16-byte
//     entries (25.7 KB): the A operand of tap (ky, kx) is the same image shifted by ky rows and kx entries, one
//     conflict-free ds_read_b128 (the second row of a 32-pixel block is rotated by 20 mod 16 = 4 columns);
//   * a weight STAGE is one kernel row of a chunk: 5 taps x 16 input channels x 128 output channels x 2 planes = 40 KB,
//     contiguous in the prepared weights, copied to LDS as it is;
//   * two patch buffers + two weight stages = 133 376 bytes of LDS: one workgroup per CU, one wave per SIMD with the
//     whole register file.  The next stage's weights (and, in a chunk's fourth stage, the next chunk's patch) are
//     requested BEFORE the stage's 120 MFMAs per wave and written to the other buffer behind them: one barrier per
//     stage, 120 MFMAs (3840 matrix-pipe cycles) per wave between two barriers;
//   * per tap a wave reads 8 patch + 4 weight operands for 24 MFMAs, the next tap's between the current one's MFMAs
//     (0.5 of the LDS bandwidth at full matrix rate, as in the 3 x 3 kernel);
//   * one workgroup per (pixel tile, output-channel tile), output-channel tiles of a pixel tile next to each other in
//     the grid (they read the same patch through L2).  Not persistent: a tile is >= 10 stages, its unoverlapped
//     prologue (one patch, one stage) a few per cent of that.
// Edges: patch pixels beyond the image are buffer loads out of range (zeros), output pixels beyond it and channels
// from ld up are masked stores; every descriptor's range ends with its tensor.
//
// The tile body is csrc/conv5x5_gemm_body.inc, shared with the data gradient (conv5x5_grad.hip), which takes its
// `Side::mirror` branches; this file has the kernel that includes it, the fp32 weight preparation, the host checks and the
// entry points.  The repack kernels and the prepare unit are conv5x5_common.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sbmc_hip.h"
#include "common.hpp"
#include "conv5x5_common.hpp"

namespace sbmc {

// The forward Side of the shared body: A = x, Y = y, aux = bias [Cout].  The patch starts at the tile's own first pixel,
// which is the descriptor's base: a patch pixel can only lie beyond the image's bottom or right edge, one side to check
// per coordinate.  Stage j reads prepared kernel row j, tap i column i; the epilogue: scale back, bias, activation.
__global__ __launch_bounds__(256) void conv5_kernel(Conv5Params p) {
    using Side = Conv5Fwd;
#include "conv5x5_gemm_body.inc"
}

// ---- weights [cout][cin][5][5] (any strides) -> the two f16 planes in stage order, zero-padded ----
// entry ((((ct K16 + k16) 5 + ky) 5 + kx) 2 + plane) 2 + khalf) 128 + co holds the 8 values of conv5x5_common.hpp's
// unit (ct, k16, ky, kx, khalf, co)
struct Prep5Params {
    Prep5Src src;
    const unsigned* wmax;
    u32x4* wp;
    float* wscale;
};
__global__ __launch_bounds__(256) void prep5_weights_kernel(Prep5Params p) {
    const float c = pow2_scale_of(*p.wmax);
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u == 0) *p.wscale = c;
    if (u >= prep5_units(p.src)) return;
    const Prep5Unit t = prep5_unit(p.src, u);
    u32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned hp, lp;
        f16_split_pair(t.v[2 * i], t.v[2 * i + 1], c, hp, lp);
        h[i] = hp;
        l[i] = lp;
    }
    const long base = ((((long)(t.ct * p.src.K16 + t.k16) * 5 + t.ky) * 5 + t.kx) * 2) * 2 * C5_NT + t.khalf * C5_NT + t.co;
    p.wp[base] = h;
    p.wp[base + 2 * C5_NT] = l;
}

// one descriptor spans a tile's patch rows of the input and its tile rows of the output
static bool conv5_strides_ok(int w, long long ldx, long long ldy) {
    return c5_strides_ok(C5_PS + 1, w, ldx, C5_TS + 1, w - 4, ldy, 4);
}

static bool conv5_dims_ok(int n, int h, int w, int cin, int cout) {
    if (!c5_shape_ok(n, h, w, cin, cout)) return false;
    const long long ldx = c5_pad16(cin), ldy = c5_pad16(cout), ncot = (cout + C5_NT - 1) / C5_NT;
    if (!conv5_strides_ok(w, ldx, ldy)) return false;
    const long long tiles = (long long)n * ((h - 4 + C5_TS - 1) / C5_TS) * ((w - 4 + C5_TS - 1) / C5_TS) * ncot;
    return tiles < 0x7FFFFFFFll && ncot * (ldx / 16) * 5 * C5_WSTAGE * 16 < C5_MAXOFF;
}

}  // namespace sbmc

using namespace sbmc;

extern "C" int sbmc_conv5x5_supported(int n, int h, int w, int cin, int cout) {
    return conv5_dims_ok(n, h, w, cin, cout) ? 1 : 0;
}

extern "C" int sbmc_conv5x5_padded_channels(int c) { return c < 1 || c > (1 << 20) ? 0 : c5_pad16(c); }

extern "C" size_t sbmc_conv5x5_weights_bytes(int cin, int cout) {
    if (!conv5_dims_ok(1, 5, 5, cin, cout)) return 0;
    // prepared planes + [scale, bit pattern of the largest magnitude]
    return (size_t)((cout + C5_NT - 1) / C5_NT) * (c5_pad16(cin) / 16) * 5 * C5_WSTAGE * 16 + 16;
}

extern "C" int sbmc_conv5x5_prepare_weights_f32(const float* w, long s_co, long s_ci, long s_ky, long s_kx,
                                                 long storage_elems, int cin, int cout, void* wp, void* stream) {
    const size_t bytes = sbmc_conv5x5_weights_bytes(cin, cout);
    if (!bytes || !w || !wp || (uintptr_t)wp % 16 || (uintptr_t)w % 16 || storage_elems < 1) return SBMC_HIP_EINVAL;
    char* tail = static_cast<char*>(wp) + bytes - 16;
    float* wscale = reinterpret_cast<float*>(tail);
    unsigned* wmax = reinterpret_cast<unsigned*>(tail + 4);
    const int rc = sbmc_conv3x3_absmax_f32(w, storage_elems, wmax, stream);
    if (rc != 0) return rc;
    const Prep5Params p{prep5_src(w, s_co, s_ci, s_ky, s_kx, cin, cout), wmax, static_cast<u32x4*>(wp), wscale};
    const long units = prep5_units(p.src);
    hipLaunchKernelGGL(prep5_weights_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_bias_act_nhwc_f32(const float* x, int ldx, const unsigned* xmax, const void* wp,
                                               const float* bias, float* y, int ldy, int n, int h, int w, int cin,
                                               int cout, float slope, unsigned* amax, void* stream) {
    if (!conv5_dims_ok(n, h, w, cin, cout) || !x || !xmax || !wp || !bias || !y) return SBMC_HIP_EINVAL;
    if (!c5_ld_ok(ldx, cin) || !c5_ld_ok(ldy, cout)) return SBMC_HIP_EINVAL;
    if ((uintptr_t)x % 16 || (uintptr_t)wp % 16 || (uintptr_t)y % 16 || (uintptr_t)bias % 4 || (uintptr_t)xmax % 4 ||
        (uintptr_t)amax % 4)
        return SBMC_HIP_EINVAL;
    // (a buffer wider than the rounded channel count: the same 31-bit rule for its strides)
    if (!conv5_strides_ok(w, ldx, ldy)) return SBMC_HIP_EINVAL;
    Conv5Params p;
    p.a = x; p.wp = static_cast<const u32x4*>(wp); p.y = y; p.amag = xmax;
    p.wscale = reinterpret_cast<const float*>(static_cast<const char*>(wp) + sbmc_conv5x5_weights_bytes(cin, cout) - 16);
    p.aux = bias; p.amax = amax;                          // (this Side's aux: the bias, Cout values)
    p.N = n; p.Ha = h; p.Wa = w; p.Hy = h - 4; p.Wy = w - 4; p.lda = ldx; p.ldy = ldy; p.Cout = cout;
    p.K16 = c5_pad16(cin) / 16;
    p.tiles_x = (p.Wy + C5_TS - 1) / C5_TS; p.tiles_y = (p.Hy + C5_TS - 1) / C5_TS; p.nct = (cout + C5_NT - 1) / C5_NT;
    p.slope = slope;
    return conv5_gemm_launch(conv5_kernel, p, stream);
}

extern "C" int sbmc_conv5x5_pack_nchw_f32(const float* x, float* y, int ldy, int n, int c, long hw, void* stream) {
    return repack5<float, float, true>(x, y, ldy, n, c, hw, stream);
}

extern "C" int sbmc_conv5x5_unpack_nhwc_f32(const float* x, int ldx, float* y, int n, int c, long hw, void* stream) {
    return repack5<float, float, false>(x, y, ldx, n, c, hw, stream);
}
