// 5 x 5 convolution of a channels-last HALF image, stride 1, NO padding ("valid") -- every convolution of KPCN's two
// chains (reference sbmc/models.py:221-291) under torch.autocast(float16) -- with bias + activation in the epilogue and
// a half result: the one-plane sibling of csrc/conv5x5.hip, as Conv3x3BiasActHalfNHWC is of the fp32 3 x 3 kernel.
//
// The arithmetic is autocast's: the half inputs as they are, the fp32 weights rounded to half once (at preparation),
// exact products summed in fp32 by v_mfma_f32_32x32x16_f16, bias and activation in fp32, ONE rounding to half on the
// store.  No scales, no magnitude words: a value beyond the half range becomes inf, as with the library.
//
// CHANNELS, as in conv5x5.hip: every tensor is a channels-last buffer [n][h][w][ld], ld the count rounded up to 16, EXACT
// ZEROS in the padding channels (kept zero from layer to layer: a padding output channel has zero weights and no bias,
// the epilogue writes act(0) = 0), the prepared weights zero-padded to match (16 on the reduction side, 128 on the other).
//
// Implicit GEMM, A = pixels x (tap, cin) from the image, B = (tap, cin) x cout from the weights.  With one plane and one
// accumulator set the fp32 kernel's wave tile (8 x 16 pixels x 64 channels) would read 4 + 2 operands per 8 MFMAs: 0.75
// of the LDS bandwidth at full matrix rate.  The registers the second accumulator set occupied go into a wider wave tile:
//   * a workgroup (4 waves, one per SIMD) owns 32 x 16 output pixels (rows x columns) x 128 output channels; a wave
//     8 x 16 pixels x ALL 128 channels = 4 x 4 accumulators of 32 x 32 (256 of the wave's 512 registers): per tap 4 patch
//     + 4 weight operands for 16 MFMAs, 0.5 of the LDS bandwidth again; the four waves read the same weights and four
//     different row bands of the patch;
//   * the patch (36 x 20 pixels) is kept per CHUNK of 32 input channels, 64 contiguous bytes per pixel, fetched once for
//     all 25 taps and both K = 16 steps, copied to LDS as it is: [octet 4][pixel] 16-byte entries (46 336 bytes; the
//     region stride 724 = 4 mod 16 spreads the four octets of four neighbouring pixels that 16 staging lanes write over
//     all 16 slots of 16 bytes).  The A operand of tap (ky, kx), K step ks is the same image shifted by ky rows and kx
//     entries in octets 2 ks, 2 ks + 1: conv5x5.hip's conflict-free ds_read_b128 (the second row of a 32-pixel block
//     rotated by 20 mod 16 = 4 columns), "plane" read as "second 16 channels";
//   * a weight STAGE is one kernel row of ONE granule of 16 input channels: 5 taps x 2 octets x 128 output channels =
//     1280 entries = 20 480 bytes, contiguous in the prepared weights, copied as it is, double-buffered;
//   * two patch buffers + two weight stages = 133 632 bytes of LDS: one workgroup per CU, one wave per SIMD with the
//     whole register file.  The next stage's weights (and, in three of a granule's five stages, two of the twelve
//     three-row rounds of the NEXT chunk's patch) are requested BEFORE the stage's 80 MFMAs per wave and written to the
//     other buffer behind them: one barrier per stage, no load under a branch, one loop body for every granule;
//   * the reduction walks GRANULES, not chunks: 100 channels are 7 granules, the last chunk's second K step does not
//     exist -- 35 stages, not 40 -- and its upper two octets are not fetched (their lanes' offsets are out of range);
//   * a layer's prepared weights: cout tiles x granules x 5 kernel rows x 20 480 bytes (100 -> 441: 4 x 7 x 5 x 20 480 =
//     2 867 200 bytes).
// Two waves per SIMD on the 64-channel wave tile were the alternative, had 256 accumulators + operands + staging not
// fitted one wave's registers: they do (profiles/conv5x5_half_kernel_resources.txt: 256 AGPRs + 84 VGPRs, no spill,
// occupancy 1), so the wide tile with its lower LDS traffic ships.
// Edges: patch pixels beyond the image are buffer loads out of range (zeros), output pixels beyond it and channels from
// ld up are masked stores; every descriptor's range ends with its tensor.  Vector stores only.
// From conv5x5_common.hpp this file takes what does not depend on the fp32 kernels' 16 x 16 plan: C5_NT (128 output
// channels), c5_rsrc, c5_mfma, c5_pad16, C5_OOB, C5_MAXOFF and the vector types; the grid decode c5_tile and the 32 x 32
// block's lane rotation and accumulator map (c5_pcol, c5_acc_row, c5_acc_col); the prepare unit (prep5_unit), the repack
// (repack5) and the host rules (c5_shape_ok, c5_ld_ok, c5_strides_ok).  NOT conv5x5_gemm_body.inc: the main loop below is
// another plan, and its tile, patch and stage constants are the H5_ ones.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sbmc_hip.h"
#include "common.hpp"
#include "conv5x5_common.hpp"

namespace sbmc {

constexpr int H5_TY = 32, H5_TX = 16;                 // tile (output pixels): rows x columns
constexpr int H5_PY = H5_TY + 4, H5_PX = H5_TX + 4;   // patch
constexpr int H5_PP = H5_PY * H5_PX;                  // patch pixels (720)
constexpr int H5_PR = H5_PP + 4;                      // entries of one octet's region: 724 = 4 (mod 16)
constexpr int H5_ABUF = 4 * H5_PR;                    // 16-byte entries of one patch chunk: [octet 4][pixel]
constexpr int H5_WSTAGE = 5 * 2 * C5_NT;              // 16-byte entries of one weight stage: [kx 5][k half 2][cout 128]
constexpr unsigned H5_LDS_BYTES = (2 * H5_ABUF + 2 * H5_WSTAGE) * 16;      // 133632 of the CU's 163840
constexpr int H5_AROUNDS = H5_PY / 3;                                      // staging rounds of three patch rows: 12
constexpr int H5_WROUNDS = H5_WSTAGE / 256;                                // 5 entries of a stage per thread

struct Conv5HalfParams {
    const _Float16* x;       // [N, H, W, ldx]
    const u32x4* wp;         // prepared weights: [cout tile][K16][ky][kx][k half][128] entries of 8 halves
    _Float16* y;             // [N, H - 4, W - 4, ldy]
    const float* bias;       // [Cout]
    int N, H, W, Ho, Wo, ldx, ldy, Cout;
    int K16;                 // granules of 16 input channels
    int tiles_x, tiles_y, ncot;
    float slope;             // 1: linear, 0: ReLU, else LeakyReLU
};

__global__ __launch_bounds__(256) void conv5_half_kernel(Conv5HalfParams p) {
    extern __shared__ float4 h5_lds[];
    u32x4* As = reinterpret_cast<u32x4*>(h5_lds);
    u32x4* Ws = As + 2 * H5_ABUF;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_id();
    const int l31 = lane & 31, lhi = lane >> 5;
    const int pcol = c5_pcol(l31);
    const int K16 = p.K16, nchunks = (K16 + 1) >> 1, nstages = K16 * 5;

    const C5Tile tl = c5_tile<H5_TY, H5_TX>(blockIdx.x, p.ncot, p.tiles_x, p.tiles_y);
    const int ct = tl.ct, x0 = tl.x0, y0 = tl.y0, n = tl.n;

    // ---- staging of a patch chunk: 16-byte units (pixel, octet), 80 in a patch row; threads 0 .. 239 take three rows a
    // round, twelve rounds: ONE offset register, a wave-uniform step between rounds, one LDS address + immediates.
    // Threads 240 .. 255 double threads 224 .. 239 (the same unit read and written twice) instead of sitting out under a
    // branch: the compiler moves loads whose values are only used under a branch into it, behind the MFMAs ----
    const long long xelems = (long long)p.N * p.H * p.W * p.ldx;
    const long long xfirst = (((long long)n * p.H + y0) * p.W + x0) * p.ldx;
    const rsrc_t rx = c5_rsrc(p.x + xfirst, (xelems - xfirst) * 2);
    const rsrc_t rnone = c5_rsrc(p.x, 0);
    const int atid = tid < 3 * 4 * H5_PX ? tid : tid - 16;
    const int arow = atid / (4 * H5_PX), acol = (atid % (4 * H5_PX)) >> 2, aoct = atid & 3;
    const bool aidle = x0 + acol >= p.W;
    const unsigned avoff = (unsigned)((arow * p.W + acol) * p.ldx + aoct * 8) * 2u;
    const unsigned astep = (unsigned)(3 * p.W * p.ldx) * 2u;
    const int arows = aidle ? 0 : p.H - y0 - arow;     // round j's row is in the image while 3 j < arows
    // (valid = false: a request beyond the last chunk -- an empty descriptor, every lane reads zero.  The range check
    // sees the lane's offset only, not the chunk's: the lanes of a granule that does not exist -- the upper octets of an
    // odd count's last chunk -- are switched off by their offset, like those beyond the image.)
    // One round j (three patch rows) per call: two rounds a stage in the main loop, so that eight registers, not 48, wait
    // behind a stage's MFMAs; all twelve at once in the prologue.
    auto issue_a = [&](int cc, int j, bool valid) -> u32x4 {
        const rsrc_t r = valid ? rx : rnone;
        const int rows = (aoct >= 2 && 2 * cc + 1 >= K16) ? 0 : arows;
        return __builtin_amdgcn_raw_buffer_load_b128(r, 3 * j < rows ? avoff + (unsigned)j * astep : C5_OOB,
                                                     (unsigned)cc * 64u, 0);
    };
    u32x4* const a_dst = As + aoct * H5_PR + arow * H5_PX + acol;
    auto commit_a = [&](int abuf, int j, u32x4 v) { a_dst[abuf * H5_ABUF + j * 3 * H5_PX] = v; };
    // ---- staging of a weight stage s = 5 granule + ky: 1280 entries, 5 per thread ----
    const long long wentries = (long long)p.ncot * nstages * H5_WSTAGE;
    const rsrc_t rw = c5_rsrc(p.wp, wentries * 16);
    u32x4 wreg[H5_WROUNDS];
    auto issue_w = [&](int s, bool valid) {
        const rsrc_t r = valid ? rw : rnone;
        const unsigned block = valid ? (unsigned)(ct * nstages + s) : 0u;
#pragma unroll
        for (int i = 0; i < H5_WROUNDS; ++i)
            wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)(tid + 256 * i) * 16u,
                                                            block * (unsigned)(H5_WSTAGE * 16), 0);
    };
    auto commit_w = [&](int wbuf) {
#pragma unroll
        for (int i = 0; i < H5_WROUNDS; ++i) Ws[wbuf * H5_WSTAGE + tid + 256 * i] = wreg[i];
    };

    f32x16 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // operands of one tap: A 4 m-blocks, B 4 n-blocks
    struct Ops { u32x4 a[4], b[4]; };
    auto load_ops = [&](Ops& o, const u32x4* Ab, const u32x4* Wb, int kx) {
        o.b[0] = Wb[kx * 256];
        o.a[0] = Ab[kx];
        o.b[1] = Wb[kx * 256 + 32];
        o.a[1] = Ab[2 * H5_PX + kx];
#pragma unroll
        for (int ni = 2; ni < 4; ++ni) o.b[ni] = Wb[kx * 256 + ni * 32];
#pragma unroll
        for (int mi = 2; mi < 4; ++mi) o.a[mi] = Ab[mi * 2 * H5_PX + kx];
    };
    auto mfmas = [&](const Ops& o) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = c5_mfma(o.a[mi], o.b[ni], acc[mi][ni]);
    };
    // the next tap's 8 operand fetches go BETWEEN the current tap's 16 MFMAs (2 MFMAs, 1 fetch, ...)
    auto interleave = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);      // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
        }
    };
    // this lane's operand addresses in patch buffer 0 / weight buffer 0 (octet within the K step = k half = lane / 32)
    const u32x4* const a_lane = As + lhi * H5_PR + (wave * 8 + (l31 >> 4)) * H5_PX + pcol;
    const u32x4* const w_lane = Ws + lhi * C5_NT + l31;

    // ---- prologue: chunk 0's patch and the first stage ----
    {
        u32x4 a0[H5_AROUNDS];
#pragma unroll
        for (int j = 0; j < H5_AROUNDS; ++j) a0[j] = issue_a(0, j, true);
        issue_w(0, true);
#pragma unroll
        for (int j = 0; j < H5_AROUNDS; ++j) commit_a(0, j, a0[j]);
        commit_w(0);
    }
    __syncthreads();

    // Granule g = 2 cc + ks reads patch buffer cc % 2, octets 2 ks and 2 ks + 1; its stage s = 5 g + ky reads weight
    // buffer s % 2 = (g + ky) % 2.  The weights of stage s + 1 are requested at its start and written to the other buffer
    // -- last read in stage s - 1, before the previous barrier -- at its end; two of the twelve rounds of the patch of
    // chunk cc + 1 are requested at the start of each of the stages ky 0 .. 2 of both granules of chunk cc and written at
    // its end to the buffer chunk cc does not read: a chunk that has a successor is whole.  ONE loop body for both
    // granules of a chunk (ks only moves addresses): a branch around the second one's stages costs copies of all 256
    // accumulators at its join.
    for (int g = 0; g < K16; ++g) {
        const int cc = g >> 1, ks = g & 1;
        const bool more = cc + 1 < nchunks;
        const u32x4* const Ac = a_lane + (cc & 1) * H5_ABUF + ks * 2 * H5_PR;
        auto stage = [&](const int ky) {
            const int s = g * 5 + ky, wbuf = (g + ky) & 1, j0 = 2 * (3 * ks + ky);
            issue_w(s + 1, s + 1 < nstages);
            u32x4 a0, a1;
            if (ky < 3) {
                a0 = issue_a(cc + 1, j0, more);
                a1 = issue_a(cc + 1, j0 + 1, more);
            }
            __builtin_amdgcn_sched_barrier(0);         // (the requests stay in front of the stage's MFMAs)
            const u32x4* Ab = Ac + ky * H5_PX;
            const u32x4* Wb = w_lane + wbuf * H5_WSTAGE;
            Ops o0, o1;
            load_ops(o0, Ab, Wb, 0);
            load_ops(o1, Ab, Wb, 1);
            mfmas(o0);
            interleave();
            load_ops(o0, Ab, Wb, 2);
            mfmas(o1);
            interleave();
            load_ops(o1, Ab, Wb, 3);
            mfmas(o0);
            interleave();
            load_ops(o0, Ab, Wb, 4);
            mfmas(o1);
            interleave();
            mfmas(o0);
            if (ky < 3) {
                commit_a((cc + 1) & 1, j0, a0);
                commit_a((cc + 1) & 1, j0 + 1, a1);
            }
            commit_w(wbuf ^ 1);
            __syncthreads();
        };
        stage(0);
        stage(1);
        stage(2);
        stage(3);
        stage(4);
    }

    // ---- epilogue: bias, activation, one rounding to half, masked stores ----
    // (the accumulators are read by hand below, and the compiler does not see that those reads wait for the last MFMAs: a
    // v_accvgpr_read of the result of the 8-pass v_mfma_f32_32x32x16_f16 needs 11 wait states behind it, the two s_nop 15
    // give 32.  Another MFMA shape -- 16 passes need 18 -- wants this count looked at again; only the numerical tests guard it.)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15");
    __builtin_amdgcn_sched_barrier(0);
    const long long yelems = (long long)p.N * p.Ho * p.Wo * p.ldy;
    const long long yfirst = (((long long)n * p.Ho + y0) * p.Wo + x0) * p.ldy;
    const rsrc_t ry = c5_rsrc(p.y + yfirst, (yelems - yfirst) * 2);
    float bv[4];
    int ch[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        ch[ni] = ct * C5_NT + ni * 32 + l31;
        bv[ni] = ch[ni] < p.Cout ? p.bias[ch[ni]] : 0.f;
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wave * 8 + mi * 2 + c5_acc_row(r);
            const int col = c5_acc_col(r, lhi);
            const bool ok = y0 + row < p.Ho && x0 + col < p.Wo;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const bool st = ok && ch[ni] < p.ldy;
                const unsigned voff = st ? (unsigned)((row * p.Wo + col) * p.ldy + ch[ni]) * 2u : C5_OOB;
                // (read where it is used: left to the compiler, all 256 accumulators are copied to ordinary registers at
                // the loop's exit and what else is live goes to scratch)
                float v;
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(acc[mi][ni][r]));
                v += bv[ni];
                v = v > 0.f ? v : v * p.slope;
                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (_Float16)v), ry, voff, 0, 0);
            }
        }
    }
}

// ---- weights [cout][cin][5][5] (any strides), fp32 -> half (round to nearest) in stage order, zero-padded ----
// entry (((((ct K16 + k16) 5 + ky) 5 + kx) 2 + khalf) 128 + co holds the 8 values of conv5x5_common.hpp's unit
// (ct, k16, ky, kx, khalf, co): the entries are numbered as the units are
struct Prep5HalfParams {
    Prep5Src src;
    u32x4* wp;
};
__global__ __launch_bounds__(256) void prep5_half_weights_kernel(Prep5HalfParams p) {
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u >= prep5_units(p.src)) return;
    const Prep5Unit t = prep5_unit(p.src, u);
    h8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (_Float16)t.v[i];
    p.wp[u] = __builtin_bit_cast(u32x4, v);
}

// one descriptor spans a tile's patch rows of the input and its tile rows of the output
static bool conv5_half_strides_ok(int w, long long ldx, long long ldy) {
    return c5_strides_ok(H5_PY + 1, w, ldx, H5_TY + 1, w - 4, ldy, 2);
}

static bool conv5_half_dims_ok(int n, int h, int w, int cin, int cout) {
    if (!c5_shape_ok(n, h, w, cin, cout)) return false;
    const long long ldx = c5_pad16(cin), ldy = c5_pad16(cout), ncot = (cout + C5_NT - 1) / C5_NT;
    if (!conv5_half_strides_ok(w, ldx, ldy)) return false;
    const long long tiles = (long long)n * ((h - 4 + H5_TY - 1) / H5_TY) * ((w - 4 + H5_TX - 1) / H5_TX) * ncot;
    return tiles < 0x7FFFFFFFll && ncot * (ldx / 16) * 5 * H5_WSTAGE * 16 < C5_MAXOFF;
}

}  // namespace sbmc

using namespace sbmc;

extern "C" int sbmc_conv5x5_half_supported(int n, int h, int w, int cin, int cout) {
    return conv5_half_dims_ok(n, h, w, cin, cout) ? 1 : 0;
}

extern "C" size_t sbmc_conv5x5_half_weights_bytes(int cin, int cout) {
    if (!conv5_half_dims_ok(1, 5, 5, cin, cout)) return 0;
    return (size_t)((cout + C5_NT - 1) / C5_NT) * (c5_pad16(cin) / 16) * 5 * H5_WSTAGE * 16;
}

extern "C" int sbmc_conv5x5_half_prepare_weights(const float* w, long s_co, long s_ci, long s_ky, long s_kx, int cin,
                                                  int cout, void* wp, void* stream) {
    const size_t bytes = sbmc_conv5x5_half_weights_bytes(cin, cout);
    if (!bytes || !w || !wp || (uintptr_t)wp % 16 || (uintptr_t)w % 4) return SBMC_HIP_EINVAL;
    const Prep5HalfParams p{prep5_src(w, s_co, s_ci, s_ky, s_kx, cin, cout), static_cast<u32x4*>(wp)};
    const long units = prep5_units(p.src);              // (= bytes / 16: one entry a unit)
    hipLaunchKernelGGL(prep5_half_weights_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_half_bias_act_nhwc(const void* x, int ldx, const void* wp, const float* bias, void* y, int ldy,
                                                int n, int h, int w, int cin, int cout, float slope, void* stream) {
    if (!conv5_half_dims_ok(n, h, w, cin, cout) || !x || !wp || !bias || !y) return SBMC_HIP_EINVAL;
    if (!c5_ld_ok(ldx, cin) || !c5_ld_ok(ldy, cout)) return SBMC_HIP_EINVAL;
    if ((uintptr_t)x % 16 || (uintptr_t)wp % 16 || (uintptr_t)y % 16 || (uintptr_t)bias % 4) return SBMC_HIP_EINVAL;
    // (a buffer wider than the rounded channel count: the same 31-bit rule for its strides)
    if (!conv5_half_strides_ok(w, ldx, ldy)) return SBMC_HIP_EINVAL;
    Conv5HalfParams p;
    p.x = static_cast<const _Float16*>(x); p.wp = static_cast<const u32x4*>(wp); p.y = static_cast<_Float16*>(y);
    p.bias = bias;
    p.N = n; p.H = h; p.W = w; p.Ho = h - 4; p.Wo = w - 4; p.ldx = ldx; p.ldy = ldy; p.Cout = cout;
    p.K16 = c5_pad16(cin) / 16;
    p.tiles_x = (p.Wo + H5_TX - 1) / H5_TX; p.tiles_y = (p.Ho + H5_TY - 1) / H5_TY; p.ncot = (cout + C5_NT - 1) / C5_NT;
    p.slope = slope;
    const unsigned grid = (unsigned)((long long)n * p.tiles_y * p.tiles_x * p.ncot);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_half_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)H5_LDS_BYTES);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    hipLaunchKernelGGL(conv5_half_kernel, dim3(grid), dim3(256), H5_LDS_BYTES, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_half_pack_nchw_f32(const float* x, void* y, int ldy, int n, int c, long hw, void* stream) {
    return repack5<float, _Float16, true>(x, static_cast<_Float16*>(y), ldy, n, c, hw, stream);
}

extern "C" int sbmc_conv5x5_half_pack_nchw_f16(const void* x, void* y, int ldy, int n, int c, long hw, void* stream) {
    return repack5<_Float16, _Float16, true>(static_cast<const _Float16*>(x), static_cast<_Float16*>(y), ldy, n, c, hw, stream);
}

extern "C" int sbmc_conv5x5_half_unpack_nhwc(const void* x, int ldx, void* y, int n, int c, long hw, void* stream) {
    return repack5<_Float16, _Float16, false>(static_cast<const _Float16*>(x), static_cast<_Float16*>(y), ldx, n, c, hw, stream);
}
