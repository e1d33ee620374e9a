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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sbmc_hip.h"
#include "common.hpp"
#include "conv5x5_common.hpp"

namespace sbmc {

struct Conv5Params {
    const float* x;          // [N, H, W, ldx]
    const u32x4* wp;         // prepared weights: [cout tile][K16][ky][kx][plane][k half][128] entries of 8 halves
    float* y;                // [N, H - 4, W - 4, ldy]
    const unsigned* xmax;    // bit pattern of max |x|
    const float* wscale;     // the weights' scale
    const float* bias;       // [Cout]
    unsigned* amax;          // raised to the bit pattern of max |y| (a word zeroed by the caller); or nullptr
    int N, H, W, Ho, Wo, ldx, ldy, Cout;
    int K16;                 // chunks of 16 input channels
    int tiles_x, tiles_y, ncot;
    float slope;             // 1: linear, 0: ReLU, else LeakyReLU
};

__global__ __launch_bounds__(256) void conv5_kernel(Conv5Params p) {
    extern __shared__ float4 c5_lds[];
    u32x4* As = reinterpret_cast<u32x4*>(c5_lds);
    u32x4* Ws = As + 2 * C5_ABUF;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_id();
    const int l31 = lane & 31, lhi = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;
    // Row i of a 32 x 32 block is pixel (i / 16, column) of the block's 2 rows x 16 columns.  ds_read_b128 serves lanes
    // {0-3, 12-15, 20-27} (and so on) together: with the patch rows 20 entries apart, the second row's lanes are rotated
    // by 20 mod 16 = 4 columns so that every such group covers 16 different 16-byte slots: lane 16 + j reads column
    // (j + 12) mod 16.
    const int pcol = (l31 + 12 * (l31 >> 4)) & 15;
    const float cx = pow2_scale_of(*p.xmax);
    const float oscale = (1.f / cx) * (1.f / *p.wscale);
    const int nchunks = p.K16;

    // the tile: output-channel tiles of one pixel tile are neighbours in the grid
    unsigned t = blockIdx.x;
    const int ct = (int)(t % (unsigned)p.ncot);
    t /= (unsigned)p.ncot;
    const int x0 = (int)(t % (unsigned)p.tiles_x) * C5_TS;
    t /= (unsigned)p.tiles_x;
    const int y0 = (int)(t % (unsigned)p.tiles_y) * C5_TS;
    const int n = (int)(t / (unsigned)p.tiles_y);

    // ---- staging of a patch chunk: unit u = (pixel u / 2, octet u % 2), 32 contiguous bytes ----
    const long long xelems = (long long)p.N * p.H * p.W * p.ldx;
    const long long xfirst = (((long long)n * p.H + y0) * p.W + x0) * p.ldx;
    const rsrc_t rx = c5_rsrc(p.x + xfirst, (xelems - xfirst) * 4);
    const rsrc_t rnone = c5_rsrc(p.x, 0);
    u32x4 areg[C5_AROUNDS][2];
    unsigned avoff[C5_AROUNDS];
#pragma unroll
    for (int j = 0; j < C5_AROUNDS; ++j) {
        const int u = tid + 256 * j, q = u >> 1, half = u & 1;
        const int qr = q / C5_PS, qc = q - qr * C5_PS;
        const bool in = u < 2 * C5_PP && y0 + qr < p.H && x0 + qc < p.W;
        avoff[j] = in ? (unsigned)((qr * p.W + qc) * p.ldx + half * 8) * 4u : C5_OOB;
    }
    // (valid = false: a request beyond the last chunk -- an empty descriptor, every lane reads zero.  No load of the main
    // loop sits under a branch: at a control-flow join the compiler waits for ALL outstanding loads.)
    auto issue_a = [&](int cc, bool valid) {
        const rsrc_t r = valid ? rx : rnone;
#pragma unroll
        for (int j = 0; j < C5_AROUNDS; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                areg[j][i] = __builtin_amdgcn_raw_buffer_load_b128(r, avoff[j], (unsigned)cc * 64u + 16u * i, 0);
    };
    auto commit_a = [&](int abuf) {
#pragma unroll
        for (int j = 0; j < C5_AROUNDS; ++j) {
            const int u = tid + 256 * j, q = u >> 1, half = u & 1;
            if (u < 2 * C5_PP) {
                u32x4 hh, ll;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned w0 = areg[j][c / 2][(2 * c) % 4];
                    const unsigned w1 = areg[j][c / 2][(2 * c + 1) % 4];
                    unsigned hp, lp;
                    f16_split_pair(__builtin_bit_cast(float, w0), __builtin_bit_cast(float, w1), cx, hp, lp);
                    hh[c] = hp;
                    ll[c] = lp;
                }
                u32x4* d = As + abuf * C5_ABUF + half * C5_PR + q;
                d[0] = hh;
                d[2 * C5_PR] = ll;
            }
        }
    };
    // ---- staging of a weight stage (chunk cc, kernel row ky): 2560 entries, 10 per thread ----
    const long long wentries = (long long)p.ncot * p.K16 * 5 * C5_WSTAGE;
    const rsrc_t rw = c5_rsrc(p.wp, wentries * 16);
    u32x4 wreg[C5_WROUNDS];
    auto issue_w = [&](int cc, int ky, bool valid) {
        const rsrc_t r = valid ? rw : rnone;
        const unsigned block = valid ? (unsigned)((ct * p.K16 + cc) * 5 + ky) : 0u;
#pragma unroll
        for (int i = 0; i < C5_WROUNDS; ++i)
            wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)(tid + 256 * i) * 16u,
                                                            block * (unsigned)(C5_WSTAGE * 16), 0);
    };
    auto commit_w = [&](int wbuf) {
#pragma unroll
        for (int i = 0; i < C5_WROUNDS; ++i) Ws[wbuf * C5_WSTAGE + tid + 256 * i] = wreg[i];
    };

    // Two accumulator sets: hx hw in one, the cross products hx lw + lx hw -- 2^-11 of it and smaller -- in the other,
    // added once in the epilogue.  Every MFMA rounds its accumulator: with all three products in one set the sum of
    // 25 K16 terms is rounded 75 K16 times at its full magnitude, this way 25 K16 times (the cross sums' roundings are
    // 2^-11 of that).  One wave per SIMD owns 512 registers: 256 accumulators fit.
    f32x16 acc[4][2], acx[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = acx[mi][ni][r] = 0.f;

    // operands of one tap: A 4 m-blocks x 2 planes, B 2 n-blocks x 2 planes
    struct Ops { u32x4 ah[4], al[4], bh[2], bl[2]; };
    auto load_ops = [&](Ops& o, const u32x4* Ab, const u32x4* Wb, int kx) {
        o.bh[0] = Wb[kx * 512];
        o.ah[0] = Ab[kx];
        o.bh[1] = Wb[kx * 512 + 32];
#pragma unroll
        for (int mi = 1; mi < 4; ++mi) o.ah[mi] = Ab[mi * 2 * C5_PS + kx];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) o.bl[ni] = Wb[kx * 512 + 256 + ni * 32];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) o.al[mi] = Ab[2 * C5_PR + mi * 2 * C5_PS + kx];
    };
    auto mfmas = [&](const Ops& o) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = c5_mfma(o.ah[mi], o.bh[ni], acc[mi][ni]);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acx[mi][ni] = c5_mfma(o.ah[mi], o.bl[ni], acx[mi][ni]);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acx[mi][ni] = c5_mfma(o.al[mi], o.bh[ni], acx[mi][ni]);
    };
    // the next tap's 12 operand fetches go BETWEEN the current tap's 24 MFMAs (2 MFMAs, 1 fetch, ...)
    auto interleave = [&]() {
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);      // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
        }
    };
    // this lane's operand addresses in patch buffer 0 / weight buffer 0 (octet = k half = lane / 32)
    const u32x4* const a_lane = As + lhi * C5_PR + (mh * 8 + (l31 >> 4)) * C5_PS + pcol;
    const u32x4* const w_lane = Ws + lhi * C5_NT + nh * 64 + l31;

    // ---- prologue: chunk 0's patch and its first stage ----
    issue_a(0, true);
    issue_w(0, 0, true);
    commit_a(0);
    commit_w(0);
    __syncthreads();

    // Stage s = 5 cc + ky reads patch buffer cc % 2 and weight buffer s % 2.  The weights of stage s + 1 are requested
    // at its start and written to buffer (s + 1) % 2 -- last read in stage s - 1, before the previous barrier -- at its
    // end; the patch of chunk cc + 1 is requested at the start of stage ky = 3 and written at the end of stage ky = 4.
    for (int cc = 0; cc < nchunks; ++cc) {
        const bool more = cc + 1 < nchunks;
        const u32x4* const Ac = a_lane + (cc & 1) * C5_ABUF;
        auto stage = [&](const int ky) {
            const int s = cc * 5 + ky;
            if (ky < 4) issue_w(cc, ky + 1, true);
            else issue_w(cc + 1, 0, more);
            if (ky == 3) issue_a(cc + 1, more);
            const u32x4* Ab = Ac + ky * C5_PS;
            const u32x4* Wb = w_lane + (s & 1) * C5_WSTAGE;
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
            if (ky == 4) commit_a((cc + 1) & 1);
            commit_w((s + 1) & 1);
            __syncthreads();
        };
        stage(0);
        stage(1);
        stage(2);
        stage(3);
        stage(4);
    }

    // ---- epilogue: scale back, bias, activation, largest magnitude, masked stores ----
    const long long yelems = (long long)p.N * p.Ho * p.Wo * p.ldy;
    const long long yfirst = (((long long)n * p.Ho + y0) * p.Wo + x0) * p.ldy;
    const rsrc_t ry = c5_rsrc(p.y + yfirst, (yelems - yfirst) * 4);
    float bv[2];
    int ch[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        ch[ni] = ct * C5_NT + nh * 64 + ni * 32 + l31;
        bv[ni] = ch[ni] < p.Cout ? p.bias[ch[ni]] : 0.f;
    }
    unsigned amax_run = 0;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // accumulator register r of a 32 x 32 block: row (r & 3) + 8 (r >> 2) + 4 (lane / 32) of the block = pixel
            // (r >> 3, rotated column) of its 2 rows x 16 columns; output channel lane % 32
            const int row = mh * 8 + mi * 2 + (r >> 3);
            const int col = ((r & 3) + 8 * ((r >> 2) & 1) + 4 * lhi + 12 * (r >> 3)) & 15;
            const bool ok = y0 + row < p.Ho && x0 + col < p.Wo;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const bool st = ok && ch[ni] < p.ldy;
                const unsigned voff = st ? (unsigned)((row * p.Wo + col) * p.ldy + ch[ni]) * 4u : C5_OOB;
                float v = (acc[mi][ni][r] + acx[mi][ni][r]) * oscale + bv[ni];
                v = v > 0.f ? v : v * p.slope;
                if (st) {
                    const unsigned a = abits(v);
                    amax_run = amax_run > a ? amax_run : a;
                }
                buf_store(v, ry, voff, 0);
            }
        }
    }
    if (p.amax) amax_publish(amax_run, p.amax);          // (wave-uniform condition; a barrier inside)
}

// ---- weights [cout][cin][5][5] (any strides) -> the two f16 planes in stage order, zero-padded ----
// entry ((((ct K16 + k16) 5 + ky) 5 + kx) 2 + plane) 2 + khalf) 128 + co holds input channels 16 k16 + 8 khalf .. + 7
// of output channel 128 ct + co at tap (ky, kx); channels beyond cin / cout: zeros
struct Prep5Params {
    const float* w;
    long s_co, s_ci, s_ky, s_kx;
    int cout, cin, K16, ncot;
    const unsigned* wmax;
    u32x4* wp;
    float* wscale;
};
__global__ __launch_bounds__(256) void prep5_weights_kernel(Prep5Params p) {
    const float c = pow2_scale_of(*p.wmax);
    const long units = (long)p.ncot * p.K16 * 25 * 2 * C5_NT;
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u == 0) *p.wscale = c;
    if (u >= units) return;
    const int co = (int)(u % C5_NT);
    long r = u / C5_NT;
    const int khalf = (int)(r % 2);
    r /= 2;
    const int kx = (int)(r % 5);
    r /= 5;
    const int ky = (int)(r % 5);
    r /= 5;
    const int k16 = (int)(r % p.K16), ct = (int)(r / p.K16);
    const int oc = ct * C5_NT + co, ic0 = k16 * 16 + khalf * 8;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = (oc < p.cout && ic0 + i < p.cin) ? p.w[(long)oc * p.s_co + (long)(ic0 + i) * p.s_ci + ky * p.s_ky + kx * p.s_kx] : 0.f;
    u32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned hp, lp;
        f16_split_pair(v[2 * i], v[2 * i + 1], c, hp, lp);
        h[i] = hp;
        l[i] = lp;
    }
    const long base = ((((long)(ct * p.K16 + k16) * 5 + ky) * 5 + kx) * 2) * 2 * C5_NT + khalf * C5_NT + co;
    p.wp[base] = h;
    p.wp[base + 2 * C5_NT] = l;
}

// ---- planar [n][c][hw] <-> channels-last [n][hw][ld] with zeros in the channels from c up: tiles of 64 pixels x 32
// channels through LDS, 256-byte rows on the planar side, 128-byte rows on the other ----
template <bool TO_NHWC>
__global__ __launch_bounds__(256) void repack5_kernel(const float* __restrict__ src, float* __restrict__ dst, int c, int ld,
                                                      long hw, int ctiles, long ptiles) {
    __shared__ float tile[32][65];
    long b = blockIdx.x;
    const int cti = (int)(b % ctiles);
    b /= ctiles;
    const long pt = b % ptiles;
    const long n = b / ptiles;
    const long p0 = pt * 64;
    const int c0 = cti * 32;
    const int tid = (int)threadIdx.x;
    const float* planar = (TO_NHWC ? src : dst) + n * (long)c * hw;
    const float* nhwc = (TO_NHWC ? dst : src) + n * hw * ld;
    if (TO_NHWC) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cl = (tid >> 6) + 4 * i, px = tid & 63;
            tile[cl][px] = (c0 + cl < c && p0 + px < hw) ? planar[(long)(c0 + cl) * hw + p0 + px] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int px = (tid >> 5) + 8 * i, cl = tid & 31;
            if (p0 + px < hw && c0 + cl < ld) const_cast<float*>(nhwc)[(p0 + px) * ld + c0 + cl] = tile[cl][px];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int px = (tid >> 5) + 8 * i, cl = tid & 31;
            tile[cl][px] = (p0 + px < hw && c0 + cl < c) ? nhwc[(p0 + px) * ld + c0 + cl] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cl = (tid >> 6) + 4 * i, px = tid & 63;
            if (c0 + cl < c && p0 + px < hw) const_cast<float*>(planar)[(long)(c0 + cl) * hw + p0 + px] = tile[cl][px];
        }
    }
}

static bool conv5_dims_ok(int n, int h, int w, int cin, int cout) {
    if (n < 1 || h < 5 || w < 5 || cin < 1 || cout < 1 || cin > (1 << 20) || cout > (1 << 20)) return false;
    const long long ldx = c5_pad16(cin), ldy = c5_pad16(cout), ncot = (cout + C5_NT - 1) / C5_NT;
    // byte offsets inside one tile's rows stay below 2^31 (patch rows of the input, tile rows of the output)
    if ((long long)(C5_PS + 1) * w * ldx * 4 >= C5_MAXOFF || (long long)(C5_TS + 1) * (w - 4) * ldy * 4 >= C5_MAXOFF) return false;
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
    Prep5Params p;
    p.w = w; p.s_co = s_co; p.s_ci = s_ci; p.s_ky = s_ky; p.s_kx = s_kx;
    p.cout = cout; p.cin = cin; p.K16 = c5_pad16(cin) / 16; p.ncot = (cout + C5_NT - 1) / C5_NT;
    p.wmax = wmax; p.wp = static_cast<u32x4*>(wp); p.wscale = wscale;
    const long units = (long)p.ncot * p.K16 * 25 * 2 * C5_NT;
    hipLaunchKernelGGL(prep5_weights_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_bias_act_nhwc_f32(const float* x, int ldx, const unsigned* xmax, const void* wp,
                                               const float* bias, float* y, int ldy, int n, int h, int w, int cin,
                                               int cout, float slope, unsigned* amax, void* stream) {
    if (!conv5_dims_ok(n, h, w, cin, cout) || !x || !xmax || !wp || !bias || !y) return SBMC_HIP_EINVAL;
    if (ldx < cin || ldy < cout || ldx % 16 || ldy % 16 || ldx > (1 << 20) || ldy > (1 << 20)) return SBMC_HIP_EINVAL;
    if ((uintptr_t)x % 16 || (uintptr_t)wp % 16 || (uintptr_t)y % 16 || (uintptr_t)bias % 4 || (uintptr_t)xmax % 4 ||
        (uintptr_t)amax % 4)
        return SBMC_HIP_EINVAL;
    // (a buffer wider than the rounded channel count: the same 31-bit rule for its strides)
    if ((long long)(C5_PS + 1) * w * ldx * 4 >= C5_MAXOFF || (long long)(C5_TS + 1) * (w - 4) * ldy * 4 >= C5_MAXOFF)
        return SBMC_HIP_EINVAL;
    Conv5Params p;
    p.x = x; p.wp = static_cast<const u32x4*>(wp); p.y = y; p.xmax = xmax;
    p.wscale = reinterpret_cast<const float*>(static_cast<const char*>(wp) + sbmc_conv5x5_weights_bytes(cin, cout) - 16);
    p.bias = bias; p.amax = amax;
    p.N = n; p.H = h; p.W = w; p.Ho = h - 4; p.Wo = w - 4; p.ldx = ldx; p.ldy = ldy; p.Cout = cout;
    p.K16 = c5_pad16(cin) / 16;
    p.tiles_x = (p.Wo + C5_TS - 1) / C5_TS; p.tiles_y = (p.Ho + C5_TS - 1) / C5_TS; p.ncot = (cout + C5_NT - 1) / C5_NT;
    p.slope = slope;
    const unsigned grid = (unsigned)((long long)n * p.tiles_y * p.tiles_x * p.ncot);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)C5_LDS_BYTES);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    hipLaunchKernelGGL(conv5_kernel, dim3(grid), dim3(256), C5_LDS_BYTES, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

static int repack5(bool to_nhwc, const float* src, float* dst, int ld, int n, int c, long hw, void* stream) {
    if (n < 0 || c < 1 || hw < 0 || ld < c || ld % 16 || ld > (1 << 20)) return SBMC_HIP_EINVAL;
    if (n == 0 || hw == 0) return 0;
    if (!src || !dst || (uintptr_t)src % 4 || (uintptr_t)dst % 4) return SBMC_HIP_EINVAL;
    // (the channels-last side is covered up to ld: the packing writes its zeros)
    const int ctiles = ((to_nhwc ? ld : c) + 31) / 32;
    const long ptiles = (hw + 63) / 64;
    const long long blocks = (long long)n * ptiles * ctiles;
    if (blocks >= 0x7FFFFFFFll) return SBMC_HIP_EINVAL;
    if (to_nhwc)
        hipLaunchKernelGGL(repack5_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, c, ld, hw, ctiles, ptiles);
    else
        hipLaunchKernelGGL(repack5_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, c, ld, hw, ctiles, ptiles);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_pack_nchw_f32(const float* x, float* y, int ldy, int n, int c, long hw, void* stream) {
    return repack5(true, x, y, ldy, n, c, hw, stream);
}

extern "C" int sbmc_conv5x5_unpack_nhwc_f32(const float* x, int ldx, float* y, int n, int c, long hw, void* stream) {
    return repack5(false, x, y, ldx, n, c, hw, stream);
}
