// The gradients of csrc/conv5x5.hip's 5 x 5 valid convolution -- `torch.nn.Conv2d(..., 5)`'s backward in KPCN's two chains
// (reference sbmc/models.py:221-291) -- on the forward's buffers (channels-last fp32 [n][h][w][ld], ld the channel count
// rounded up to 16, EXACT ZEROS in the padding channels), scales (magnitude words -> pow2_scale_of) and arithmetic
// (f16_split_pair, three f16 products per term on v_mfma_f32_32x32x16_f16, fp32 accumulation).
//
// (a) DATA GRADIENT with the producing layer's activation adjoint (conv5_dgrad_kernel):
//       gx[n,y,x,ci] = act'(xsaved[n,y,x,ci]) sum_{ky,kx,co} gz[n,y-ky,x-kx,co] w[co,ci,ky,kx]
//     is the forward's implicit GEMM over gz padded by 4 zeros each way, with the channel sides exchanged and the taps
//     mirrored.  The plan is the forward's to the letter, and so is the code: conv5_dgrad_kernel is csrc/
//     conv5x5_gemm_body.inc (16 x 16 pixels x 128 channels per workgroup, a 20 x 20 patch per 16-channel chunk as two f16
//     planes, 40 KB weight stages in two buffers, one barrier per stage, acc / acx, operand fetches between the MFMAs) with
//     `Side::mirror` set; the weights are sbmc_conv5x5_prepare_weights_f32's with strides and counts exchanged,
//     and the mirror is the body's: stage j reads prepared kernel row 4 - j, tap i column 4 - i.  This Side's own:
//       * the patch origin (y0 - 4, x0 - 4) in gz coordinates lies above / left of the tensor for border tiles, and a
//         row-major offset past a row's end lands in the next row, not in zeros: every patch pixel carries an in-range
//         predicate on BOTH sides of both coordinates (the out-of-range sentinel offset otherwise); the descriptor's base
//         is the first patch row that exists (a non-negative row of the image), byte offsets from it below 2^31;
//       * the epilogue scales back, multiplies by act' read from the saved activation at the output pixel (v > 0 ? 1 :
//         slope; a null xsaved: nothing to undo), raises *amax to max |gx| (the next layer down scales by it) and stores
//         masked.  A padding channel has zero weights: it is written as 0.
//
// (b) WEIGHT AND BIAS GRADIENT (conv5_wgrad_kernel + conv5_wgrad_reduce_kernel):
//       gw[co][ci][ky][kx] = sum_{n,y,x} gz[n,y,x,co] x[n,y+ky,x+kx,ci],   gb[co] = sum gz
//     The reduction runs over pixels, so the staging transposes: the MFMA's k index is 8 consecutive pixels of one channel.
//       * a workgroup owns one tap column kx (the shift is folded into its x addresses: pixel octets stay aligned), all
//         five ky, 128 output x 64 input channels and a contiguous RANGE of row stages; a row stage is 32 pixels of one
//         gz row, walked down a 32-pixel column strip, strip after strip, image after image;
//       * LDS: a ring of six x rows ([plane][pixel octet][channel] 16-byte entries, 8 KB a row) -- each row is fetched
//         once and serves five gz rows; the sixth slot takes the next row while five are read -- and two gz stages of
//         16 KB: 80 KB, two workgroups per CU.  The next stage's rows are in flight in registers during a stage's MFMAs
//         and written behind them: one barrier per stage.  A new strip (or range) fetches its first five x rows under a
//         branch of its own: once per strip height;
//       * staging: a thread owns 4 pixels x 4 channels (four 16-byte loads), splits them and writes 8-byte halves of
//         entries.  Channel 4 q + c of a tile is kept at slot 32 c + q (16 c + q on the x side): the 32 lanes of a write
//         fall on 32 different 8-byte slots, a wave's operand read on consecutive entries -- no bank conflict either
//         way; an accumulator row only means another channel (undone by the reduction kernel);
//       * a wave (two per SIMD: one of each resident workgroup) holds 64 x 32 channels x 5 taps = 10 accumulators of 32 x 32 (160 registers); 60 MFMAs
//         per stage;
//       * the ranges' partial sums go to the caller's scratch and a second kernel adds them in a fixed order (no float
//         atomics: the result does not depend on the run), scales back by both tensors' scales and writes co < cout,
//         ci < cin through the [co][ci][ky][kx] strides.  The bias partials ride along: the workgroups of kx = 0 and
//         input tile 0 sum the gz values they stage, in fp32;
//       * the number of ranges is one rule (w5_splits): two workgroups per compute unit (what LDS and registers allow)
//         over the (kx, channel tile) combinations, at least four stages a range.
//     Where this differs from the forward, and why: ONE accumulator set takes all three products.  A second set for the
//     cross products (the forward's acx) makes 320 accumulator registers, of which 64 do not fit the 256 AGPRs: the compiler
//     then spilled 22 registers (92 bytes of scratch per lane) inside the MFMA stream, and 120 with the two k steps fenced
//     apart.  A range's sum is a few thousand MFMA accumulations long, against the forward's 25 K16 <= 700 with far larger
//     terms relative to the result: the extra roundings stay below the bound of tests/test_gpu_conv5x5_grad.py.  The
//     operand fetches are left to the compiler's scheduler: 14 LDS reads per 30 MFMAs.
//
// build.EXTRA_FLAGS: the same as conv5x5.hip's (no packed fp32 arithmetic): the dgrad epilogue is the forward's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sbmc_hip.h"
#include "common.hpp"
#include "conv5x5_common.hpp"

namespace sbmc {

using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

// =====================================================================================================================
// (a) data gradient
// The data-gradient Side of the shared body: A = gz [N, H - 4, W - 4, ldg], Y = gx [N, H, W, ldx],
// aux = the producing layer's activated output (this layer's input, Y's shape) or nullptr, the prepared weights with the
// channel sides exchanged.  Patch pixel (qr, qc) is gz pixel (y0 - 4 + qr, x0 - 4 + qc), checked on both sides of both
// coordinates; the descriptor's base is the first patch row that exists (y0 <= H - 1: it is a row of gz).  Stage j reads
// prepared kernel row 4 - j, tap i column 4 - i: the mirror.
__global__ __launch_bounds__(256) void conv5_dgrad_kernel(Conv5Params p) {
    using Side = Conv5Dgrad;
#include "conv5x5_gemm_body.inc"
}

// ---- g *= act'(ysaved), elementwise over a whole padded buffer, and the largest magnitude of the result: the adjoint of
// a chain's LAST activation, which no data-gradient epilogue applies ----
__global__ __launch_bounds__(256) void conv5_act_adjoint_kernel(float4* __restrict__ g, const float4* __restrict__ ysaved,
                                                                float slope, long n4, unsigned* amax) {
    unsigned m = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 v = g[i];
        const float4 s = ysaved[i];
        v.x = s.x > 0.f ? v.x : v.x * slope;
        v.y = s.y > 0.f ? v.y : v.y * slope;
        v.z = s.z > 0.f ? v.z : v.z * slope;
        v.w = s.w > 0.f ? v.w : v.w * slope;
        g[i] = v;
        m = amax4(m, v);
    }
    amax_publish(m, amax);
}

// =====================================================================================================================
// (b) weight and bias gradient
constexpr int W5_PX = 32;                       // pixels of a row stage
constexpr int W5_MT = 128, W5_NT = 64;          // output / input channels of a workgroup
constexpr int W5_GBUF = 2 * 4 * W5_MT;          // 16-byte entries of a gz stage: [plane 2][pixel octet 4][slot 128]
constexpr int W5_XROW = 2 * 4 * W5_NT;          // ... of an x row: [plane 2][pixel octet 4][slot 64]
constexpr int W5_RING = 6;                      // x rows in LDS: five in use, one being written
constexpr unsigned W5_LDS_BYTES = (2 * W5_GBUF + W5_RING * W5_XROW) * 16;       // 81920
constexpr int W5_TILE = 5 * W5_MT * W5_NT;      // floats of a workgroup's partial sums: [ky 5][co row 128][ci slot 64]
constexpr int W5_MIN_STAGES = 4;                // row stages of a range at least

struct Wgrad5Params {
    const float* gz;         // [N, H - 4, W - 4, ldg]
    const float* x;          // [N, H, W, ldx]
    float* partial;          // [nsplit][ncombo][W5_TILE]
    float* bpartial;         // [nsplit][ncot][128]
    const unsigned* gmax;
    const unsigned* xmax;
    int N, H, W, Ho, Wo, ldg, ldx;
    int nstrips, ncot, ncit, nsplit;
    long long total;         // row stages: N nstrips Ho
};

__global__ __launch_bounds__(256) void conv5_wgrad_kernel(Wgrad5Params p) {
    extern __shared__ float4 w5_lds[];
    u32x4* Gs = reinterpret_cast<u32x4*>(w5_lds);
    u32x4* Xs = Gs + 2 * W5_GBUF;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_id();
    const int l31 = lane & 31, lhi = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;
    const float cg = pow2_scale_of(*p.gmax);
    const float cx = pow2_scale_of(*p.xmax);

    // the workgroup: (range, output tile, input tile, tap column), the tap columns of a tile next to each other
    unsigned t = blockIdx.x;
    const int kx = (int)(t % 5u);
    t /= 5u;
    const int cit = (int)(t % (unsigned)p.ncit);
    t /= (unsigned)p.ncit;
    const int ct = (int)(t % (unsigned)p.ncot);
    const int split = (int)(t / (unsigned)p.ncot);
    const long long s_begin = p.total * split / p.nsplit, s_end = p.total * (split + 1) / p.nsplit;

    // ---- staging roles: 4 pixels (pixel quad 2 octet + h of the stage) x 4 channels (quad cq of the tile) ----
    const int gh = tid & 1, gcq = (tid >> 1) & 31, goct = tid >> 6;
    const int gch = ct * W5_MT + 4 * gcq;
    const bool gchok = gch < p.ldg;
    const int xh = tid & 1, xcq = (tid >> 1) & 15, xoct = (tid >> 5) & 3;
    const int xch = cit * W5_NT + 4 * xcq;
    const bool xrole = tid < 128;                          // (waves 0 and 1)
    const bool xchok = xrole && xch < p.ldx;
    const rsrc_t rnone = c5_rsrc(p.gz, 0);
    u32x4 greg[4], xreg[4];
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};

    // one gz row / x row per descriptor: every offset is checked against the row's end; a pixel beyond the row and a
    // channel beyond the buffer's stride carry the sentinel (a channel offset past ld would land in the next pixel)
    auto issue_g = [&](int n, int y, int xs, bool valid) {
        const float* row = p.gz + (((long long)n * p.Ho + y) * p.Wo) * p.ldg;
        const rsrc_t r = valid ? c5_rsrc(row, (long long)p.Wo * p.ldg * 4) : rnone;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int px = xs + 4 * (2 * goct + gh) + q;
            const unsigned voff = (px < p.Wo && gchok) ? (unsigned)(px * p.ldg + gch) * 4u : C5_OOB;
            greg[q] = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
        }
    };
    auto issue_x = [&](int n, int yr, int xs, bool valid) {
        const float* row = p.x + (((long long)n * p.H + yr) * p.W) * p.ldx;
        const rsrc_t r = valid ? c5_rsrc(row, (long long)p.W * p.ldx * 4) : rnone;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int px = xs + kx + 4 * (2 * xoct + xh) + q;
            const unsigned voff = (px < p.W && xchok) ? (unsigned)(px * p.ldx + xch) * 4u : C5_OOB;
            xreg[q] = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
        }
    };
    auto comp = [](const u32x4& v, int c) { return __builtin_bit_cast(float, c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w))); };
    // channel c of the quad: the four pixels as two f16 pairs per plane = half an entry (8 bytes)
    auto split4 = [&](const u32x4 (&reg)[4], int c, float scale, u32x2& hh, u32x2& ll) {
        unsigned h0, l0, h1, l1;
        f16_split_pair(comp(reg[0], c), comp(reg[1], c), scale, h0, l0);
        f16_split_pair(comp(reg[2], c), comp(reg[3], c), scale, h1, l1);
        hh[0] = h0; hh[1] = h1;
        ll[0] = l0; ll[1] = l1;
    };
    auto commit_g = [&](int buf) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u32x2 hh, ll;
            split4(greg, c, cg, hh, ll);
            u32x2* d = reinterpret_cast<u32x2*>(Gs + buf * W5_GBUF + goct * W5_MT + c * 32 + gcq) + gh;
            d[0] = hh;
            d[2 * 4 * W5_MT] = ll;                          // (plane 1: 4 W5_MT entries = 8 W5_MT halves on)
            bsum[c] += (comp(greg[0], c) + comp(greg[1], c)) + (comp(greg[2], c) + comp(greg[3], c));
        }
    };
    auto commit_x = [&](int slot) {
        if (xrole) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                u32x2 hh, ll;
                split4(xreg, c, cx, hh, ll);
                u32x2* d = reinterpret_cast<u32x2*>(Xs + slot * W5_XROW + xoct * W5_NT + c * 16 + xcq) + xh;
                d[0] = hh;
                d[2 * 4 * W5_NT] = ll;
            }
        }
    };
    // the five x rows of a strip's (or a range's) first stage: rows y .. y + 4 into their ring slots, one after the other
    // through the registers of the row in flight (none is, then)
    auto fill = [&](int n, int y, int xs) {
        for (int j = 0; j < 5; ++j) {
            issue_x(n, y + j, xs, true);
            commit_x((y + j) % W5_RING);
        }
    };

    f32x16 acc[5][2];
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ky][mi][r] = 0.f;

    const u32x4* const g_lane = Gs + lhi * W5_MT + mh * 64 + l31;
    const u32x4* const x_lane = Xs + lhi * W5_NT + nh * 32 + l31;
    // a stage's products: gz row y (buffer buf) against x rows y .. y + 4 (ring slots (y + ky) % 6); two k steps of 16 pixels
    auto products = [&](int buf, int y6) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 ah[2], al[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                ah[mi] = g_lane[buf * W5_GBUF + ks * 2 * W5_MT + mi * 32];
                al[mi] = g_lane[buf * W5_GBUF + 4 * W5_MT + ks * 2 * W5_MT + mi * 32];
            }
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                const int slot = y6 + ky >= W5_RING ? y6 + ky - W5_RING : y6 + ky;
                const u32x4 bh = x_lane[slot * W5_XROW + ks * 2 * W5_NT];
                const u32x4 bl = x_lane[slot * W5_XROW + 4 * W5_NT + ks * 2 * W5_NT];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    acc[ky][mi] = c5_mfma(ah[mi], bh, acc[ky][mi]);
                    acc[ky][mi] = c5_mfma(ah[mi], bl, acc[ky][mi]);
                    acc[ky][mi] = c5_mfma(al[mi], bh, acc[ky][mi]);
                }
            }
        }
    };

    // ---- the range's first stage ----
    int y = (int)(s_begin % p.Ho);
    long long rest = s_begin / p.Ho;
    int strip = (int)(rest % p.nstrips);
    int n = (int)(rest / p.nstrips);
    issue_g(n, y, strip * W5_PX, true);
    fill(n, y, strip * W5_PX);
    commit_g(0);
    __syncthreads();

    // Stage s reads gz buffer s % 2 and five ring slots.  The rows of stage s + 1 are requested at its start and written at
    // its end: the gz row into the other buffer (last read in stage s - 1, before the previous barrier), x row y + 5 into
    // the sixth slot (the same).  A stage that opens a new strip needs five new x rows in slots that are in use: it
    // requests none ahead (an empty descriptor, not a branch) and fills them behind a barrier of its own.
    int buf = 0, y6 = y % W5_RING;
    for (long long s = s_begin; s < s_end; ++s) {
        int ny = y + 1, nstrip = strip, nn = n;
        if (ny == p.Ho) {
            ny = 0;
            if (++nstrip == p.nstrips) { nstrip = 0; ++nn; }
        }
        const bool more = s + 1 < s_end;
        issue_g(nn, ny, nstrip * W5_PX, more);
        issue_x(nn, ny + 4, nstrip * W5_PX, more && ny != 0);
        products(buf, y6);
        if (more) {
            if (ny == 0) {
                __syncthreads();
                fill(nn, 0, nstrip * W5_PX);
            } else {
                commit_x((ny + 4) % W5_RING);
            }
            commit_g(buf ^ 1);
        }
        __syncthreads();
        buf ^= 1;
        y = ny; strip = nstrip; n = nn;
        y6 = ny == 0 ? 0 : (y6 + 1 == W5_RING ? 0 : y6 + 1);
    }

    // ---- the partial sums: [ky][co row][ci slot], a wave's 32 lanes on 128 consecutive bytes ----
    float* tile = p.partial + (size_t)blockIdx.x * W5_TILE;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int corow = (mh * 2 + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                tile[(ky * W5_MT + corow) * W5_NT + nh * 32 + l31] = acc[ky][mi][r];
            }
    // ---- the bias partials: eight threads hold sums of a channel quad (the last barrier is behind every LDS read) ----
    if (kx == 0 && cit == 0) {
        float* red = reinterpret_cast<float*>(Gs);
#pragma unroll
        for (int c = 0; c < 4; ++c) red[(goct * 2 + gh) * W5_MT + 4 * gcq + c] = bsum[c];
        __syncthreads();
        if (tid < W5_MT) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += red[j * W5_MT + tid];
            p.bpartial[((size_t)split * p.ncot + ct) * W5_MT + tid] = s;
        }
    }
}

struct Wreduce5Params {
    const float* partial;
    const float* bpartial;
    float* gw;
    float* gb;
    long s_co, s_ci, s_ky, s_kx;
    const unsigned* gmax;
    const unsigned* xmax;
    int cin, cout, ncot, ncit, nsplit, ncombo;
};

// blockIdx.y < ncombo: element blockIdx.x 256 + thread of combination (ct, cit, kx)'s tile, summed over the ranges in
// their order; blockIdx.y == ncombo: the bias gradient
__global__ __launch_bounds__(256) void conv5_wgrad_reduce_kernel(Wreduce5Params p) {
    const int combo = (int)blockIdx.y;
    if (combo == p.ncombo) {
        for (int co = (int)(blockIdx.x * 256 + threadIdx.x); co < p.cout; co += (int)gridDim.x * 256) {
            float s = 0.f;
            for (int k = 0; k < p.nsplit; ++k) s += p.bpartial[((size_t)k * p.ncot + co / W5_MT) * W5_MT + co % W5_MT];
            p.gb[co] = s;
        }
        return;
    }
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    float s = 0.f;
    for (int k = 0; k < p.nsplit; ++k) s += p.partial[((size_t)k * p.ncombo + combo) * W5_TILE + e];
    const int kx = combo % 5, cit = (combo / 5) % p.ncit, ct = combo / (5 * p.ncit);
    const int cislot = e % W5_NT, corow = (e / W5_NT) % W5_MT, ky = e / (W5_NT * W5_MT);
    // slot -> channel: the staging keeps channel 4 q + c at slot 32 c + q (gz) / 16 c + q (x)
    const int co = ct * W5_MT + 4 * (corow % 32) + corow / 32;
    const int ci = cit * W5_NT + 4 * (cislot % 16) + cislot / 16;
    if (co < p.cout && ci < p.cin) {
        const float oscale = (1.f / pow2_scale_of(*p.gmax)) * (1.f / pow2_scale_of(*p.xmax));
        p.gw[co * p.s_co + ci * p.s_ci + ky * p.s_ky + kx * p.s_kx] = s * oscale;
    }
}

static int w5_cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1) {
        (void)hipGetLastError();
        return 256;
    }
    return cus;
}

// one descriptor spans the patch rows of gz from a tile's first existing one, another a tile's rows of gx / xsaved
static bool dgrad5_strides_ok(int w, long long ldg, long long ldx) {
    return c5_strides_ok(C5_PS + 1, w - 4, ldg, C5_TS + 1, w, ldx, 4);
}
// ... one row of x, another one row of gz
static bool wgrad5_strides_ok(int w, long long ldg, long long ldx) { return c5_strides_ok(1, w, ldx, 1, w - 4, ldg, 4); }

static bool dgrad5_dims_ok(int n, int h, int w, int cin, int cout) {
    if (!c5_shape_ok(n, h, w, cin, cout)) return false;
    const long long ldx = c5_pad16(cin), ldg = c5_pad16(cout), ncit = (cin + C5_NT - 1) / C5_NT;
    if (!dgrad5_strides_ok(w, ldg, ldx)) return false;
    const long long tiles = (long long)n * ((h + C5_TS - 1) / C5_TS) * ((w + C5_TS - 1) / C5_TS) * ncit;
    return tiles < 0x7FFFFFFFll && ncit * (ldg / 16) * 5 * C5_WSTAGE * 16 < C5_MAXOFF;
}

static bool wgrad5_dims_ok(int n, int h, int w, int cin, int cout) {
    if (!c5_shape_ok(n, h, w, cin, cout) || !wgrad5_strides_ok(w, c5_pad16(cout), c5_pad16(cin))) return false;
    const long long ncombo = (long long)((cout + W5_MT - 1) / W5_MT) * ((cin + W5_NT - 1) / W5_NT) * 5;
    return ncombo < 65535;
}

// ranges of row stages: two workgroups per compute unit (80 KB of LDS and 248 registers each) over the (tap column, channel
// tile) combinations, W5_MIN_STAGES stages at least
static int w5_splits(int n, int h, int w, int cin, int cout) {
    const long long total = (long long)n * (h - 4) * ((w - 4 + W5_PX - 1) / W5_PX);
    const int ncombo = ((cout + W5_MT - 1) / W5_MT) * ((cin + W5_NT - 1) / W5_NT) * 5;
    long long s = 2 * w5_cu_count() / ncombo;
    if (s > total / W5_MIN_STAGES) s = total / W5_MIN_STAGES;
    return (int)(s < 1 ? 1 : s);
}

}  // namespace sbmc

using namespace sbmc;

extern "C" int sbmc_conv5x5_dgrad_supported(int n, int h, int w, int cin, int cout) {
    return dgrad5_dims_ok(n, h, w, cin, cout) ? 1 : 0;
}

extern "C" int sbmc_conv5x5_dgrad_adj_nhwc_f32(const float* gz, int ldg, const unsigned* gmax, const void* wp_swapped,
                                                const float* xsaved, float slope, float* gx, int ldx, int n, int h, int w,
                                                int cin, int cout, unsigned* amax, void* stream) {
    if (!dgrad5_dims_ok(n, h, w, cin, cout) || !gz || !gmax || !wp_swapped || !gx) return SBMC_HIP_EINVAL;
    if (!c5_ld_ok(ldx, cin) || !c5_ld_ok(ldg, cout)) return SBMC_HIP_EINVAL;
    if ((uintptr_t)gz % 16 || (uintptr_t)wp_swapped % 16 || (uintptr_t)gx % 16 || (uintptr_t)xsaved % 16 || (uintptr_t)gmax % 4 ||
        (uintptr_t)amax % 4)
        return SBMC_HIP_EINVAL;
    if (!dgrad5_strides_ok(w, ldg, ldx)) return SBMC_HIP_EINVAL;
    Conv5Params p;
    // (this Side's aux: the saved activation, a whole tensor of gx's shape, or nullptr)
    p.a = gz; p.wp = static_cast<const u32x4*>(wp_swapped); p.aux = xsaved; p.y = gx; p.amag = gmax;
    // (the weights were prepared with the sides exchanged: cout is their reduction side)
    p.wscale = reinterpret_cast<const float*>(static_cast<const char*>(wp_swapped) + sbmc_conv5x5_weights_bytes(cout, cin) - 16);
    p.amax = amax;
    p.N = n; p.Hy = h; p.Wy = w; p.Ha = h - 4; p.Wa = w - 4; p.lda = ldg; p.ldy = ldx; p.Cout = 0;      // (no bias: Cout unused)
    p.K16 = c5_pad16(cout) / 16;
    p.tiles_x = (w + C5_TS - 1) / C5_TS; p.tiles_y = (h + C5_TS - 1) / C5_TS; p.nct = (cin + C5_NT - 1) / C5_NT;
    p.slope = slope;
    return conv5_gemm_launch(conv5_dgrad_kernel, p, stream);
}

extern "C" int sbmc_conv5x5_act_adjoint_nhwc_f32(float* g, const float* ysaved, float slope, long elems, unsigned* amax,
                                                  void* stream) {
    if (elems < 0 || elems % 16 || !amax || (uintptr_t)amax % 4) return SBMC_HIP_EINVAL;
    if (elems == 0) return 0;
    if (!g || !ysaved || (uintptr_t)g % 16 || (uintptr_t)ysaved % 16) return SBMC_HIP_EINVAL;
    const long n4 = elems / 4;
    const long blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(conv5_act_adjoint_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<float4*>(g), reinterpret_cast<const float4*>(ysaved), slope, n4, amax);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_wgrad_supported(int n, int h, int w, int cin, int cout) {
    return wgrad5_dims_ok(n, h, w, cin, cout) ? 1 : 0;
}

extern "C" size_t sbmc_conv5x5_wgrad_scratch_bytes(int n, int h, int w, int cin, int cout) {
    if (!wgrad5_dims_ok(n, h, w, cin, cout)) return 0;
    const size_t ncot = (size_t)(cout + W5_MT - 1) / W5_MT, ncit = (size_t)(cin + W5_NT - 1) / W5_NT;
    // per range: a tile of partial sums per (output tile, input tile, tap column) + 128 bias sums per output tile
    return (size_t)w5_splits(n, h, w, cin, cout) * (ncot * ncit * 5 * W5_TILE + ncot * W5_MT) * 4;
}

extern "C" int sbmc_conv5x5_wgrad_bias_f32(const float* gz, int ldg, const unsigned* gmax, const float* x, int ldx,
                                            const unsigned* xmax, float* gw, long s_co, long s_ci, long s_ky, long s_kx,
                                            float* gb, void* scratch, int n, int h, int w, int cin, int cout, void* stream) {
    if (!wgrad5_dims_ok(n, h, w, cin, cout) || !gz || !gmax || !x || !xmax || !gw || !gb || !scratch) return SBMC_HIP_EINVAL;
    if (!c5_ld_ok(ldx, cin) || !c5_ld_ok(ldg, cout)) return SBMC_HIP_EINVAL;
    if ((uintptr_t)gz % 16 || (uintptr_t)x % 16 || (uintptr_t)scratch % 16 || (uintptr_t)gw % 4 || (uintptr_t)gb % 4 ||
        (uintptr_t)gmax % 4 || (uintptr_t)xmax % 4)
        return SBMC_HIP_EINVAL;
    if (!wgrad5_strides_ok(w, ldg, ldx)) return SBMC_HIP_EINVAL;
    Wgrad5Params p;
    p.gz = gz; p.x = x; p.gmax = gmax; p.xmax = xmax;
    p.N = n; p.H = h; p.W = w; p.Ho = h - 4; p.Wo = w - 4; p.ldg = ldg; p.ldx = ldx;
    p.nstrips = (p.Wo + W5_PX - 1) / W5_PX; p.ncot = (cout + W5_MT - 1) / W5_MT; p.ncit = (cin + W5_NT - 1) / W5_NT;
    p.nsplit = w5_splits(n, h, w, cin, cout);
    p.total = (long long)n * p.Ho * p.nstrips;
    const int ncombo = p.ncot * p.ncit * 5;
    p.partial = static_cast<float*>(scratch);
    p.bpartial = p.partial + (size_t)p.nsplit * ncombo * W5_TILE;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_wgrad_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)W5_LDS_BYTES);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    hipLaunchKernelGGL(conv5_wgrad_kernel, dim3((unsigned)(ncombo * p.nsplit)), dim3(256), W5_LDS_BYTES, (hipStream_t)stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    Wreduce5Params q;
    q.partial = p.partial; q.bpartial = p.bpartial; q.gw = gw; q.gb = gb;
    q.s_co = s_co; q.s_ci = s_ci; q.s_ky = s_ky; q.s_kx = s_kx; q.gmax = gmax; q.xmax = xmax;
    q.cin = cin; q.cout = cout; q.ncot = p.ncot; q.ncit = p.ncit; q.nsplit = p.nsplit; q.ncombo = ncombo;
    hipLaunchKernelGGL(conv5_wgrad_reduce_kernel, dim3(W5_TILE / 256, (unsigned)(ncombo + 1)), dim3(256), 0, (hipStream_t)stream, q);
    return (int)hipGetLastError();
}
