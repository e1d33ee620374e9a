// The gradients of csrc/conv5x5_half.hip's 5 x 5 valid convolution on HALF activations -- `torch.nn.Conv2d(..., 5)`'s
// backward in KPCN's two chains (reference sbmc/models.py:221-291) under torch.autocast(float16) -- on that file's buffers
// (channels-last half [n][h][w][ld], ld the channel count rounded up to 16, EXACT ZEROS in the padding channels) and
// arithmetic (the half tensors as they are, fp32 weights rounded to half once at preparation, exact products summed in
// fp32 by v_mfma_f32_32x32x16_f16).  No scales, no magnitude words: a value beyond the half range becomes inf, as with the
// library.  Vector stores only; every buffer descriptor ends with its tensor (or with one row of it).
//
// (a) DATA GRADIENT with the producing layer's activation adjoint (conv5_half_dgrad_kernel), half in, half out:
//       gx[n,y,x,ci] = act'(xsaved[n,y,x,ci]) sum_{ky,kx,co} gz[n,y-ky,x-kx,co] w[co,ci,ky,kx]
//     The half forward's plan over gz padded by 4 zeros each way: a workgroup owns 32 x 16 pixels x 128 channels of gx, a
//     wave 8 x 16 pixels x all 128 channels (4 x 4 accumulators of 32 x 32), the 36 x 20 patch of gz is staged per chunk of
//     32 channels, a weight stage is 20 480 bytes, double-buffered, one barrier per stage, and the reduction walks granules
//     of 16 gz channels.  The prepared weights are sbmc_conv5x5_half_prepare_weights' with the channel strides and counts
//     exchanged; the kernel mirrors the taps (stage j reads prepared kernel row 4 - j, tap i column 4 - i).  The main loop
//     is written out here and not shared with conv5_half_kernel through an include: that kernel's register allocation
//     (256 AGPRs + 84 VGPRs, occupancy 1, no spill) is pinned by tests/test_conv5x5_half_host.py, and the fp32 pair's
//     experience (conv5x5_common.hpp) is that the same text in another frame compiles to another schedule.  What differs:
//       * the patch origin (y0 - 4, x0 - 4) in gz coordinates lies above / left of the tensor for border tiles, and a
//         row-major offset past a row's end lands in the next row, not in zeros: every patch pixel carries an in-range
//         predicate on BOTH sides of both coordinates; the descriptor's base is the first patch row that exists;
//       * the epilogue rounds the sum to half and multiplies by act' read from the saved half activation at the output
//         pixel (v > 0 ? 1 : slope; a null xsaved: nothing to undo), stores masked; a padding channel has zero weights and
//         is written as 0.  With ReLU (and no activation) that is ONE rounding: act' in {0, 1} is exact either side of it.
//         With a LeakyReLU slope the product is rounded again: autocast's arithmetic, where the convolution's backward
//         hands a half gx to the activation's backward -- so a chain's gradients are those of its layers run one by one,
//         to the bit, for any slope.  (Slope first and one rounding is 2^-11 closer to the exact product on the negative
//         side and a whole half ulp, up to 2^-10, away from the layered form wherever the two roundings fall apart.)
//         The 64 saved values of an accumulator row band are requested together, ahead of their use.
//
// (b) WEIGHT AND BIAS GRADIENT (conv5_half_wgrad_kernel + conv5_half_wgrad_reduce_kernel), half gz and x in, fp32 out:
//       gw[co][ci][ky][kx] = sum_{n,y,x} gz[n,y,x,co] x[n,y+ky,x+kx,ci],   gb[co] = sum gz
//     The reduction runs over pixels: the MFMA's k index is 8 consecutive pixels of one channel, the staging transposes.
//     Kept from the fp32 kernel (conv5x5_grad.hip): one tap column kx per workgroup with the shift folded into the x
//     addresses (pixel octets stay aligned), 128 output x 64 input channels and a contiguous RANGE of row stages (32
//     pixels of one gz row, down a 32-pixel column strip, strip after strip, image after image) per workgroup, the ring of
//     six x rows in LDS (each row fetched once for five gz rows), two gz stages, one barrier per stage, the partial sums
//     of the ranges in the caller's scratch added in a fixed order by a second kernel (no float atomics: the result does
//     not depend on the run), the bias partials riding along in fp32.  There is no scale-back step.
//     The tile, for ONE plane and ONE product per term.  Per pixel octet a wave tile of Mb output-channel blocks x Nb
//     input-channel blocks x 5 kernel rows that fetches every operand from LDS reads Mb + 5 Nb operands for 5 Mb Nb MFMAs,
//     and 80 Mb Nb accumulator registers must stay within 256 (Mb Nb <= 3):
//       * 2 x 1 (the fp32 kernel's wave tile, one plane deleted): 7 reads per 10 MFMAs = 0.7 -- LDS-bound, as
//         conv5x5_half.hip's header says of 0.75;
//       * 3 x 1: 8 per 15 = 0.53, 240 accumulators: one wave per SIMD, and 96-channel tiles fit KPCN's 100 output
//         channels badly (two tiles, 48 % of the MFMAs on padding);
//       * 1 x 3: 16 per 15: worse than either.
//     The 5 Nb term is the x operand of every kernel row, and it is the same data stage after stage: x row y + ky of gz
//     row y is x row (y + 1) + (ky - 1) of the next.  SHIPPED: the 2 x 1 wave tile (64 output x 32 input channels x 5
//     rows, 160 accumulators) with the five x rows' operands HELD IN REGISTERS (40) and rotated from stage to stage: a
//     stage reads its 4 gz operands and the 2 operands of the ONE new x row -- 6 reads per 20 MFMAs = 0.3 per MFMA (a
//     strip's first stage reads all five rows: 14, once per strip height).  160 + 40 + staging fits 256 registers: two
//     workgroups per CU (two waves per SIMD) hide each other's staging and barrier; a row is 4.5 KB and a gz stage 8 KB, 43 KB
//     of LDS a workgroup.  Rejected besides the above: 2 x 2 x 5 with held operands (0.2, but 320 accumulators: the fp32
//     kernel's header records what the compiler does beyond 256), and more workgroups per CU (LDS would allow three: the
//     registers do not).
//       * staging: a thread owns 4 pixels x 8 channels (four 16-byte loads), transposes them with 16 byte permutes and
//         writes eight 8-byte halves of entries.  Waves 0 and 1 stage gz, wave 2 the x row (one set of registers serves
//         either role); channel 8 q + c of a tile is kept at slot 16 c + q (8 c + q on the x side, whose pixel octets lie
//         72 entries apart: 1152 = 128 mod 256 bytes), so that the 32 lanes of a write fall on 256 different bytes and a
//         wave's operand read on consecutive entries; an accumulator row only means another channel (undone by the
//         reduction kernel).
//
// (c) conv5_half_pack_adj_kernel: the planar cotangent (half or fp32) -> channels-last half, multiplied by the adjoint of
//     the chain's LAST activation read from the saved half output (one rounding); the unpack of gx to planar fp32.  Planar
//     half out, and the pack without an adjoint, are conv5x5_half.hip's entry points.
//
// build.EXTRA_FLAGS: the other 5 x 5 files' (no packed fp32 arithmetic).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sbmc_hip.h"
#include "common.hpp"
#include "conv5x5_common.hpp"

namespace sbmc {

using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

// =====================================================================================================================
// (a) data gradient.  The H5_ constants are conv5x5_half.hip's (the plan is that file's).
constexpr int H5_TY = 32, H5_TX = 16;                 // tile (gx pixels): rows x columns
constexpr int H5_PY = H5_TY + 4, H5_PX = H5_TX + 4;   // patch (gz pixels)
constexpr int H5_PP = H5_PY * H5_PX;                  // 720
constexpr int H5_PR = H5_PP + 4;                      // entries of one octet's region: 724 = 4 (mod 16)
constexpr int H5_ABUF = 4 * H5_PR;                    // 16-byte entries of one patch chunk: [octet 4][pixel]
constexpr int H5_WSTAGE = 5 * 2 * C5_NT;              // 16-byte entries of one weight stage: [kx 5][k half 2][128]
constexpr unsigned H5_LDS_BYTES = (2 * H5_ABUF + 2 * H5_WSTAGE) * 16;      // 133632
constexpr int H5_AROUNDS = H5_PY / 3;                 // staging rounds of three patch rows: 12
constexpr int H5_WROUNDS = H5_WSTAGE / 256;           // 5 entries of a stage per thread

struct Dgrad5HalfParams {
    const _Float16* gz;      // [N, H - 4, W - 4, ldg]
    const u32x4* wp;         // prepared with the sides exchanged: [cin tile][K16 of cout][ky][kx][k half][128]
    const _Float16* xsaved;  // [N, H, W, ldx] or nullptr
    _Float16* gx;            // [N, H, W, ldx]
    int N, H, W, Ha, Wa, ldg, ldx;
    int K16;                 // granules of 16 gz channels
    int tiles_x, tiles_y, ncit;
    float slope;             // act' below zero
};

__global__ __launch_bounds__(256) void conv5_half_dgrad_kernel(Dgrad5HalfParams p) {
    extern __shared__ float4 hd5_lds[];
    u32x4* As = reinterpret_cast<u32x4*>(hd5_lds);
    u32x4* Ws = As + 2 * H5_ABUF;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_id();
    const int l31 = lane & 31, lhi = lane >> 5;
    const int pcol = c5_pcol(l31);
    const int K16 = p.K16, nchunks = (K16 + 1) >> 1, nstages = K16 * 5;

    const C5Tile tl = c5_tile<H5_TY, H5_TX>(blockIdx.x, p.ncit, p.tiles_x, p.tiles_y);
    const int ct = tl.ct, x0 = tl.x0, y0 = tl.y0, n = tl.n;

    // ---- staging of a patch chunk: conv5_half_kernel's roles (three patch rows a round, twelve rounds, threads 240 ..
    // 255 doubling 224 .. 239).  Patch pixel (qr, qc) is gz pixel (y0 - 4 + qr, x0 - 4 + qc): the column's predicate does
    // not depend on the round, the row's is 3 j in [alo, arows).  Offsets count from gz row rbase, the first patch row
    // that exists (y0 <= H - 1: y0 - 4 <= Ha - 1); a row above it has a negative offset, wrapped and never used ----
    const int gy0 = y0 - 4, rbase = gy0 > 0 ? gy0 : 0;
    const long long aelems = (long long)p.N * p.Ha * p.Wa * p.ldg;
    const long long afirst = (((long long)n * p.Ha + rbase) * p.Wa) * p.ldg;
    const rsrc_t ra = c5_rsrc(p.gz + afirst, (aelems - afirst) * 2);
    const rsrc_t rnone = c5_rsrc(p.gz, 0);
    const int atid = tid < 3 * 4 * H5_PX ? tid : tid - 16;
    const int arow = atid / (4 * H5_PX), acol = (atid % (4 * H5_PX)) >> 2, aoct = atid & 3;
    const int gc = x0 - 4 + acol;
    const bool aidle = gc < 0 || gc >= p.Wa;
    const unsigned avoff = (unsigned)(((gy0 + arow - rbase) * p.Wa + gc) * p.ldg + aoct * 8) * 2u;
    const unsigned astep = (unsigned)(3 * p.Wa * p.ldg) * 2u;
    const int alo = rbase - gy0 - arow;                    // round j's row is a row of gz from 3 j >= alo ...
    const int arows = aidle ? 0 : p.Ha - gy0 - arow;       // ... while 3 j < arows
    auto issue_a = [&](int cc, int j, bool valid) -> u32x4 {
        const rsrc_t r = valid ? ra : rnone;
        const int rows = (aoct >= 2 && 2 * cc + 1 >= K16) ? 0 : arows;
        const bool in = 3 * j >= alo && 3 * j < rows;
        return __builtin_amdgcn_raw_buffer_load_b128(r, in ? avoff + (unsigned)j * astep : C5_OOB, (unsigned)cc * 64u, 0);
    };
    u32x4* const a_dst = As + aoct * H5_PR + arow * H5_PX + acol;
    auto commit_a = [&](int abuf, int j, u32x4 v) { a_dst[abuf * H5_ABUF + j * 3 * H5_PX] = v; };
    // ---- staging of a weight stage: granule g, PREPARED kernel row kr ----
    const long long wentries = (long long)p.ncit * nstages * H5_WSTAGE;
    const rsrc_t rw = c5_rsrc(p.wp, wentries * 16);
    u32x4 wreg[H5_WROUNDS];
    auto issue_w = [&](int g, int kr, bool valid) {
        const rsrc_t r = valid ? rw : rnone;
        const unsigned block = valid ? (unsigned)(ct * nstages + g * 5 + kr) : 0u;
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

    // operands of one tap: A 4 m-blocks, B 4 n-blocks; tap i of a stage: the patch shifted by i entries against prepared
    // column 4 - i
    struct Ops { u32x4 a[4], b[4]; };
    auto load_ops = [&](Ops& o, const u32x4* Ab, const u32x4* Wb, int i) {
        const int kc = 4 - i;
        o.b[0] = Wb[kc * 256];
        o.a[0] = Ab[i];
        o.b[1] = Wb[kc * 256 + 32];
        o.a[1] = Ab[2 * H5_PX + i];
#pragma unroll
        for (int ni = 2; ni < 4; ++ni) o.b[ni] = Wb[kc * 256 + ni * 32];
#pragma unroll
        for (int mi = 2; mi < 4; ++mi) o.a[mi] = Ab[mi * 2 * H5_PX + i];
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
    const u32x4* const a_lane = As + lhi * H5_PR + (wave * 8 + (l31 >> 4)) * H5_PX + pcol;
    const u32x4* const w_lane = Ws + lhi * C5_NT + l31;

    // ---- prologue: chunk 0's patch and the first stage (prepared kernel row 4) ----
    {
        u32x4 a0[H5_AROUNDS];
#pragma unroll
        for (int j = 0; j < H5_AROUNDS; ++j) a0[j] = issue_a(0, j, true);
        issue_w(0, 4, true);
#pragma unroll
        for (int j = 0; j < H5_AROUNDS; ++j) commit_a(0, j, a0[j]);
        commit_w(0);
    }
    __syncthreads();

    // conv5_half_kernel's pipeline: granule g = 2 cc + ks reads patch buffer cc % 2, octets 2 ks and 2 ks + 1; its stage
    // s = 5 g + j reads weight buffer s % 2; the next stage's weights and two rounds of the next chunk's patch are
    // requested before a stage's MFMAs and written behind them; one loop body for both granules of a chunk.
    for (int g = 0; g < K16; ++g) {
        const int cc = g >> 1, ks = g & 1;
        const bool more = cc + 1 < nchunks;
        const u32x4* const Ac = a_lane + (cc & 1) * H5_ABUF + ks * 2 * H5_PR;
        auto stage = [&](const int j) {
            const int s = g * 5 + j, wbuf = (g + j) & 1, j0 = 2 * (3 * ks + j);
            if (j < 4) issue_w(g, 3 - j, true);
            else issue_w(g + 1, 4, s + 1 < nstages);
            u32x4 a0, a1;
            if (j < 3) {
                a0 = issue_a(cc + 1, j0, more);
                a1 = issue_a(cc + 1, j0 + 1, more);
            }
            __builtin_amdgcn_sched_barrier(0);         // (the requests stay in front of the stage's MFMAs)
            const u32x4* Ab = Ac + j * H5_PX;
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
            if (j < 3) {
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

    // ---- epilogue: act' from the saved activation, one rounding to half, masked stores ----
    // (the accumulators are read by hand, as in conv5_half_kernel: 11 wait states behind the last 8-pass MFMA, the two
    // s_nop 15 give 32)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15");
    __builtin_amdgcn_sched_barrier(0);
    const long long yelems = (long long)p.N * p.H * p.W * p.ldx;
    const long long yfirst = (((long long)n * p.H + y0) * p.W + x0) * p.ldx;
    const rsrc_t ry = c5_rsrc(p.gx + yfirst, (yelems - yfirst) * 2);
    const bool undo = p.xsaved != nullptr;
    const rsrc_t rs = undo ? c5_rsrc(p.xsaved + yfirst, (yelems - yfirst) * 2) : rnone;
    int ch[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) ch[ni] = ct * C5_NT + ni * 32 + l31;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        unsigned saved[16][4];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wave * 8 + mi * 2 + c5_acc_row(r);
            const int col = c5_acc_col(r, lhi);
            const bool ok = y0 + row < p.H && x0 + col < p.W;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const bool st = ok && ch[ni] < p.ldx;
                const unsigned voff = st ? (unsigned)((row * p.W + col) * p.ldx + ch[ni]) * 2u : C5_OOB;
                saved[r][ni] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs, voff, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wave * 8 + mi * 2 + c5_acc_row(r);
            const int col = c5_acc_col(r, lhi);
            const bool ok = y0 + row < p.H && x0 + col < p.W;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const bool st = ok && ch[ni] < p.ldx;
                const unsigned voff = st ? (unsigned)((row * p.W + col) * p.ldx + ch[ni]) * 2u : C5_OOB;
                float v;
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(acc[mi][ni][r]));
                // (the sum rounded to half, THEN the slope and a second rounding: the library's half gx followed by
                // autocast's LeakyReLU backward on it, to the bit; for act' in {0, 1} the product is exact)
                _Float16 hv = (_Float16)v;
                hv = (undo && !((float)raw_half(saved[r][ni]) > 0.f)) ? (_Float16)((float)hv * p.slope) : hv;
                __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, hv), ry, voff, 0, 0);
            }
        }
    }
}

// =====================================================================================================================
// (b) weight and bias gradient
constexpr int HW5_PX = 32;                      // pixels of a row stage
constexpr int HW5_MT = 128, HW5_NT = 64;        // output / input channels of a workgroup
constexpr int HW5_GBUF = 4 * HW5_MT;            // 16-byte entries of a gz stage: [pixel octet 4][slot 128]
constexpr int HW5_XOCT = HW5_NT + 8;            // entries between the pixel octets of an x row (64 slots + 8 unused)
constexpr int HW5_XROW = 4 * HW5_XOCT;          // ... of an x row
constexpr int HW5_RING = 6;                     // x rows in LDS: five in use, one being written
constexpr unsigned HW5_LDS_BYTES = (2 * HW5_GBUF + HW5_RING * HW5_XROW) * 16;      // 44032
constexpr int HW5_TILE = 5 * HW5_MT * HW5_NT;   // floats of a workgroup's partial sums: [ky 5][co row 128][ci slot 64]
constexpr int HW5_MIN_STAGES = 4;               // row stages of a range at least

struct Wgrad5HalfParams {
    const _Float16* gz;      // [N, H - 4, W - 4, ldg]
    const _Float16* x;       // [N, H, W, ldx]
    float* partial;          // [nsplit][ncombo][HW5_TILE]
    float* bpartial;         // [nsplit][ncot][128]
    int N, H, W, Ho, Wo, ldg, ldx;
    int nstrips, ncot, ncit, nsplit;
    long long total;         // row stages: N nstrips Ho
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv5_half_wgrad_kernel(Wgrad5HalfParams p) {
    extern __shared__ float4 hw5_lds[];
    u32x4* Gs = reinterpret_cast<u32x4*>(hw5_lds);
    u32x4* Xs = Gs + 2 * HW5_GBUF;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_id();
    const int l31 = lane & 31, lhi = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;

    // the workgroup: (range, output tile, input tile, tap column), the tap columns of a tile next to each other
    unsigned t = blockIdx.x;
    const int kx = (int)(t % 5u);
    t /= 5u;
    const int cit = (int)(t % (unsigned)p.ncit);
    t /= (unsigned)p.ncit;
    const int ct = (int)(t % (unsigned)p.ncot);
    const int split = (int)(t / (unsigned)p.ncot);
    const long long s_begin = p.total * split / p.nsplit, s_end = p.total * (split + 1) / p.nsplit;

    // ---- staging roles, one per WAVE: waves 0, 1 the gz stage, wave 2 the x row, wave 3 none.  A thread owns 4 pixels
    // (half h of pixel octet oct) x 8 channels (octet cq of the tile) ----
    const bool isg = wave < 2, isx = wave == 2;
    const int sh = tid & 1;
    const int scq = isg ? (tid >> 1) & 15 : (tid >> 1) & 7;
    const int soct = isg ? tid >> 5 : (tid >> 4) & 3;
    const int sch = isg ? ct * HW5_MT + 8 * scq : cit * HW5_NT + 8 * scq;
    const int sld = isg ? p.ldg : p.ldx, sw = isg ? p.Wo : p.W;
    const bool schok = (isg || isx) && sch < sld;
    const int spx = (isg ? 0 : kx) + 8 * soct + 4 * sh;      // (the tap column's shift: pixel octets stay aligned)
    const rsrc_t rnone = c5_rsrc(p.gz, 0);
    // this thread's half entries of channel c = 0: + c * scs entries from one to the next
    u32x2* const sdst = reinterpret_cast<u32x2*>(isg ? Gs + soct * HW5_MT + scq : Xs + soct * HW5_XOCT + scq) + sh;
    const int scs = isg ? 16 : 8;
    u32x4 sreg[4];
    float bsum[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) bsum[c] = 0.f;

    // one gz row / x row per descriptor: every offset is checked against the row's end; a pixel beyond the row and a
    // channel beyond the buffer's stride carry the sentinel (a channel offset past ld would land in the next pixel).
    // yr: the row of the role's tensor (wave-uniform)
    auto issue = [&](int n, int yr, int xs, bool valid) {
        const _Float16* row = isg ? p.gz + (((long long)n * p.Ho + yr) * p.Wo) * p.ldg
                                  : p.x + (((long long)n * p.H + yr) * p.W) * p.ldx;
        const rsrc_t r = valid && !(wave == 3) ? c5_rsrc(row, (long long)sw * sld * 2) : rnone;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int px = xs + spx + q;
            const unsigned voff = (px < sw && schok) ? (unsigned)(px * sld + sch) * 2u : C5_OOB;
            sreg[q] = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
        }
    };
    // 4 pixels x 8 channels -> channel c's four pixels = half an entry (8 bytes), at `entry` (a gz buffer / a ring slot)
    auto commit = [&](int entry) {
        u32x2* d = sdst + 2 * entry;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const unsigned sel = (c & 1) ? 0x07060302u : 0x05040100u;
            u32x2 v;
            v[0] = __builtin_amdgcn_perm(sreg[1][c >> 1], sreg[0][c >> 1], sel);
            v[1] = __builtin_amdgcn_perm(sreg[3][c >> 1], sreg[2][c >> 1], sel);
            d[2 * c * scs] = v;
        }
    };
    auto bias_add = [&]() {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int sft = (c & 1) * 16;
            bsum[c] += ((float)raw_half(sreg[0][c >> 1] >> sft) + (float)raw_half(sreg[1][c >> 1] >> sft)) +
                       ((float)raw_half(sreg[2][c >> 1] >> sft) + (float)raw_half(sreg[3][c >> 1] >> sft));
        }
    };
    const bool bias_wg = kx == 0 && cit == 0;
    auto commit_g = [&](int buf) {
        if (isg) {
            commit(buf * HW5_GBUF);
            if (bias_wg) bias_add();
        }
    };
    auto commit_x = [&](int slot) {
        if (isx) commit(slot * HW5_XROW);
    };
    // the five x rows of a strip's (or a range's) first stage: rows y .. y + 4 into their ring slots, one after the other
    // through wave 2's registers (it has no row in flight then)
    auto fill = [&](int n, int y, int xs) {
        if (isx) {
            for (int j = 0; j < 5; ++j) {
                issue(n, y + j, xs, true);
                commit((y + j) % HW5_RING * HW5_XROW);
            }
        }
    };

    f32x16 acc[5][2];
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ky][mi][r] = 0.f;

    const u32x4* const g_lane = Gs + lhi * HW5_MT + mh * 64 + l31;
    const u32x4* const x_lane = Xs + lhi * HW5_XOCT + nh * 32 + l31;
    // the operands of x rows y .. y + 4, two k steps of 16 pixels each: held from stage to stage
    u32x4 xb[5][2];
    auto read_x = [&](int ky, int slot) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) xb[ky][ks] = x_lane[slot * HW5_XROW + ks * 2 * HW5_XOCT];
    };
    auto wrap = [](int s) { return s >= HW5_RING ? s - HW5_RING : s; };

    // ---- the range's first stage ----
    int y = (int)(s_begin % p.Ho);
    long long rest = s_begin / p.Ho;
    int strip = (int)(rest % p.nstrips);
    int n = (int)(rest / p.nstrips);
    if (isg) issue(n, y, strip * HW5_PX, true);
    fill(n, y, strip * HW5_PX);
    commit_g(0);
    __syncthreads();

    // Stage s reads gz buffer s % 2 and the newest ring slot.  The rows of stage s + 1 are requested at its start and
    // written at its end: the gz row into the other buffer (last read in stage s - 1, before the previous barrier), x row
    // y + 5 into the sixth slot.  A stage that opens a new strip needs five new x rows in slots that may be in use: none is
    // requested ahead (an empty descriptor, not a branch), they are filled behind a barrier of their own and the next
    // stage reads all five.
    int buf = 0, y6 = y % HW5_RING;
    bool fresh = true;
    for (long long s = s_begin; s < s_end; ++s) {
        int ny = y + 1, nstrip = strip, nn = n;
        if (ny == p.Ho) {
            ny = 0;
            if (++nstrip == p.nstrips) { nstrip = 0; ++nn; }
        }
        const bool more = s + 1 < s_end;
        issue(nn, isg ? ny : ny + 4, nstrip * HW5_PX, more && (isg || ny != 0));
        if (fresh) {
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) read_x(ky, wrap(y6 + ky));
        } else {
#pragma unroll
            for (int ky = 0; ky < 4; ++ky)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) xb[ky][ks] = xb[ky + 1][ks];
            read_x(4, wrap(y6 + 4));
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 a[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) a[mi] = g_lane[buf * HW5_GBUF + ks * 2 * HW5_MT + mi * 32];
#pragma unroll
            for (int ky = 0; ky < 5; ++ky)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) acc[ky][mi] = c5_mfma(a[mi], xb[ky][ks], acc[ky][mi]);
        }
        if (more) {
            if (ny == 0) {
                __syncthreads();
                fill(nn, 0, nstrip * HW5_PX);
            } else {
                commit_x((ny + 4) % HW5_RING);
            }
            commit_g(buf ^ 1);
        }
        __syncthreads();
        buf ^= 1;
        fresh = ny == 0;
        y = ny; strip = nstrip; n = nn;
        y6 = ny == 0 ? 0 : (y6 + 1 == HW5_RING ? 0 : y6 + 1);
    }

    // ---- the partial sums: [ky][co row][ci slot], a wave's 32 lanes on 128 consecutive bytes ----
    float* tile = p.partial + (size_t)blockIdx.x * HW5_TILE;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int corow = (mh * 2 + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                tile[(ky * HW5_MT + corow) * HW5_NT + nh * 32 + l31] = acc[ky][mi][r];
            }
    // ---- the bias partials: eight threads hold sums of a channel octet (the last barrier is behind every LDS read) ----
    if (bias_wg) {
        float* red = reinterpret_cast<float*>(Gs);
        if (isg) {
#pragma unroll
            for (int c = 0; c < 8; ++c) red[(soct * 2 + sh) * HW5_MT + 8 * scq + c] = bsum[c];
        }
        __syncthreads();
        if (tid < HW5_MT) {
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += red[j * HW5_MT + tid];
            p.bpartial[((size_t)split * p.ncot + ct) * HW5_MT + tid] = sum;
        }
    }
}

struct Wreduce5HalfParams {
    const float* partial;
    const float* bpartial;
    float* gw;
    float* gb;
    long s_co, s_ci, s_ky, s_kx;
    int cin, cout, ncot, ncit, nsplit, ncombo;
};

// blockIdx.y < ncombo: element blockIdx.x 256 + thread of combination (ct, cit, kx)'s tile, summed over the ranges in
// their order; blockIdx.y == ncombo: the bias gradient
__global__ __launch_bounds__(256) void conv5_half_wgrad_reduce_kernel(Wreduce5HalfParams p) {
    const int combo = (int)blockIdx.y;
    if (combo == p.ncombo) {
        for (int co = (int)(blockIdx.x * 256 + threadIdx.x); co < p.cout; co += (int)gridDim.x * 256) {
            float s = 0.f;
            for (int k = 0; k < p.nsplit; ++k) s += p.bpartial[((size_t)k * p.ncot + co / HW5_MT) * HW5_MT + co % HW5_MT];
            p.gb[co] = s;
        }
        return;
    }
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    float s = 0.f;
    for (int k = 0; k < p.nsplit; ++k) s += p.partial[((size_t)k * p.ncombo + combo) * HW5_TILE + e];
    const int kx = combo % 5, cit = (combo / 5) % p.ncit, ct = combo / (5 * p.ncit);
    const int cislot = e % HW5_NT, corow = (e / HW5_NT) % HW5_MT, ky = e / (HW5_NT * HW5_MT);
    // slot -> channel: the staging keeps channel 8 q + c at slot 16 c + q (gz) / 8 c + q (x)
    const int co = ct * HW5_MT + 8 * (corow % 16) + corow / 16;
    const int ci = cit * HW5_NT + 8 * (cislot % 8) + cislot / 8;
    if (co < p.cout && ci < p.cin) p.gw[co * p.s_co + ci * p.s_ci + ky * p.s_ky + kx * p.s_kx] = s;
}

// =====================================================================================================================
// (c) planar cotangent [n][c][hw] (half or fp32) -> channels-last half [n][hw][ld], times act'(ysaved) (ysaved: the chain's
// activated output, channels-last half of the same shape): repack5_kernel's tiles of 64 pixels x 32 channels through LDS
template <typename S>
__global__ __launch_bounds__(256) void conv5_half_pack_adj_kernel(const S* __restrict__ src, const _Float16* __restrict__ ysaved,
                                                                  float slope, _Float16* __restrict__ dst, int c, int ld, long hw,
                                                                  int ctiles, long ptiles) {
    __shared__ float tile[32][65];
    long b = blockIdx.x;
    const int cti = (int)(b % ctiles);
    b /= ctiles;
    const long pt = b % ptiles;
    const long n = b / ptiles;
    const long p0 = pt * 64;
    const int c0 = cti * 32;
    const int tid = (int)threadIdx.x;
    const S* planar = src + n * (long)c * hw;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int cl = (tid >> 6) + 4 * i, px = tid & 63;
        tile[cl][px] = (c0 + cl < c && p0 + px < hw) ? (float)planar[(long)(c0 + cl) * hw + p0 + px] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int px = (tid >> 5) + 8 * i, cl = tid & 31;
        if (p0 + px < hw && c0 + cl < ld) {
            const long at = (n * hw + p0 + px) * ld + c0 + cl;
            const float v = tile[cl][px];
            dst[at] = (_Float16)((float)ysaved[at] > 0.f ? v : v * slope);
        }
    }
}

template <typename S>
static int pack_adj5(const S* g, const _Float16* ysaved, float slope, _Float16* gz, int ld, int n, int c, long hw, void* stream) {
    if (n < 0 || c < 1 || hw < 0 || !c5_ld_ok(ld, c)) return SBMC_HIP_EINVAL;
    if (n == 0 || hw == 0) return 0;
    if (!g || !ysaved || !gz || (uintptr_t)g % sizeof(S) || (uintptr_t)ysaved % 2 || (uintptr_t)gz % 2) return SBMC_HIP_EINVAL;
    const int ctiles = (ld + 31) / 32;
    const long ptiles = (hw + 63) / 64;
    const long long blocks = (long long)n * ptiles * ctiles;
    if (blocks >= 0x7FFFFFFFll) return SBMC_HIP_EINVAL;
    hipLaunchKernelGGL((conv5_half_pack_adj_kernel<S>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, ysaved, slope,
                       gz, c, ld, hw, ctiles, ptiles);
    return (int)hipGetLastError();
}

static int hw5_cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 1) {
        (void)hipGetLastError();
        return 256;
    }
    return cus;
}

// one descriptor spans the patch rows of gz from a tile's first existing one, another a tile's rows of gx / xsaved
static bool dgrad5_half_strides_ok(int w, long long ldg, long long ldx) {
    return c5_strides_ok(H5_PY + 1, w - 4, ldg, H5_TY + 1, w, ldx, 2);
}
// ... one row of x, another one row of gz
static bool wgrad5_half_strides_ok(int w, long long ldg, long long ldx) { return c5_strides_ok(1, w, ldx, 1, w - 4, ldg, 2); }

static bool dgrad5_half_dims_ok(int n, int h, int w, int cin, int cout) {
    if (!c5_shape_ok(n, h, w, cin, cout)) return false;
    const long long ldx = c5_pad16(cin), ldg = c5_pad16(cout), ncit = (cin + C5_NT - 1) / C5_NT;
    if (!dgrad5_half_strides_ok(w, ldg, ldx)) return false;
    const long long tiles = (long long)n * ((h + H5_TY - 1) / H5_TY) * ((w + H5_TX - 1) / H5_TX) * ncit;
    return tiles < 0x7FFFFFFFll && ncit * (ldg / 16) * 5 * H5_WSTAGE * 16 < C5_MAXOFF;
}

static bool wgrad5_half_dims_ok(int n, int h, int w, int cin, int cout) {
    if (!c5_shape_ok(n, h, w, cin, cout) || !wgrad5_half_strides_ok(w, c5_pad16(cout), c5_pad16(cin))) return false;
    const long long ncombo = (long long)((cout + HW5_MT - 1) / HW5_MT) * ((cin + HW5_NT - 1) / HW5_NT) * 5;
    return ncombo < 65535;
}

// ranges of row stages: two workgroups per compute unit (what the registers allow) over the (tap column, channel tile)
// combinations, HW5_MIN_STAGES stages at least
static int hw5_splits(int n, int h, int w, int cin, int cout) {
    const long long total = (long long)n * (h - 4) * ((w - 4 + HW5_PX - 1) / HW5_PX);
    const int ncombo = ((cout + HW5_MT - 1) / HW5_MT) * ((cin + HW5_NT - 1) / HW5_NT) * 5;
    long long s = 2 * hw5_cu_count() / ncombo;
    if (s > total / HW5_MIN_STAGES) s = total / HW5_MIN_STAGES;
    return (int)(s < 1 ? 1 : s);
}

}  // namespace sbmc

using namespace sbmc;

extern "C" int sbmc_conv5x5_half_dgrad_supported(int n, int h, int w, int cin, int cout) {
    return dgrad5_half_dims_ok(n, h, w, cin, cout) ? 1 : 0;
}

extern "C" int sbmc_conv5x5_half_dgrad_adj_nhwc(const void* gz, int ldg, const void* wp_swapped, const void* xsaved, float slope,
                                                 void* gx, int ldx, int n, int h, int w, int cin, int cout, void* stream) {
    if (!dgrad5_half_dims_ok(n, h, w, cin, cout) || !gz || !wp_swapped || !gx) return SBMC_HIP_EINVAL;
    if (!c5_ld_ok(ldx, cin) || !c5_ld_ok(ldg, cout)) return SBMC_HIP_EINVAL;
    if ((uintptr_t)gz % 16 || (uintptr_t)wp_swapped % 16 || (uintptr_t)gx % 16 || (uintptr_t)xsaved % 16) return SBMC_HIP_EINVAL;
    if (!dgrad5_half_strides_ok(w, ldg, ldx)) return SBMC_HIP_EINVAL;
    Dgrad5HalfParams p;
    p.gz = static_cast<const _Float16*>(gz); p.wp = static_cast<const u32x4*>(wp_swapped);
    p.xsaved = static_cast<const _Float16*>(xsaved); p.gx = static_cast<_Float16*>(gx);
    p.N = n; p.H = h; p.W = w; p.Ha = h - 4; p.Wa = w - 4; p.ldg = ldg; p.ldx = ldx;
    // (the weights were prepared with the sides exchanged: cout is their reduction side)
    p.K16 = c5_pad16(cout) / 16;
    p.tiles_x = (w + H5_TX - 1) / H5_TX; p.tiles_y = (h + H5_TY - 1) / H5_TY; p.ncit = (cin + C5_NT - 1) / C5_NT;
    p.slope = slope;
    const unsigned grid = (unsigned)((long long)n * p.tiles_y * p.tiles_x * p.ncit);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_half_dgrad_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)H5_LDS_BYTES);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    hipLaunchKernelGGL(conv5_half_dgrad_kernel, dim3(grid), dim3(256), H5_LDS_BYTES, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_half_wgrad_supported(int n, int h, int w, int cin, int cout) {
    return wgrad5_half_dims_ok(n, h, w, cin, cout) ? 1 : 0;
}

extern "C" size_t sbmc_conv5x5_half_wgrad_scratch_bytes(int n, int h, int w, int cin, int cout) {
    if (!wgrad5_half_dims_ok(n, h, w, cin, cout)) return 0;
    const size_t ncot = (size_t)(cout + HW5_MT - 1) / HW5_MT, ncit = (size_t)(cin + HW5_NT - 1) / HW5_NT;
    // per range: a tile of partial sums per (output tile, input tile, tap column) + 128 bias sums per output tile
    return (size_t)hw5_splits(n, h, w, cin, cout) * (ncot * ncit * 5 * HW5_TILE + ncot * HW5_MT) * 4;
}

extern "C" int sbmc_conv5x5_half_wgrad_bias(const void* gz, int ldg, const void* x, int ldx, float* gw, long s_co, long s_ci,
                                             long s_ky, long s_kx, float* gb, void* scratch, int n, int h, int w, int cin,
                                             int cout, void* stream) {
    if (!wgrad5_half_dims_ok(n, h, w, cin, cout) || !gz || !x || !gw || !gb || !scratch) return SBMC_HIP_EINVAL;
    if (!c5_ld_ok(ldx, cin) || !c5_ld_ok(ldg, cout)) return SBMC_HIP_EINVAL;
    if ((uintptr_t)gz % 16 || (uintptr_t)x % 16 || (uintptr_t)scratch % 16 || (uintptr_t)gw % 4 || (uintptr_t)gb % 4)
        return SBMC_HIP_EINVAL;
    if (!wgrad5_half_strides_ok(w, ldg, ldx)) return SBMC_HIP_EINVAL;
    Wgrad5HalfParams p;
    p.gz = static_cast<const _Float16*>(gz); p.x = static_cast<const _Float16*>(x);
    p.N = n; p.H = h; p.W = w; p.Ho = h - 4; p.Wo = w - 4; p.ldg = ldg; p.ldx = ldx;
    p.nstrips = (p.Wo + HW5_PX - 1) / HW5_PX; p.ncot = (cout + HW5_MT - 1) / HW5_MT; p.ncit = (cin + HW5_NT - 1) / HW5_NT;
    p.nsplit = hw5_splits(n, h, w, cin, cout);
    p.total = (long long)n * p.Ho * p.nstrips;
    const int ncombo = p.ncot * p.ncit * 5;
    p.partial = static_cast<float*>(scratch);
    p.bpartial = p.partial + (size_t)p.nsplit * ncombo * HW5_TILE;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv5_half_wgrad_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)HW5_LDS_BYTES);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    hipLaunchKernelGGL(conv5_half_wgrad_kernel, dim3((unsigned)(ncombo * p.nsplit)), dim3(256), HW5_LDS_BYTES, (hipStream_t)stream, p);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    Wreduce5HalfParams q;
    q.partial = p.partial; q.bpartial = p.bpartial; q.gw = gw; q.gb = gb;
    q.s_co = s_co; q.s_ci = s_ci; q.s_ky = s_ky; q.s_kx = s_kx;
    q.cin = cin; q.cout = cout; q.ncot = p.ncot; q.ncit = p.ncit; q.nsplit = p.nsplit; q.ncombo = ncombo;
    hipLaunchKernelGGL(conv5_half_wgrad_reduce_kernel, dim3(HW5_TILE / 256, (unsigned)(ncombo + 1)), dim3(256), 0,
                       (hipStream_t)stream, q);
    return (int)hipGetLastError();
}

extern "C" int sbmc_conv5x5_half_pack_adj_nchw_f32(const float* g, const void* ysaved, float slope, void* gz, int ld, int n, int c,
                                                    long hw, void* stream) {
    return pack_adj5<float>(g, static_cast<const _Float16*>(ysaved), slope, static_cast<_Float16*>(gz), ld, n, c, hw, stream);
}

extern "C" int sbmc_conv5x5_half_pack_adj_nchw_f16(const void* g, const void* ysaved, float slope, void* gz, int ld, int n, int c,
                                                    long hw, void* stream) {
    return pack_adj5<_Float16>(static_cast<const _Float16*>(g), static_cast<const _Float16*>(ysaved), slope,
                               static_cast<_Float16*>(gz), ld, n, c, hw, stream);
}

extern "C" int sbmc_conv5x5_half_unpack_nhwc_f32(const void* x, int ldx, float* y, int n, int c, long hw, void* stream) {
    return repack5<_Float16, float, false>(static_cast<const _Float16*>(x), y, ldx, n, c, hw, stream);
}
