// What the three 5 x 5 files share.
//   * csrc/conv5x5.hip (forward) and csrc/conv5x5_grad.hip (data gradient) run ONE implicit-GEMM tile body,
//     csrc/conv5x5_gemm_body.inc: the 16 x 16 pixels x 128 channels plan described at the top of conv5x5.hip, with its LDS
//     carve-up, patch and weight staging, two accumulator sets, operand fetches between the MFMAs, five-stage pipeline and
//     the accumulator walk of the epilogue.  conv5_kernel and conv5_dgrad_kernel include it as their body with
//     `using Side = Conv5Fwd / Conv5Dgrad` (below); `if constexpr (Side::mirror)` picks what the mathematics changes: where a
//     patch pixel lies and whether it exists, which prepared kernel row / column a stage / tap reads, and what the
//     epilogue does with a sum.
//   * All three, csrc/conv5x5_half.hip included: the grid decode, the accumulator-register -> pixel map of a 32 x 32 block
//     and the lane rotation that goes with it, the decode + gather of a weight-prepare unit, the planar <-> channels-last
//     repack, the host-side shape and stride rules, the descriptor of a tensor's tail, the matrix instruction.
// The wgrad kernels of conv5x5_grad.hip and the half kernel's main loop are other plans: they take the constants and the
// small helpers only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sbmc_hip.h"
#include "common.hpp"

namespace sbmc {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using h8 = __attribute__((ext_vector_type(8))) _Float16;

constexpr int C5_TS = 16;                     // tile side (output pixels)
constexpr int C5_PS = C5_TS + 4;              // patch side
constexpr int C5_PP = C5_PS * C5_PS;          // patch pixels (400)
constexpr int C5_PR = C5_PP + 2;              // entries of one (plane, octet) region: 2 C5_PR = 4 (mod 8), so that the two
                                              // octets a pair of staging lanes writes fall into different halves of 128 B
constexpr int C5_ABUF = 2 * 2 * C5_PR;        // 16-byte entries of one patch chunk: [plane 2][octet 2][pixel]
constexpr int C5_NT = 128;                    // output channels of a tile
constexpr int C5_WSTAGE = 5 * 2 * 2 * C5_NT;  // 16-byte entries of one weight stage: [kx 5][plane 2][k half 2][cout 128]
constexpr unsigned C5_LDS_BYTES = (2 * C5_ABUF + 2 * C5_WSTAGE) * 16;      // 133376 of the CU's 163840
constexpr int C5_AROUNDS = (2 * C5_PP + 255) / 256;                        // staging rounds of (pixel, octet) units
constexpr int C5_WROUNDS = C5_WSTAGE / 256;                                // 10 entries of a stage per thread
constexpr unsigned C5_OOB = 0xFFFFFFF0u;
constexpr long long C5_MAXOFF = 0x7FFFFFF0ll;

// a descriptor over `bytes` bytes from a wave-uniform base: offsets from `bytes` up read zero / are not written
__device__ __forceinline__ rsrc_t c5_rsrc(const void* base, long long bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    void* u = reinterpret_cast<void*>(((uintptr_t)hi << 32) | lo);
    const unsigned range = (unsigned)(bytes < 0 ? 0 : (bytes > C5_MAXOFF ? C5_MAXOFF : bytes));
    return __builtin_amdgcn_make_buffer_rsrc(u, 0, __builtin_amdgcn_readfirstlane(range), 0x00020000);
}

__device__ __forceinline__ f32x16 c5_mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

static inline int c5_pad16(int c) { return (c + 15) / 16 * 16; }

// ---- host-side rules, each written once ----
// the shape line of every 5 x 5 entry point
static inline bool c5_shape_ok(int n, int h, int w, int cin, int cout) {
    return n >= 1 && h >= 5 && w >= 5 && cin >= 1 && cout >= 1 && cin <= (1 << 20) && cout <= (1 << 20);
}
// a channels-last buffer's channel stride for c channels
static inline bool c5_ld_ok(int ld, int c) { return ld >= c && ld % 16 == 0 && ld <= (1 << 20); }
// byte offsets inside rows_in rows of the tensor a kernel reads (w_in pixels of ld_in elements a row) and rows_out rows of
// the one it writes stay below 2^31: the rows one descriptor spans
static inline bool c5_strides_ok(int rows_in, long long w_in, long long ld_in, int rows_out, long long w_out, long long ld_out,
                                 int esize) {
    return rows_in * w_in * ld_in * esize < C5_MAXOFF && rows_out * w_out * ld_out * esize < C5_MAXOFF;
}

// ---- the tile of a workgroup: output-channel tiles of one pixel tile are neighbours in the grid (they read the same
// patch through L2) ----
struct C5Tile { int ct, x0, y0, n; };
template <int TY, int TX>
__device__ __forceinline__ C5Tile c5_tile(unsigned t, int nct, int tiles_x, int tiles_y) {
    C5Tile o;
    o.ct = (int)(t % (unsigned)nct);
    t /= (unsigned)nct;
    o.x0 = (int)(t % (unsigned)tiles_x) * TX;
    t /= (unsigned)tiles_x;
    o.y0 = (int)(t % (unsigned)tiles_y) * TY;
    o.n = (int)(t / (unsigned)tiles_y);
    return o;
}

// Row i of a 32 x 32 block is pixel (i / 16, column) of the block's 2 rows x 16 columns.  ds_read_b128 serves lanes
// {0-3, 12-15, 20-27} (and so on) together: with the patch rows 20 entries apart, the second row's lanes are rotated
// by 20 mod 16 = 4 columns so that every such group covers 16 different 16-byte slots: lane 16 + j reads column
// (j + 12) mod 16.
__device__ __forceinline__ int c5_pcol(int l31) { return (l31 + 12 * (l31 >> 4)) & 15; }
// accumulator register r of a 32 x 32 block: row (r & 3) + 8 (r >> 2) + 4 (lane / 32) of the block = pixel
// (r >> 3, rotated column) of its 2 rows x 16 columns; output channel lane % 32
__device__ __forceinline__ int c5_acc_row(int r) { return r >> 3; }
__device__ __forceinline__ int c5_acc_col(int r, int lhi) { return ((r & 3) + 8 * ((r >> 2) & 1) + 4 * lhi + 12 * (r >> 3)) & 15; }

// =====================================================================================================================
// The fp32 implicit-GEMM tile (forward and data gradient).  The A side is the tensor the patches come from (the forward's
// x, the data gradient's gz), the Y side the one the tile is written to.
struct Conv5Params {
    const float* a;          // [N, Ha, Wa, lda]
    const u32x4* wp;         // prepared weights: [Y-channel tile][K16][ky][kx][plane][k half][128] entries of 8 halves
    float* y;                // [N, Hy, Wy, ldy]
    const unsigned* amag;    // bit pattern of max |a|
    const float* wscale;     // the weights' scale
    const float* aux;        // forward: bias [Cout]; data gradient: the saved activation [N, Hy, Wy, ldy] or nullptr
    unsigned* amax;          // raised to the bit pattern of max |y| (a word zeroed by the caller); or nullptr
    int N, Ha, Wa, Hy, Wy, lda, ldy, Cout;
    int K16;                 // chunks of 16 A channels
    int tiles_x, tiles_y, nct;
    float slope;             // 1: linear, 0: ReLU, else LeakyReLU (the data gradient: act' below zero)
};

// The two Sides of conv5x5_gemm_body.inc.  The body is INCLUDED in each kernel, not called: as a __forceinline__ function
// template (parameters by value, every Side hook inlined) the same text compiled to another schedule of the same
// instructions -- the chunk loop 9 instructions shorter -- and the forward measured 0.4-0.7 % slower on every layer; through
// a reference to the parameters the epilogue's 128 `st ? offset : sentinel` selects became branches (1.5 %).  Included, the
// forward's listing is the one the kernel had when the body stood in conv5x5.hip.
struct Conv5Fwd { static constexpr bool mirror = false; };
struct Conv5Dgrad { static constexpr bool mirror = true; };
// The launch both Sides share (the caller has checked the shapes and filled p).
template <typename Kernel>
static int conv5_gemm_launch(Kernel kernel, const Conv5Params& p, void* stream) {
    const unsigned grid = (unsigned)((long long)p.N * p.tiles_y * p.tiles_x * p.nct);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)C5_LDS_BYTES);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), C5_LDS_BYTES, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

// =====================================================================================================================
// Weights [cout][cin][5][5] (any strides) in stage order, zero-padded: unit u = ((((ct K16 + k16) 5 + ky) 5 + kx) 2 + khalf)
// 128 + co is input channels 16 k16 + 8 khalf .. + 7 of output channel 128 ct + co at tap (ky, kx); channels beyond cin /
// cout: zeros.  What a prepare kernel makes of the 8 values (two scaled planes, one rounding to half) is its own.
struct Prep5Src {
    const float* w;
    long s_co, s_ci, s_ky, s_kx;
    int cout, cin, K16, ncot;
};
struct Prep5Unit { int ct, k16, ky, kx, khalf, co; float v[8]; };
__host__ __device__ inline long prep5_units(const Prep5Src& p) { return (long)p.ncot * p.K16 * 25 * 2 * C5_NT; }
static inline Prep5Src prep5_src(const float* w, long s_co, long s_ci, long s_ky, long s_kx, int cin, int cout) {
    return Prep5Src{w, s_co, s_ci, s_ky, s_kx, cout, cin, c5_pad16(cin) / 16, (cout + C5_NT - 1) / C5_NT};
}
__device__ __forceinline__ Prep5Unit prep5_unit(const Prep5Src& p, long u) {
    Prep5Unit o;
    o.co = (int)(u % C5_NT);
    long r = u / C5_NT;
    o.khalf = (int)(r % 2);
    r /= 2;
    o.kx = (int)(r % 5);
    r /= 5;
    o.ky = (int)(r % 5);
    r /= 5;
    o.k16 = (int)(r % p.K16);
    o.ct = (int)(r / p.K16);
    const int oc = o.ct * C5_NT + o.co, ic0 = o.k16 * 16 + o.khalf * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        o.v[i] = (oc < p.cout && ic0 + i < p.cin)
                     ? p.w[(long)oc * p.s_co + (long)(ic0 + i) * p.s_ci + o.ky * p.s_ky + o.kx * p.s_kx] : 0.f;
    return o;
}

// =====================================================================================================================
// Planar [n][c][hw] (S) <-> channels-last [n][hw][ld] (D when TO_NHWC, else the source) with zeros in the channels from c
// up: tiles of 64 pixels x 32 channels through LDS, 64-pixel rows on the planar side, 32-channel rows on the other.
template <typename S, typename D, bool TO_NHWC>
__global__ __launch_bounds__(256) void repack5_kernel(const S* __restrict__ src, D* __restrict__ dst, int c, int ld, long hw,
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
    if (TO_NHWC) {
        const S* planar = src + n * (long)c * hw;
        D* nhwc = dst + n * hw * ld;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cl = (tid >> 6) + 4 * i, px = tid & 63;
            tile[cl][px] = (c0 + cl < c && p0 + px < hw) ? (float)planar[(long)(c0 + cl) * hw + p0 + px] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int px = (tid >> 5) + 8 * i, cl = tid & 31;
            if (p0 + px < hw && c0 + cl < ld) nhwc[(p0 + px) * ld + c0 + cl] = (D)tile[cl][px];
        }
    } else {
        const S* nhwc = src + n * hw * ld;
        D* planar = dst + n * (long)c * hw;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int px = (tid >> 5) + 8 * i, cl = tid & 31;
            tile[cl][px] = (p0 + px < hw && c0 + cl < c) ? (float)nhwc[(p0 + px) * ld + c0 + cl] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cl = (tid >> 6) + 4 * i, px = tid & 63;
            if (c0 + cl < c && p0 + px < hw) planar[(long)(c0 + cl) * hw + p0 + px] = (D)tile[cl][px];
        }
    }
}

// (pointers aligned to their element: 4 bytes for float, 2 for half)
template <typename S, typename D, bool TO_NHWC>
static int repack5(const S* src, D* dst, int ld, int n, int c, long hw, void* stream) {
    if (n < 0 || c < 1 || hw < 0 || !c5_ld_ok(ld, c)) return SBMC_HIP_EINVAL;
    if (n == 0 || hw == 0) return 0;
    if (!src || !dst || (uintptr_t)src % sizeof(S) || (uintptr_t)dst % sizeof(D)) return SBMC_HIP_EINVAL;
    // (the channels-last side is covered up to ld: the packing writes its zeros)
    const int ctiles = ((TO_NHWC ? ld : c) + 31) / 32;
    const long ptiles = (hw + 63) / 64;
    const long long blocks = (long long)n * ptiles * ctiles;
    if (blocks >= 0x7FFFFFFFll) return SBMC_HIP_EINVAL;
    hipLaunchKernelGGL((repack5_kernel<S, D, TO_NHWC>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, c, ld,
                       hw, ctiles, ptiles);
    return (int)hipGetLastError();
}

}  // namespace sbmc
