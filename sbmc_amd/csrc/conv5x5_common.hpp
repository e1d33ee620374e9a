// What csrc/conv5x5.hip (forward) and csrc/conv5x5_grad.hip (data and weight gradients) share: the tile constants of the
// 16 x 16 pixels x 128 channels plan, the descriptor of a tensor's tail, the matrix instruction.
#pragma once
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

}  // namespace sbmc
