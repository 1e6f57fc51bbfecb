// tone_dev.h -- the tones of a decoded message, re-encoded from its a91 (ft8_encode of ft8_lib encode.c: encode174, the Gray map,
// the Costas arrays), for the kernels that rebuild a record's signal: the mask of multipass.hip, refine.hip, subtract.hip.
// The record loop of record_dev.h (ft8_messages_kernel, ft8_append_kernel) encodes a whole codeword at once, in its own form,
// with the Gray and Costas constants defined here.
#pragma once
#include "ft8gpu_internal.h"

namespace {

constexpr uint32_t kGrayPacked = 0u | 1u << 3 | 3u << 6 | 2u << 9 | 5u << 12 | 6u << 15 | 4u << 18 | 7u << 21;   // {0,1,3,2,5,6,4,7}
constexpr uint32_t kCostasPacked = 3u | 1u << 3 | 4u << 6 | 0u << 9 | 6u << 12 | 5u << 15 | 2u << 18;           // {3,1,4,0,6,5,2}

// bit i (MSB first) of the 174-bit codeword of a91 = (w0, w1, w2): the 91 message bits, then the 83 parity bits
// (parity of a91 & generator row i - 91, ft8_encode's encode174)
__device__ __forceinline__ uint32_t codeword_bit(uint32_t w0, uint32_t w1, uint32_t w2, const MsgTables *__restrict__ tab, int i) {
    if (i < kLdpcK) {
        const uint32_t w = i < 32 ? w0 : (i < 64 ? w1 : w2);
        return (w >> (31 - (i & 31))) & 1u;
    }
    const int m = i - kLdpcK;
    return (uint32_t)__popc((w0 & tab->gen[m][0]) ^ (w1 & tab->gen[m][1]) ^ (w2 & tab->gen[m][2])) & 1u;
}

// tone of symbol k (0..78) of the message whose a91 dwords (little-endian, as stored in a record) are a0..a2
__device__ __forceinline__ uint32_t tone_of_symbol(uint32_t a0, uint32_t a1, uint32_t a2, const MsgTables *__restrict__ tab, int k) {
    if (k < 7) return (kCostasPacked >> (3 * k)) & 7u;
    if (k >= 36 && k < 43) return (kCostasPacked >> (3 * (k - 36))) & 7u;
    if (k >= 72) return (kCostasPacked >> (3 * (k - 72))) & 7u;
    const uint32_t w0 = __builtin_bswap32(a0), w1 = __builtin_bswap32(a1), w2 = __builtin_bswap32(a2) & 0xFFFFFFE0u;
    const int d = k < 36 ? k - 7 : k - 14;                                   // data symbol 0..57
    const uint32_t v = codeword_bit(w0, w1, w2, tab, 3 * d) << 2 | codeword_bit(w0, w1, w2, tab, 3 * d + 1) << 1 |
                       codeword_bit(w0, w1, w2, tab, 3 * d + 2);
    return (kGrayPacked >> (3 * v)) & 7u;
}

}  // namespace
