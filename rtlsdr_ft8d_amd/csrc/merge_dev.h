// merge_dev.h -- the merge of a front end that decodes one input as several frames (the bands of an audio clip, audio.hip; the
// channels of a wide capture, wide.hip), kept once: the parts' records in part order, a record dropped when one already kept
// carries the same a91, freq_hz rebuilt on the input's own bin scale and the part index written into pad[0].
#pragma once
#include "ft8gpu_internal.h"

namespace {

// The records of input c: part_msgs [c][nparts][50] with counts part_n [c][nparts], part b starting at bin bin[b] of the input;
// msgs [c][50 nparts], n_msgs [c].  A record is 16 dwords (float members give 4-byte alignment): a91 = dwords 12 .. 14,
// freq_hz = dword 7, cand.freq_offset / freq_sub = the low half / the top byte of dword 11, pad[0] = the low byte of dword 15.
// kNearOnly: equal a91 makes a duplicate only when the two parts start less than 256 bins apart, that is where their
// spectra can overlap (a record already kept names its part in pad[0]).
template <bool kNearOnly>
__device__ __forceinline__ void merge_parts(const ft8gpu_message *__restrict__ part_msgs, const int32_t *__restrict__ part_n, int c,
                                            int nparts, const int32_t *bin, ft8gpu_message *msgs, int32_t *__restrict__ n_msgs) {
    const int cap = kMaxMessages * nparts;
    uint32_t *dst = (uint32_t *)(msgs + (size_t)c * cap);
    int kept = 0;
    for (int b = 0; b < nparts; ++b) {
        int n = part_n[c * nparts + b];
        n = n < 0 ? 0 : n > kMaxMessages ? kMaxMessages : n;
        const uint32_t *src = (const uint32_t *)(part_msgs + ((size_t)c * nparts + b) * kMaxMessages);
        for (int k = 0; k < n && kept < cap; ++k) {
            const uint32_t *r = src + 16 * k;
            bool dup = false;
            for (int i = 0; i < kept && !dup; ++i) {
                dup = dst[16 * i + 12] == r[12] && dst[16 * i + 13] == r[13] && dst[16 * i + 14] == r[14];
                if constexpr (kNearOnly) {
                    const int apart = bin[b] - bin[dst[16 * i + 15] & 0xffu];
                    dup = dup && apart > -256 && apart < 256;
                }
            }
            if (dup) continue;
            uint32_t *d = dst + 16 * kept;
            for (int i = 0; i < 16; ++i) d[i] = r[i];
            const int fo = (int16_t)(r[11] & 0xffffu);
            const int fs = (int)(r[11] >> 24);
            d[7] = __float_as_uint(((float)(fo + bin[b]) + (float)fs / 2) * 6.25f);
            d[15] = (r[15] & 0xffffff00u) | (uint32_t)b;
            ++kept;
        }
    }
    n_msgs[c] = kept;
}

}  // namespace
