// messages.hip -- the second output path: every unique message of a frame with an SNR estimate, its time offset and its
// frequency (ft8gpu_decode_messages / ft8gpu_collect_messages).  The reference numbers its unique messages at
// rtlsdr_ft8d.c:1487-1520 but keeps only the CQ ones; this path keeps them all, in the same order, up to the same 50.
//
// Two kernels (DESIGN.md "Every decoded message"):
//   ft8_noise_baseline_kernel  per frame and column (freq_sub, bin): the 47th smallest of the column's 184 bytes
//                              (block, time_sub), the 25th percentile over time.  One workgroup per frame, a thread per
//                              column, so every load instruction of a wave reads 64 consecutive bytes of a row.
//   ft8_messages_kernel        one wave per frame, lane = candidate, 64 candidates at a time: the dedup of the spots
//                              kernel (dedup_dev.h), then every new message re-encodes its 79 tones from a91, sums the
//                              power under them, takes the noise floor beside them and writes its 64-byte record.  The
//                              loop is record_dev.h's, which the append kernel of multipass.hip runs too.
#include "record_dev.h"

namespace {

// ---- noise baseline -------------------------------------------------------------------------------------------------
constexpr int kColumnRows = kRowsPerFrame;     // 184 = 92 blocks x 2 time_subs

// #{bytes of w < v} for the four bytes of a packed dword
__device__ __forceinline__ int count_below(uint32_t w, uint32_t v) {
    return (int)((w & 0xFFu) < v) + (int)(((w >> 8) & 0xFFu) < v) + (int)(((w >> 16) & 0xFFu) < v) + (int)((w >> 24) < v);
}

__global__ __launch_bounds__(kColumns)
void ft8_noise_baseline_kernel(const uint8_t *__restrict__ mag, uint8_t *__restrict__ base, int nframes) {
    const int frame = blockIdx.x;
    if (frame >= nframes) return;
    const int c = threadIdx.x;
    const uint8_t *col = mag + (size_t)frame * kMagArray + c;
    uint32_t w[kColumnRows / 4];
#pragma unroll
    for (int q = 0; q < kColumnRows / 4; ++q)
        w[q] = (uint32_t)col[(4 * q) * kColumns] | ((uint32_t)col[(4 * q + 1) * kColumns] << 8) |
               ((uint32_t)col[(4 * q + 2) * kColumns] << 16) | ((uint32_t)col[(4 * q + 3) * kColumns] << 24);
    // The k-th smallest (k = 46) is the largest v with #{x < v} <= k: #{x < v} does not decrease with v, so v is built
    // bit by bit from the top, each bit kept when the count allows it.
    uint32_t v = 0;
#pragma unroll
    for (int bit = 7; bit >= 0; --bit) {
        const uint32_t t = v | (1u << bit);
        int below = 0;
#pragma unroll
        for (int q = 0; q < kColumnRows / 4; ++q) below += count_below(w[q], t);
        if (below <= kBaseRank) v = t;
    }
    base[(size_t)frame * kColumns + c] = (uint8_t)v;
}

// ---- message records: the loop of record_dev.h over a frame's own candidates, the table empty at the start ----------
__global__ __launch_bounds__(256)
void ft8_messages_kernel(const uint8_t *__restrict__ mag, const uint8_t *__restrict__ base,
                         const ft8gpu_candidate *__restrict__ cands, const int32_t *__restrict__ counts,
                         const ft8gpu_decode_status *__restrict__ status, const MsgTables *__restrict__ tab,
                         int nframes, int max_candidates, int min_score,
                         ft8gpu_message *__restrict__ msgs, int32_t *__restrict__ n_msgs) {
    record_body<false>(mag, base, cands, counts, status, tab, nullptr, nframes, max_candidates, min_score, msgs, n_msgs);
}

}  // namespace

hipError_t launch_noise_baseline(const uint8_t *mag, uint8_t *base, int nframes, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_noise_baseline_kernel, dim3(nframes), dim3(kColumns), 0, s, mag, base, nframes);
    return hipGetLastError();
}

hipError_t launch_messages(const uint8_t *mag, const uint8_t *base, const ft8gpu_candidate *cands, const int32_t *counts,
                           const ft8gpu_decode_status *status, const MsgTables *tab, int nframes, int max_candidates,
                           int min_score, ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_messages_kernel, dim3((nframes + 3) / 4), dim3(256), 0, s,
                       mag, base, cands, counts, status, tab, nframes, max_candidates, min_score, msgs, n_msgs);
    return hipGetLastError();
}
