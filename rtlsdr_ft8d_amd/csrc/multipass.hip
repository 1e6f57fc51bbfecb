// multipass.hip -- decoding again after the decoded signals are masked out of the waterfall (ft8gpu_decode_messages_passes,
// ft8gpu_mask_messages, ft8gpu_append_messages; DESIGN.md "Multi-pass decoding").
//
// Three kernels:
//   ft8_mask_kernel         one workgroup per frame: copies the frame's waterfall (16-byte lane loads) into its output slot,
//                           then, after a barrier, sets the cell under every symbol of every record to be masked to the
//                           noise baseline of the cell's column; one lane per (record, symbol) re-encodes that symbol's tone
//                           from a91.  In the compacting form the output slot is rank(f), the frame's place among the frames
//                           that gained records in the last pass, and the kernel writes the slot -> frame map and their count.
//   ft8_append_kernel       one wave per frame: the frame's existing records seed the dedup table, then the leader loop of
//                           the messages kernel over this pass's candidates appends every new message behind them.
//   ft8_pass_counts_kernel  copies the counts after a pass into the per-pass count table.
// The record loop (fetch and gate, dedup, tone encoder, SNR estimate, record layout) is the one ft8_messages_kernel runs:
// record_dev.h holds it once, and the append kernel is its seeded instance.
#include "record_dev.h"

namespace {

constexpr int kMaskThreads = 256;

// ---- mask (and compact) ---------------------------------------------------------------------------------------------
// compact == 0 (ft8gpu_mask_messages): out[f] = mag[f] with the cells of records [first[f], n_msgs[f]) replaced.
// compact != 0 (the pass pipeline, mag = the first pass's waterfall): a frame is active when it gained records in the last
// pass (first[f] < n_msgs[f], first = the counts before that pass) and has room for more (n_msgs[f] < 50); the active
// frames, in frame order, get out[rank] = mag[f] with the cells of ALL their records [0, n_msgs[f]) replaced -- which is
// the last pass's waterfall masked with the new records, because a replaced cell always takes the baseline of its
// column -- and map[rank] = f; *n_active = the number of active frames.
__global__ __launch_bounds__(kMaskThreads)
void ft8_mask_kernel(const uint8_t *__restrict__ mag, const uint8_t *__restrict__ base, const ft8gpu_message *__restrict__ msgs,
                     const int32_t *__restrict__ first, const int32_t *__restrict__ n_msgs, const MsgTables *__restrict__ tab,
                     int nframes, int compact, uint8_t *__restrict__ out, int32_t *__restrict__ map, int32_t *__restrict__ n_active) {
    __shared__ int s_rank;
    const int frame = blockIdx.x;
    const int t = threadIdx.x;
    const int nf = n_msgs[frame];
    const int hi = nf < 0 ? 0 : (nf > kMaxMessages ? kMaxMessages : nf);
    int lo, slot = frame;
    if (compact) {
        auto active = [&](int f) { const int n = n_msgs[f]; return first[f] < n && n < kMaxMessages; };
        // rank = #{active frames before this one}: a workgroup-wide count (LDS atomics; the sum does not depend on their order)
        if (t == 0) s_rank = 0;
        __syncthreads();
        int below = 0;
        for (int f = t; f < frame; f += kMaskThreads) below += active(f) ? 1 : 0;
        if (below) atomicAdd(&s_rank, below);
        __syncthreads();
        const int rank = s_rank;
        const bool me = active(frame);
        if (t == 0) {
            if (me) map[rank] = frame;
            if (frame == nframes - 1) *n_active = rank + (me ? 1 : 0);
        }
        if (!me) return;                                                    // workgroup-uniform
        slot = rank;
        lo = 0;
    } else {
        const int f0 = first[frame];
        lo = f0 < 0 ? 0 : (f0 > kMaxMessages ? kMaxMessages : f0);
    }

    const uint4 *src = reinterpret_cast<const uint4 *>(mag + (size_t)frame * kMagArray);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)slot * kMagArray);
    for (int i = t; i < kMagArray / 16; i += kMaskThreads) dst[i] = src[i];
    __syncthreads();                                                        // the copy is in place before any masked cell

    // one lane per (record, symbol); two records may hit one cell, and then both write the same baseline byte
    const ft8gpu_message *fm = msgs + (size_t)frame * kMaxMessages;
    const uint8_t *fbase = base + (size_t)frame * kColumns;
    uint8_t *fo_mag = out + (size_t)slot * kMagArray;
    const int cells = (hi > lo ? hi - lo : 0) * FT8GPU_NN;
    for (int i = t; i < cells; i += kMaskThreads) {
        const int r = lo + i / FT8GPU_NN, k = i % FT8GPU_NN;
        const uint32_t *rec = reinterpret_cast<const uint32_t *>(fm + r);
        const uint32_t c0 = rec[10], c1 = rec[11];                          // cand: score | time_offset, freq_offset | subs
        const int time_offset = (int16_t)(c0 >> 16);
        const int freq_offset = (int16_t)(c1 & 0xFFFFu);
        const int time_sub = (int)((c1 >> 16) & 1u), freq_sub = (int)((c1 >> 24) & 1u);
        const int blk = time_offset + k;
        if (blk < 0 || blk >= kNumBlocks) continue;
        const int fo = freq_offset < 0 ? 0 : (freq_offset > kNumBin - 8 ? kNumBin - 8 : freq_offset);   // as the SNR estimate reads it
        const int bin = fo + (int)tone_of_symbol(rec[12], rec[13], rec[14], tab, k);
        fo_mag[blk * kBlockStride + time_sub * (2 * kNumBin) + freq_sub * kNumBin + bin] = fbase[freq_sub * kNumBin + bin];
    }
}

// ---- append ---------------------------------------------------------------------------------------------------------
// slot s of the pass (its waterfall mag[s], candidates, statuses) belongs to frame map[s] (map == nullptr: frame s), whose
// baseline, records and count are base / msgs / n_msgs[frame]: the signal is summed in this pass's waterfall, the noise is
// the first pass's baseline
__global__ __launch_bounds__(256)
void ft8_append_kernel(const uint8_t *__restrict__ mag, const uint8_t *__restrict__ base,
                       const ft8gpu_candidate *__restrict__ cands, const int32_t *__restrict__ counts,
                       const ft8gpu_decode_status *__restrict__ status, const MsgTables *__restrict__ tab,
                       const int32_t *__restrict__ map, int nslots, int max_candidates, int min_score,
                       ft8gpu_message *__restrict__ msgs, int32_t *__restrict__ n_msgs) {
    record_body<true>(mag, base, cands, counts, status, tab, map, nslots, max_candidates, min_score, msgs, n_msgs);
}

// nbp[f][col] = n_msgs[f] for col in [col0, passes)
__global__ __launch_bounds__(256)
void ft8_pass_counts_kernel(const int32_t *__restrict__ n_msgs, int32_t *__restrict__ nbp, int nframes, int passes, int col0) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nframes) return;
    const int32_t v = n_msgs[f];
    for (int col = col0; col < passes; ++col) nbp[(size_t)f * passes + col] = v;
}

}  // namespace

hipError_t launch_mask(const uint8_t *mag, const uint8_t *base, const ft8gpu_message *msgs, const int32_t *first,
                       const int32_t *n_msgs, const MsgTables *tab, int nframes, int compact, uint8_t *out,
                       int32_t *map, int32_t *n_active, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_mask_kernel, dim3(nframes), dim3(kMaskThreads), 0, s,
                       mag, base, msgs, first, n_msgs, tab, nframes, compact, out, map, n_active);
    return hipGetLastError();
}

hipError_t launch_append(const uint8_t *mag, const uint8_t *base, const ft8gpu_candidate *cands, const int32_t *counts,
                         const ft8gpu_decode_status *status, const MsgTables *tab, const int32_t *map, int nslots,
                         int max_candidates, int min_score, ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s) {
    if (nslots < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_append_kernel, dim3((nslots + 3) / 4), dim3(256), 0, s,
                       mag, base, cands, counts, status, tab, map, nslots, max_candidates, min_score, msgs, n_msgs);
    return hipGetLastError();
}

hipError_t launch_pass_counts(const int32_t *n_msgs, int32_t *nbp, int nframes, int passes, int col0, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_pass_counts_kernel, dim3((nframes + 255) / 256), dim3(256), 0, s, n_msgs, nbp, nframes, passes, col0);
    return hipGetLastError();
}
