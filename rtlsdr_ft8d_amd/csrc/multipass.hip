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
// The record arithmetic (tone encoder, SNR estimate, record layout) is that of ft8_messages_kernel (messages.hip), copied
// here rather than shared so that the messages kernel's code stays exactly as it is.
#include "dedup_dev.h"
#include "tone_dev.h"

namespace {

constexpr int kColumns = 2 * kNumBin;          // noise baseline: (freq_sub, bin) per frame
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
struct AppendWaveLds {
    uint32_t ctext[64][kTextDw];
    uint32_t ttext[kMaxMessages][kTextDw];
    uint16_t chash[64];
    uint16_t thash[kMaxMessages];
};

// the 3 codeword bits starting at bit k (MSB-first words); k is a compile-time constant after unrolling
__device__ __forceinline__ uint32_t bits3(const uint32_t (&cw)[6], int k) {
    const int wi = k >> 5, o = k & 31;
    if (o <= 29) return (cw[wi] >> (29 - o)) & 7u;
    return ((cw[wi] << (o - 29)) | (cw[wi + 1] >> (61 - o))) & 7u;
}

// slot s of the pass (its waterfall mag[s], candidates, statuses) belongs to frame map[s] (map == nullptr: frame s), whose
// baseline, records and count are base / msgs / n_msgs[frame]
__global__ __launch_bounds__(256)
void ft8_append_kernel(const uint8_t *__restrict__ mag, const uint8_t *__restrict__ base,
                       const ft8gpu_candidate *__restrict__ cands, const int32_t *__restrict__ counts,
                       const ft8gpu_decode_status *__restrict__ status, const MsgTables *__restrict__ tab,
                       const int32_t *__restrict__ map, int nslots, int max_candidates, int min_score,
                       ft8gpu_message *__restrict__ msgs, int32_t *__restrict__ n_msgs) {
    __shared__ __attribute__((aligned(16))) AppendWaveLds s_all[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = blockIdx.x * 4 + wave;
    if (slot >= nslots) return;                                               // wave-uniform
    const int frame = map ? map[slot] : slot;
    AppendWaveLds &L = s_all[wave];

    const ft8gpu_candidate *fc = cands + (size_t)slot * max_candidates;
    const ft8gpu_decode_status *fs = status + (size_t)slot * max_candidates;
    const uint8_t *fmag = mag + (size_t)slot * kMagArray;
    const uint8_t *fbase = base + (size_t)frame * kColumns;
    ft8gpu_message *out = msgs + (size_t)frame * kMaxMessages;
    const int words = (max_candidates + 63) / 64;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int num_candidates = counts[slot];
    const int n_in = n_msgs[frame];
    const int n0 = n_in < 0 ? 0 : (n_in > kMaxMessages ? kMaxMessages : n_in);

    // the frame's records so far are the dedup table's first n0 entries (n0 <= 50 < 64: one lane each)
    if (lane < n0) {
        const uint32_t *r = reinterpret_cast<const uint32_t *>(out + lane);
        uint32_t t[kTextDw];
#pragma unroll
        for (int k = 0; k < kTextDw; ++k) t[k] = r[k];
        t[kTextDw - 1] &= 0xFFu;                                              // text[24]; bytes 25.. are snr_db and score
        canonical_text(t);
#pragma unroll
        for (int k = 0; k < kTextDw; ++k) L.ttext[lane][k] = t[k];
        L.thash[lane] = (uint16_t)(r[9] & 0xFFFFu);
    }
    wave_lds_sync();

    int num_decoded = n0;                                                     // wave-uniform
    for (int w = 0; w < words && num_decoded < kMaxMessages; ++w) {           // candidate order
        const int idx = w * 64 + lane;
        uint64_t cand_bits = 0;
        uint32_t rec[12] = {};                                                // the 48-byte status record
        if (idx < max_candidates) {
            cand_bits = reinterpret_cast<const uint64_t *>(fc)[idx];
            const uint32_t *r = reinterpret_cast<const uint32_t *>(fs + idx);
#pragma unroll
            for (int k = 1; k < 12; ++k) rec[k] = r[k];
        }
        const bool ok = idx < num_candidates && (int16_t)(cand_bits & 0xFFFFu) >= min_score && ((rec[2] >> 8) & 0xFFu) != 0;
        const unsigned long long live = __ballot(ok);
        if (live == 0ull) continue;                                           // wave-uniform
        uint32_t my_hash = 0;
        uint32_t raw[kTextDw] = {}, mine[kTextDw] = {};                       // the text as unpacked, and canonical
        if (ok) {
            my_hash = rec[1] & 0xFFFFu;
            L.chash[lane] = (uint16_t)my_hash;
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) {
                raw[k] = (rec[5 + k] >> 16) | ((k + 1 < 7 ? rec[6 + k] : 0u) << 16);
                if (k == kTextDw - 1) raw[k] &= 0xFFu;
                mine[k] = raw[k];
            }
            canonical_text(mine);
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) L.ctext[lane][k] = mine[k];
        }
        wave_lds_sync();

        const unsigned long long fresh = dedup_chunk(ok, my_hash, mine, lane, num_decoded, L.thash, L.ttext, L.chash, L.ctext);
        const int rank = num_decoded + __popcll(fresh & below);
        const bool keep = ((fresh >> lane) & 1ull) != 0ull && rank < kMaxMessages;
        if (keep) {
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) L.ttext[rank][k] = mine[k];
            L.thash[rank] = (uint16_t)my_hash;

            const int score = (int16_t)(cand_bits & 0xFFFFu);
            const int time_offset = (int16_t)((cand_bits >> 16) & 0xFFFFu);
            const int freq_offset = (int16_t)((cand_bits >> 32) & 0xFFFFu);
            const int time_sub = (int)((cand_bits >> 48) & 0xFFu), freq_sub = (int)((cand_bits >> 56) & 0xFFu);

            const uint32_t a0 = (rec[2] >> 16) | (rec[3] << 16), a1 = (rec[3] >> 16) | (rec[4] << 16), a2 = (rec[4] >> 16) | (rec[5] << 16);
            uint32_t cw[6];
            cw[0] = __builtin_bswap32(a0);
            cw[1] = __builtin_bswap32(a1);
            cw[2] = __builtin_bswap32(a2) & 0xFFFFFFE0u;
            uint32_t par[3] = { 0u, 0u, 0u };
#pragma unroll
            for (int m = 0; m < kLdpcM; ++m) {
                const uint32_t x = (cw[0] & tab->gen[m][0]) ^ (cw[1] & tab->gen[m][1]) ^ (cw[2] & tab->gen[m][2]);
                par[m >> 5] |= ((uint32_t)__popc(x) & 1u) << (31 - (m & 31));
            }
            cw[2] |= par[0] >> 27;
            cw[3] = (par[0] << 5) | (par[1] >> 27);
            cw[4] = (par[1] << 5) | (par[2] >> 27);
            cw[5] = par[2] << 5;

            // signal: power under the 79 tones in this pass's waterfall; noise: the first pass's baseline
            const int fo = freq_offset < 0 ? 0 : (freq_offset > kNumBin - 8 ? kNumBin - 8 : freq_offset);
            const uint8_t *cell = fmag + (time_sub & 1) * (2 * kNumBin) + (freq_sub & 1) * kNumBin + fo;
            double S = 0.0;
            int nsym = 0;
#pragma unroll
            for (int k = 0; k < FT8GPU_NN; ++k) {
                uint32_t tone;
                if (k < 7) tone = (kCostasPacked >> (3 * k)) & 7u;
                else if (k >= 36 && k < 43) tone = (kCostasPacked >> (3 * (k - 36))) & 7u;
                else if (k >= 72) tone = (kCostasPacked >> (3 * (k - 72))) & 7u;
                else {
                    const int d = k < 36 ? k - 7 : k - 14;
                    tone = (kGrayPacked >> (3 * bits3(cw, 3 * d))) & 7u;
                }
                const int blk = time_offset + k;
                if (blk >= 0 && blk < kNumBlocks) {
                    S = S + tab->power[cell[blk * kBlockStride + (int)tone]];
                    ++nsym;
                }
            }
            const uint8_t *brow = fbase + (freq_sub & 1) * kNumBin;
            uint32_t nv[32];
            int n = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int j = i < 16 ? fo - 16 + i : fo + 8 + (i - 16);
                const bool in = j >= 0 && j < kNumBin;
                nv[i] = in ? (uint32_t)brow[in ? j : 0] : 256u;
                n += in ? 1 : 0;
            }
            const int mid = (n - 1) / 2;
            uint32_t nb = 0;
#pragma unroll
            for (int bit = 7; bit >= 0; --bit) {
                const uint32_t t = nb | (1u << bit);
                int cnt = 0;
#pragma unroll
                for (int i = 0; i < 32; ++i) cnt += nv[i] < t ? 1 : 0;
                if (cnt <= mid) nb = t;
            }
            const double floor_sum = (double)nsym * tab->power[nb];
            int snr = kSnrMin;
            for (int d = 0; d < kSnrSteps; ++d)
                if (S >= floor_sum * tab->thr[d]) snr = kSnrMin + d;

            const float freq_hz = (freq_offset + (float)freq_sub / 2) * 6.25f;
            const float dt_s = (time_offset + (float)time_sub / 2) / 6.25f;
            uint32_t o[16];
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = raw[k];
            o[6] = raw[6] | ((uint32_t)(uint8_t)(int8_t)snr << 8) | ((uint32_t)(uint16_t)(int16_t)score << 16);
            o[7] = __float_as_uint(freq_hz);
            o[8] = __float_as_uint(dt_s);
            o[9] = my_hash | ((uint32_t)idx << 16);
            o[10] = (uint32_t)cand_bits;
            o[11] = (uint32_t)(cand_bits >> 32);
            o[12] = a0;
            o[13] = a1;
            o[14] = a2;
            o[15] = 0u;
            uint4 *dst = reinterpret_cast<uint4 *>(out + rank);
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        }
        num_decoded += __popcll(__ballot(keep));
        wave_lds_sync();                                                      // staging rows are rewritten by the next 64
    }
    if (lane == 0) n_msgs[frame] = num_decoded;
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
