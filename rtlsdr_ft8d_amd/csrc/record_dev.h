// record_dev.h -- the per-frame loop of the messages path, kept once: one wave per frame, lane = candidate, 64 candidates at a
// time; the dedup of dedup_dev.h, then every new message re-encodes its 79 tones from a91, sums the power under them, takes
// the noise floor beside them and writes its 64-byte record.  ft8_messages_kernel (messages.hip) instantiates it unseeded,
// ft8_append_kernel (multipass.hip) seeded with the frame's records so far.
// The SNR decision is double arithmetic in a fixed order against thresholds built on the host; the library is built
// with -ffp-contract=off, so no step is fused and tests/ft8_spec_messages.py reproduces every byte.
#pragma once
#include "dedup_dev.h"
#include "tone_dev.h"

namespace {

constexpr int kColumns = 2 * kNumBin;          // noise baseline: (freq_sub, bin) per frame; a (block, time_sub) row is 512 bytes

struct RecordWaveLds {
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

// The body of a 256-thread kernel, wave w of workgroup b taking slot 4 b + w.  Slot s of the launch (its waterfall mag[s],
// candidates, statuses, count) belongs to a frame whose baseline, records and count are base / msgs / n_msgs[frame].
// kSeed == false: frame = slot, the table starts empty, and a message behind the 50th is dropped (the reference never
//                 terminates there, rtlsdr_ft8d.c:1465-1523).
// kSeed == true:  frame = map[slot] (map == nullptr: slot), the frame's n_msgs[frame] records so far seed the dedup table,
//                 the new messages go behind them, and the loop ends when 50 is reached.
template <bool kSeed>
__device__ __forceinline__ void record_body(const uint8_t *__restrict__ mag, const uint8_t *__restrict__ base,
                                            const ft8gpu_candidate *__restrict__ cands, const int32_t *__restrict__ counts,
                                            const ft8gpu_decode_status *__restrict__ status, const MsgTables *__restrict__ tab,
                                            const int32_t *__restrict__ map, int nslots, int max_candidates, int min_score,
                                            ft8gpu_message *__restrict__ msgs, int32_t *__restrict__ n_msgs) {
    __shared__ __attribute__((aligned(16))) RecordWaveLds s_all[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slot = blockIdx.x * 4 + wave;
    if (slot >= nslots) return;                                               // wave-uniform
    int frame = slot;
    if constexpr (kSeed) frame = map ? map[slot] : slot;
    RecordWaveLds &L = s_all[wave];

    const ft8gpu_candidate *fc = cands + (size_t)slot * max_candidates;
    const ft8gpu_decode_status *fs = status + (size_t)slot * max_candidates;
    const uint8_t *fmag = mag + (size_t)slot * kMagArray;
    const uint8_t *fbase = base + (size_t)frame * kColumns;
    ft8gpu_message *out = msgs + (size_t)frame * kMaxMessages;
    const int words = (max_candidates + 63) / 64;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int num_candidates = counts[slot];

    int num_decoded = 0;                                                      // wave-uniform
    if constexpr (kSeed) {
        const int n_in = n_msgs[frame];
        const int n0 = n_in < 0 ? 0 : (n_in > kMaxMessages ? kMaxMessages : n_in);
        // the frame's records so far are the dedup table's first n0 entries (n0 <= 50 < 64: one lane each)
        if (lane < n0) {
            const uint32_t *r = reinterpret_cast<const uint32_t *>(out + lane);
            uint32_t t[kTextDw];
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) t[k] = r[k];
            t[kTextDw - 1] &= 0xFFu;                                          // text[24]; bytes 25.. are snr_db and score
            canonical_text(t);
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) L.ttext[lane][k] = t[k];
            L.thash[lane] = (uint16_t)(r[9] & 0xFFFFu);
        }
        wave_lds_sync();
        num_decoded = n0;
    }

    for (int w = 0; w < words && (!kSeed || num_decoded < kMaxMessages); ++w) {   // :1465, candidate order
        const int idx = w * 64 + lane;
        uint64_t cand_bits = 0;
        uint32_t rec[12] = {};                                                // the 48-byte status record
        if (idx < max_candidates) {
            cand_bits = reinterpret_cast<const uint64_t *>(fc)[idx];
            const uint32_t *r = reinterpret_cast<const uint32_t *>(fs + idx);
#pragma unroll
            for (int k = 1; k < 12; ++k) rec[k] = r[k];
        }
        const bool ok = idx < num_candidates && (int16_t)(cand_bits & 0xFFFFu) >= min_score && ((rec[2] >> 8) & 0xFFu) != 0;   // :1467, :1476-1485
        const unsigned long long live = __ballot(ok);
        if (live == 0ull) continue;                                           // wave-uniform
        uint32_t my_hash = 0;
        uint32_t raw[kTextDw] = {}, mine[kTextDw] = {};                       // the text as unpacked, and canonical
        if (ok) {
            my_hash = rec[1] & 0xFFFFu;                                       // crc_extracted = message.hash
            L.chash[lane] = (uint16_t)my_hash;
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) {
                raw[k] = (rec[5 + k] >> 16) | ((k + 1 < 7 ? rec[6 + k] : 0u) << 16);
                if (k == kTextDw - 1) raw[k] &= 0xFFu;                        // text[24] only (byte 47 is the record's pad)
                mine[k] = raw[k];
            }
            canonical_text(mine);
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) L.ctext[lane][k] = mine[k];
        }
        wave_lds_sync();

        const unsigned long long fresh = dedup_chunk(ok, my_hash, mine, lane, num_decoded, L.thash, L.ttext, L.chash, L.ctext);
        const int rank = num_decoded + __popcll(fresh & below);               // position among the frame's unique messages
        const bool keep = ((fresh >> lane) & 1ull) != 0ull && rank < kMaxMessages;   // table full: drop
        if (keep) {
#pragma unroll
            for (int k = 0; k < kTextDw; ++k) L.ttext[rank][k] = mine[k];
            L.thash[rank] = (uint16_t)my_hash;

            const int score = (int16_t)(cand_bits & 0xFFFFu);
            const int time_offset = (int16_t)((cand_bits >> 16) & 0xFFFFu);
            const int freq_offset = (int16_t)((cand_bits >> 32) & 0xFFFFu);
            const int time_sub = (int)((cand_bits >> 48) & 0xFFu), freq_sub = (int)((cand_bits >> 56) & 0xFFu);

            // a91 = status bytes 10..21 (little-endian dwords), and as MSB-first words for the encoder (91 bits)
            const uint32_t a0 = (rec[2] >> 16) | (rec[3] << 16), a1 = (rec[3] >> 16) | (rec[4] << 16), a2 = (rec[4] >> 16) | (rec[5] << 16);
            uint32_t cw[6];
            cw[0] = __builtin_bswap32(a0);
            cw[1] = __builtin_bswap32(a1);
            cw[2] = __builtin_bswap32(a2) & 0xFFFFFFE0u;
            // 83 parity bits: parity of (a91 & generator row m), ft8_encode's encode174 (rtlsdr_ft8d.c:934)
            uint32_t par[3] = { 0u, 0u, 0u };
#pragma unroll
            for (int m = 0; m < kLdpcM; ++m) {
                const uint32_t x = (cw[0] & tab->gen[m][0]) ^ (cw[1] & tab->gen[m][1]) ^ (cw[2] & tab->gen[m][2]);
                par[m >> 5] |= ((uint32_t)__popc(x) & 1u) << (31 - (m & 31));
            }
            cw[2] |= par[0] >> 27;                                           // codeword bits 91..173
            cw[3] = (par[0] << 5) | (par[1] >> 27);
            cw[4] = (par[1] << 5) | (par[2] >> 27);
            cw[5] = par[2] << 5;

            // signal: power under the 79 tones over the symbols inside the slot's waterfall, summed in order in double
            const int fo = freq_offset < 0 ? 0 : (freq_offset > kNumBin - 8 ? kNumBin - 8 : freq_offset);   // find_sync's range [0, 248]
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
                    const int d = k < 36 ? k - 7 : k - 14;                    // data symbol 0..57
                    tone = (kGrayPacked >> (3 * bits3(cw, 3 * d))) & 7u;
                }
                const int blk = time_offset + k;
                if (blk >= 0 && blk < kNumBlocks) {
                    S = S + tab->power[cell[blk * kBlockStride + (int)tone]];
                    ++nsym;
                }
            }
            // noise: lower median of the frame's baseline in the 50 Hz on either side of the signal's 8 bins
            const uint8_t *brow = fbase + (freq_sub & 1) * kNumBin;
            uint32_t nv[32];
            int n = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int j = i < 16 ? fo - 16 + i : fo + 8 + (i - 16);
                const bool in = j >= 0 && j < kNumBin;
                nv[i] = in ? (uint32_t)brow[in ? j : 0] : 256u;              // 256: outside, never below any threshold
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
            // snr_db = the largest d with S >= (nsym * P[nb]) * T[d]
            const double floor_sum = (double)nsym * tab->power[nb];
            int snr = kSnrMin;
            for (int d = 0; d < kSnrSteps; ++d)
                if (S >= floor_sum * tab->thr[d]) snr = kSnrMin + d;

            const float freq_hz = (freq_offset + (float)freq_sub / 2) * 6.25f;   // :1470
            const float dt_s = (time_offset + (float)time_sub / 2) / 6.25f;      // :1471
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
        num_decoded += __popcll(__ballot(keep));                              // :1520
        wave_lds_sync();                                                      // staging rows are rewritten by the next 64
    }
    if (lane == 0) n_msgs[frame] = num_decoded;                               // :1523
}

}  // namespace
