// match.hip -- the candidates belief propagation gives up on, compared with the messages a receiver expects from earlier
// slots (include/ft8gpu.h "expected messages", DESIGN.md "Expected messages").  Not part of the reference's path.  The rule is
// exact (integers and float comparisons), restated in tests/ft8_spec_match.py: soft bits, hard decision h and 8-bit weights
// as ordered-statistics decoding forms them (osd.hip); every live entry of the receiver's table is a full 77-bit hypothesis,
// its codeword c_j is compared with h, the entry with the smallest (metric, index) is judged: all-zero, hard errors, unpack77.
//
//   ft8_expect_encode_kernel  one lane per table entry, once per frame and call: CRC-14 and the 83 generator parities of the
//                             payload, the codeword as six dwords in position order, and per round of 64 entries the mask
//                             of the live ones (used != 0, not expired at the state's slot).
//   ft8_match_kernel          one wave64 per candidate, four per workgroup, the launch geometry of the LDPC kernel (its head
//                             is a copy of cand_dev.h's, the kernel says why).  Lanes are table entries: 512
//                             entries are eight rounds of 64, and a round without a live entry is skipped on the scalar
//                             side.  h and the weights are wave-uniform: three 64-bit words and eight bit planes of three
//                             words (ballots, SGPRs), so the metric of an entry is 24 and / popcount pairs on its c_j ^ h
//                             instead of 174 table steps.  metric << 9 | index through one butterfly minimum is the best
//                             entry with the rule's tie break.  The soft bits and the epilogue -- unpack77 on two 64-bit
//                             words, the 48-byte record of a BP success composed in LDS -- are the shared device code of
//                             cand_dev.h.
//   ft8_expect_update_kernel  the update rule, one wave per receiver with its table in LDS (8 KB): a receiver is a strictly
//                             sequential walk over its slots and records; an insert first looks for its 77 bits (eight
//                             entries per lane, ballots, the smallest index), then refreshes that entry or overwrites the
//                             one under the cursor.
#include "match.h"
#include "cand_dev.h"

namespace {

constexpr int kOffRec = 192;                           // dwords: 174 soft bits, then the record
constexpr int kMatchLds = kOffRec + 12;
constexpr int kIdxBits = 9;                            // 512 entries; metric <= 174 * 255 < 2^16
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;
static_assert(kExpectEntries == 1 << kIdxBits, "the key holds a table index in its low bits");
static_assert(sizeof(ft8gpu_expect_entry) == 16 && sizeof(ft8gpu_expect_state) == 8208, "table layout");

// the 77 payload bits of a table entry (or of a91) as two words, MSB first: bits 0..63, and bits 64..76 at the top
__device__ __forceinline__ void payload_words(uint32_t x, uint32_t y, uint32_t z, uint64_t &w0, uint64_t &w1) {
    w0 = (uint64_t)__builtin_bswap32(x) << 32 | __builtin_bswap32(y);
    w1 = (uint64_t)(__builtin_bswap32(z) & 0xFFF80000u) << 32;
}

__global__ __launch_bounds__(256)
void ft8_expect_encode_kernel(const ft8gpu_expect_state *__restrict__ states, uint32_t max_age,
                              const MsgTables *__restrict__ tab, uint32_t *__restrict__ cw, uint64_t *__restrict__ live) {
    const int frame = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const ft8gpu_expect_state *st = states + frame;
    const uint4 ent = reinterpret_cast<const uint4 *>(st->entry)[e];
    const uint32_t slot = st->slot;
    const bool used = ((ent.z >> 16) & 0xFFu) != 0u;
    const bool expired = max_age != 0u && (uint32_t)(slot - ent.w) > max_age;
    uint64_t w0, w1;
    payload_words(ent.x, ent.y, ent.z, w0, w1);
    // CRC-14, polynomial 0x2757, over the 77 bits and five zeros, as ft8_lib's encoder computes it
    uint32_t rem = 0;
    for (int bit = 0; bit < 82; ++bit) {
        const uint32_t b = bit < 64 ? (uint32_t)(w0 >> (63 - bit)) & 1u : (uint32_t)(w1 >> (127 - bit)) & 1u;
        rem ^= b << 13;
        rem = (rem & 0x2000u) ? ((rem << 1) ^ 0x2757u) & 0x3FFFu : (rem << 1) & 0x3FFFu;
    }
    w1 |= (uint64_t)rem << 37;                                        // bits 77..90
    // position order: position p at bit p & 63 of word p >> 6
    uint64_t c0 = __brevll(w0), c1 = __brevll(w1), c2 = 0;
    const uint32_t m0 = (uint32_t)(w0 >> 32), m1 = (uint32_t)w0, m2 = (uint32_t)(w1 >> 32);
    for (int m = 0; m < kLdpcM; ++m) {
        const uint64_t par = (uint64_t)((__popc(m0 & tab->gen[m][0]) + __popc(m1 & tab->gen[m][1]) + __popc(m2 & tab->gen[m][2])) & 1);
        const int p = kLdpcK + m;
        if (p < 128) c1 |= par << (p - 64); else c2 |= par << (p - 128);
    }
    uint32_t *out = cw + (size_t)frame * (kExpectEntries * 6) + e;
    out[0 * kExpectEntries] = (uint32_t)c0;
    out[1 * kExpectEntries] = (uint32_t)(c0 >> 32);
    out[2 * kExpectEntries] = (uint32_t)c1;
    out[3 * kExpectEntries] = (uint32_t)(c1 >> 32);
    out[4 * kExpectEntries] = (uint32_t)c2;
    out[5 * kExpectEntries] = (uint32_t)(c2 >> 32);
    const uint64_t mask = __ballot(used && !expired);
    if ((threadIdx.x & 63) == 0) live[(size_t)frame * kExpectRounds + (e >> 6)] = mask;
}

__global__ __launch_bounds__(256)
void ft8_match_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                      const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                      ft8gpu_decode_status *status_out, ft8gpu_match_info *info, int nframes, int max_candidates,
                      const uint32_t *__restrict__ cw_all, const uint64_t *__restrict__ live_all, int max_hard_errors,
                      unsigned blocks_per_frame) {
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[4][kMatchLds];

    // cand_dev.h's cand_prologue, written out: behind the shared routine this kernel's address arithmetic came out a dozen
    // VALU instructions longer (42 registers for 41) and the stage 1 % slower on 4096 frames, whichever way its exits were put
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int frame = (int)(blockIdx.x / blocks_per_frame);
    const int ci = (int)(blockIdx.x - (unsigned)frame * blocks_per_frame) * 4 + wave;
    if (frame >= nframes || ci >= max_candidates) return;
    if (ci >= counts[frame]) return;                                  // wave-uniform: records behind the count are not touched
    const size_t rec_index = (size_t)frame * max_candidates + ci;
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(status_in + rec_index);
    uint32_t *out32 = reinterpret_cast<uint32_t *>(status_out + rec_index);
    uint32_t *info32 = reinterpret_cast<uint32_t *>(info + rec_index);
    static_assert(sizeof(ft8gpu_decode_status) == 48 && sizeof(ft8gpu_match_info) == 8, "record sizes");
    uint32_t mine, dw0;
    if (!read_record(in32, lane, mine, dw0)) {                        // does not qualify
        leave_record(out32, in32, info32, mine, 0u, lane);
        return;
    }

    uint32_t *s = s_mem[wave];
    float cw[3];
    bool has[3];
    if (!soft_bits(mag, frame, cands[rec_index], reinterpret_cast<float *>(s), lane, cw, has)) {      // wave-uniform: nothing is compared
        leave_record(out32, in32, info32, mine, 6u, lane);
        return;
    }

    // ---- the live entries of the frame's table; none: result 0 ----------------------------------------------------------
    const uint64_t *live = live_all + (size_t)frame * kExpectRounds;
    uint64_t lm[kExpectRounds], any = 0ull;
#pragma unroll
    for (int r = 0; r < kExpectRounds; ++r) { lm[r] = live[r]; any |= lm[r]; }
    if (any == 0ull) {
        leave_record(out32, in32, info32, mine, 0u, lane);
        return;
    }

    // ---- hard decisions and weight planes in position order, wave-uniform ----------------------------------------------
    uint64_t H[3], P[8][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        bool hbit;
        int wt;
        hard_and_weight(__float_as_uint(cw[q]), has[q], hbit, wt);
        H[q] = __ballot(hbit);
#pragma unroll
        for (int b = 0; b < 8; ++b) P[b][q] = __ballot((wt >> b) & 1);
    }

    // ---- every live entry: lanes are entries, a round is 64 of them ----------------------------------------------------
    const uint32_t *cwf = cw_all + (size_t)frame * (kExpectEntries * 6);
    uint32_t best = kKeyNone;
#pragma unroll
    for (int r = 0; r < kExpectRounds; ++r) {
        if (lm[r] == 0ull) continue;                                  // wave-uniform
        if ((lm[r] >> lane) & 1ull) {
            const uint32_t *p = cwf + 64 * r + lane;
            uint64_t x[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                x[j] = ((uint64_t)p[(2 * j) * kExpectEntries] | ((uint64_t)p[(2 * j + 1) * kExpectEntries] << 32)) ^ H[j];
            best = min(best, (metric_of(x, P) << kIdxBits) | (uint32_t)(64 * r + lane));
        }
    }
    best = wave_min(best);
    const int index = (int)(best & (uint32_t)(kExpectEntries - 1));
    const uint32_t metric = best >> kIdxBits;

    // ---- the best entry's codeword again (one address for the wave), then the checks ----------------------------------
    uint64_t B[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        B[j] = (uint64_t)cwf[(2 * j) * kExpectEntries + index] | ((uint64_t)cwf[(2 * j + 1) * kExpectEntries + index] << 32);
    const int nhard = __popcll(B[0] ^ H[0]) + __popcll(B[1] ^ H[1]) + __popcll(B[2] ^ H[2]);

    uint32_t *rec32 = s + kOffRec;
    int result;
    if ((B[0] | B[1] | B[2]) == 0ull) result = 5;                     // the code is systematic: an all-zero payload
    else if (nhard > max_hard_errors) result = 2;
    else {
        const uint32_t crc = (uint32_t)(__brevll(B[1]) >> 37) & 0x3FFFu;      // bits 77..90: the CRC is the encoder's own
        result = compose_record(B[0], B[1], dw0, crc, crc, rec32, lane) < 0 ? 4 : 1;
    }
    store_record(out32, in32, rec32, mine, result == 1, lane);
    if (lane == 0) {
        info32[0] = (uint32_t)result | ((uint32_t)nhard << 8) | ((uint32_t)index << 16);
        info32[1] = metric;
    }
}

// ---- the update rule ---------------------------------------------------------------------------------------------------

constexpr uint32_t kZ77 = 0x0000F8FFu;                 // payload bytes 8, 9 in an entry's third dword, bits 77..79 cleared

// insert(P, kind) on the table in LDS; wave-uniform arguments, every lane takes part
__device__ __forceinline__ void table_insert(uint4 *tab, uint32_t &cursor, uint32_t slot, uint32_t x, uint32_t y, uint32_t z77,
                                             uint32_t kind, int lane) {
    int found = -1;
#pragma unroll
    for (int r = 0; r < kExpectRounds; ++r) {
        const uint4 e = tab[64 * r + lane];
        const uint64_t hit = __ballot(((e.z >> 16) & 0xFFu) != 0u && e.x == x && e.y == y && (e.z & kZ77) == z77);
        if (found < 0 && hit != 0ull) found = 64 * r + __builtin_ctzll(hit);
    }
    if (found >= 0) {
        if (lane == 0) {
            uint4 e = tab[found];
            e.z = (e.z & 0x00FFFFFFu) | ((e.z >> 24) & kind) << 24;   // a message once heard stays kind 0
            e.w = slot;
            tab[found] = e;
        }
    } else {
        const uint32_t at = cursor % (uint32_t)kExpectEntries;
        if (lane == 0) tab[at] = make_uint4(x, y, z77 | (1u << 16) | (kind << 24), slot);
        cursor = at + 1u;
    }
    wave_lds_sync();
}

__global__ __launch_bounds__(64)
void ft8_expect_update_kernel(const ft8gpu_message *__restrict__ msgs, const int32_t *__restrict__ n_msgs, int ns,
                              ft8gpu_expect_state *state, int derive) {
    __shared__ uint4 tab[kExpectEntries];
    const int lane = threadIdx.x;
    ft8gpu_expect_state *st = state + blockIdx.x;
    uint4 *entries = reinterpret_cast<uint4 *>(st->entry);
    for (int i = lane; i < kExpectEntries; i += 64) tab[i] = entries[i];
    uint32_t cursor = st->cursor, slot = st->slot;
    wave_lds_sync();

    for (int sl = 0; sl < ns; ++sl, ++slot) {
        const size_t f = (size_t)blockIdx.x * ns + sl;
        int n = n_msgs[f];
        n = n < 0 ? 0 : (n > kMaxMessages ? kMaxMessages : n);
        for (int r = 0; r < n; ++r) {
            const uint4 a = reinterpret_cast<const uint4 *>(msgs + f * kMaxMessages + r)[3];      // a91[12], pad[4]: one address
            const uint32_t x = a.x, y = a.y, z77 = a.z & kZ77;
            table_insert(tab, cursor, slot, x, y, z77, 0u, lane);
            if (!derive) continue;
            uint64_t w0, w1;
            payload_words(x, y, z77, w0, w1);
            const uint32_t n29a = (uint32_t)(w0 >> 35), n29b = (uint32_t)(w0 >> 6) & 0x1FFFFFFFu;
            const int i3 = (int)(w1 >> 51) & 7;
            if (i3 != 1 || (n29a >> 1) < ft8dev::NTOKENS + ft8dev::MAX22 || (n29b >> 1) < ft8dev::NTOKENS + ft8dev::MAX22) continue;
            for (uint32_t g = 32402u; g <= 32404u; ++g) {             // RRR, RR73, 73 with the calls swapped, ir = 0, i3 = 1
                const uint64_t d0 = (uint64_t)n29b << 35 | (uint64_t)n29a << 6 | (g >> 10);
                const uint32_t d1 = ((g & 0x3FFu) << 6) | (1u << 3);  // bits 64..79
                table_insert(tab, cursor, slot, __builtin_bswap32((uint32_t)(d0 >> 32)), __builtin_bswap32((uint32_t)d0),
                             __builtin_bswap32(d1 << 16), 1u, lane);
            }
        }
    }
    for (int i = lane; i < kExpectEntries; i += 64) entries[i] = tab[i];
    if (lane == 0) { st->cursor = cursor; st->slot = slot; }
}

}  // namespace

hipError_t launch_expect_encode(const ft8gpu_expect_state *states, int nframes, uint32_t max_age, const MsgTables *tab,
                                void *work, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    uint32_t *cw = (uint32_t *)work;
    uint64_t *live = (uint64_t *)((char *)work + (size_t)nframes * kExpectCwBytes);
    for (int f0 = 0; f0 < nframes; f0 += 65535) {                     // gridDim.y
        const int n = nframes - f0 < 65535 ? nframes - f0 : 65535;
        hipLaunchKernelGGL(ft8_expect_encode_kernel, dim3(kExpectEntries / 256, (unsigned)n), dim3(256), 0, s, states + f0, max_age, tab,
                           cw + (size_t)f0 * (kExpectEntries * 6), live + (size_t)f0 * kExpectRounds);
    }
    return hipGetLastError();
}

hipError_t launch_match(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                        const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_match_info *info,
                        int nframes, int max_candidates, const void *work, int max_hard_errors, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    CandGrid g;
    if (cand_grid(nframes, max_candidates, g) != hipSuccess) return hipErrorInvalidValue;
    const uint32_t *cw = (const uint32_t *)work;
    const uint64_t *live = (const uint64_t *)((const char *)work + (size_t)nframes * kExpectCwBytes);
    hipLaunchKernelGGL(ft8_match_kernel, dim3(g.nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info,
                       nframes, max_candidates, cw, live, max_hard_errors, g.bpf);
    return hipGetLastError();
}

hipError_t launch_expect_update(const ft8gpu_message *msgs, const int32_t *n_msgs, int nrecv, int ns,
                                ft8gpu_expect_state *state, int derive, hipStream_t s) {
    if (nrecv < 1 || ns < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_expect_update_kernel, dim3((unsigned)nrecv), dim3(64), 0, s, msgs, n_msgs, ns, state, derive);
    return hipGetLastError();
}

hipError_t launch_match_tag(const int32_t *n_before, int stride, const int32_t *n_msgs, int nframes, ft8gpu_message *msgs,
                            hipStream_t s) {
    return launch_tag(nullptr, n_before, stride, n_msgs, nframes, msgs, TagConst<2>{ 1 }, s);    // pad[2] = 1: matched
}
