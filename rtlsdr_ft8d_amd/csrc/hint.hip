// hint.hip -- call hints: a-priori decoding from the calls a receiver heard in earlier slots (include/ft8gpu.h "call hints",
// DESIGN.md "Call hints").  Not part of the reference's path.  The rule is exact and restated in tests/ft8_spec_hint.py: a
// receiver's table holds call fields (kind 1 "A ? ?", 2 "? B ?", 3 "A B ?"), every candidate BP gives up on ranks the live
// entries by how well its hard decisions agree with them, and the best few are tried by the per-hypothesis rule of a-priori
// decoding (ap.hip).
//
//   ft8_hint_encode_kernel  one lane per table entry, once per frame and call: the live test (used, kind 1..3, not expired at the
//                           state's slot, of the slot's parity) and the entry's bit word over codeword positions 0..57 (two
//                           29-bit fields bit-reversed), 8 bytes per entry: the word, and the kind of a live entry in its top bits.
//   ft8_hint_kernel         one wave64 per candidate, four per workgroup, AP's launch geometry and block order.  The head,
//                           the soft bits, the ballot words H0 / H1 and the wave maximum are used as ap.hip uses them.
//                           Preselect: lanes are table entries, eight per lane (entry 64 r + lane in round r, so a round is
//                           one 512-byte load across the wave); the mask follows from the kind, positions 74..76 are the same
//                           for every entry (one scalar popcount), nbad is a popcount against H0, the gate test runs in the
//                           lane, and the lane keeps key << 10 | small-mask bit << 9 | index of each of its entries (under
//                           2^23).  Up to four rounds of a butterfly minimum pick the winners; the lane that owns a winner
//                           retires it.  The winners' words are read again by index (wave-uniform: a scalar load) and feed
//                           cand_dev.h's ap_try, the loop body of ap.hip.  (The A/B build also holds the form without the
//                           pre-kernel, which converts the 16-byte entries in the wave; it measured slower, see the kernels.)
//   ft8_hint_update_kernel  the update rule, one wave per receiver with its table in LDS (8 KB): a strictly sequential walk
//                           over the receiver's slots and records; an insert first looks for its (kind, a, b, phase) --
//                           eight entries per lane, ballots, the smallest index -- then refreshes that entry or overwrites
//                           the one under the cursor (as match.hip's update kernel does).
#include "hint.h"
#include "cand_dev.h"

namespace {

__device__ LdpcTables d_ldpc;

constexpr int kHintEntries = FT8GPU_HINT_ENTRIES;
constexpr int kHintRounds = kHintEntries / 64;
constexpr uint32_t kField29 = 0x1FFFFFFFu;
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;
constexpr uint64_t kI3Mask = 7ull << 10, kI3Bits = 1ull << 12;       // payload bits 74..76 = 001 over positions 64..127
static_assert(kHintEntries == 512, "the key holds a table index in its low nine bits");
static_assert(sizeof(ft8gpu_hint_entry) == 16 && sizeof(ft8gpu_hint_state) == 8208, "table layout");
static_assert(sizeof(ft8gpu_hint_info) == 16, "info record");
static_assert(kHintWorkBytes == (size_t)FT8GPU_HINT_ENTRIES * 8, "an encoded entry is 8 bytes");

// an entry as one uint4: a, b, stamp, kind | used << 8 | phase << 16 | pad << 24
__device__ __forceinline__ uint32_t entry_kind(uint4 e) { return e.w & 0xFFu; }
__device__ __forceinline__ bool entry_used(uint4 e) { return ((e.w >> 8) & 0xFFu) != 0u; }
__device__ __forceinline__ uint32_t entry_phase(uint4 e) { return (e.w >> 16) & 1u; }
// a 29-bit field, MSB first, onto codeword positions: payload bit i of the field at bit i
__device__ __forceinline__ uint64_t field_positions(uint32_t v) { return (uint64_t)(__brev(v & kField29) >> 3); }
// mask and bits of an entry over codeword positions 0..63 (kind 1, 2 or 3)
__device__ __forceinline__ void entry_words(uint4 e, uint64_t &m0, uint64_t &b0) {
    const uint32_t kind = entry_kind(e);
    m0 = ((kind & 1u) ? (uint64_t)kField29 : 0ull) | ((kind & 2u) ? (uint64_t)kField29 << 29 : 0ull);
    b0 = (field_positions(e.x) | field_positions(e.y) << 29) & m0;
}

// An encoded entry (what ft8_hint_encode_kernel leaves): the bit word over positions 0..57 in bits 0..57, the kind of a live entry
// in bits 62..63 (0: not live -- unused, a kind that is none, expired, or of the other phase).
__device__ __forceinline__ uint64_t kind_mask(uint32_t kind) {
    return ((kind & 1u) ? (uint64_t)kField29 : 0ull) | ((kind & 2u) ? (uint64_t)kField29 << 29 : 0ull);
}

// kEncoded: the entries come from `work` as ft8_hint_encode_kernel left them, not from the states
template <bool kEncoded>
__device__ __forceinline__
void hint_body(float (*s_mem)[kWaveLds], const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
               const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
               ft8gpu_decode_status *status_out, ft8gpu_hint_info *info, int nframes, int max_candidates,
               int max_iters, int force_ieee_div, const ft8gpu_hint_state *__restrict__ states, const uint2 *__restrict__ work,
               int tries, int max_bad_per_64, int max_hard_errors, uint32_t max_age, int use_phase,
               unsigned blocks_per_frame, unsigned bpf_magic) {
    // AP's block order and frame / candidate split (ap.hip)
    const unsigned nb = gridDim.x, per = nb >> 3, main_blocks = per << 3;
    const unsigned vb = blockIdx.x < main_blocks ? (blockIdx.x & 7u) * per + (blockIdx.x >> 3) : blockIdx.x;
    const CandWave w = cand_prologue<true>(vb, blocks_per_frame, bpf_magic, counts, status_in, status_out, info, nframes, max_candidates);
    if (w.verdict != kCandRun) return;
    const int lane = w.lane, frame = w.frame;
    const size_t rec_index = w.rec_index;
    const uint32_t *in32 = w.in32, mine = w.mine, dw0 = w.dw0;
    uint32_t *out32 = w.out32, *info32 = w.info32;

    float *toc = s_mem[w.wave];
    float *llr = toc + kTocFloats;

    float cw0[3];
    bool has[3];
    const bool all_finite = soft_bits(mag, frame, cands[rec_index], llr, lane, cw0, has);
    uint32_t amax = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) amax = max(amax, __float_as_uint(cw0[r]) & 0x7FFFFFFFu);
    const float apmag = __uint_as_float(wave_max(amax));              // non-negative floats order as their bit patterns
    if (!all_finite || apmag == 0.0f) {                               // wave-uniform: nothing is tried
        leave_record(out32, in32, info32, mine, 6u, lane, 4);
        return;
    }
    const uint64_t H0 = __ballot(cw0[0] > 0.0f), H1 = __ballot(cw0[1] > 0.0f), H2 = __ballot(cw0[2] > 0.0f);

    // ---- preselect: the lane's eight entries, their packed keys ---------------------------------------------------------
    const ft8gpu_hint_state *st = states + frame;
    const uint4 *entries = reinterpret_cast<const uint4 *>(st->entry);
    const uint32_t slot = kEncoded ? 0u : st->slot;
    const uint2 *wtab = work + (size_t)frame * kHintEntries;
    const uint32_t nbad1 = (uint32_t)__popcll((H1 ^ kI3Bits) & kI3Mask);
    uint32_t key[kHintRounds];
#pragma unroll
    for (int r = 0; r < kHintRounds; ++r) {
        uint32_t kind;
        bool live;
        uint64_t m0, b0;
        if (kEncoded) {
            const uint2 enc = wtab[64 * r + lane];
            kind = enc.y >> 30;
            live = kind != 0u;
            m0 = kind_mask(kind);
            b0 = (uint64_t)(enc.y & 0x03FFFFFFu) << 32 | enc.x;
        } else {
            const uint4 e = entries[64 * r + lane];
            kind = entry_kind(e);
            live = entry_used(e) && kind >= 1u && kind <= 3u;
            live = live && !(max_age != 0u && (uint32_t)(slot - e.z) > max_age);
            live = live && !(use_phase != 0 && ((slot ^ entry_phase(e)) & 1u) != 0u);
            entry_words(e, m0, b0);
        }
        const uint32_t nbad = (uint32_t)__popcll((H0 ^ b0) & m0) + nbad1;
        const bool both = kind == 3u;
        const uint32_t nmask = both ? 61u : 32u;
        const bool pass = live && nbad * 64u <= (uint32_t)max_bad_per_64 * nmask;
        const uint32_t k = nbad * (both ? 32u : 61u);
        key[r] = pass ? (k << 10 | (both ? 0u : 1u) << 9 | (uint32_t)(64 * r + lane)) : kKeyNone;
    }
    uint32_t win[FT8GPU_AP_MAX_HYPOTHESES];
    int ntry = 0;
#pragma unroll
    for (int k = 0; k < FT8GPU_AP_MAX_HYPOTHESES; ++k) {
        uint32_t best = kKeyNone;
#pragma unroll
        for (int r = 0; r < kHintRounds; ++r) best = min(best, key[r]);
        win[k] = wave_min(best);
        if (k < tries && win[k] != kKeyNone) ntry = k + 1;            // (once kKeyNone, always: nothing is retired into it)
#pragma unroll
        for (int r = 0; r < kHintRounds; ++r) key[r] = key[r] == win[k] ? kKeyNone : key[r];   // keys are unique: the owner retires it
    }
    if (ntry == 0) {                                                  // no passing entry
        leave_record(out32, in32, info32, mine, 0u, lane, 4);
        return;
    }

    const LdpcLane L = ldpc_lane(d_ldpc, lane);
    const uint64_t has2_mask = __ballot(has[2]);

    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);            // the record is composed where the raw soft bits were
    uint32_t results = 0, idx01 = 0, idx23 = 0;
    int result = 0, nhard = 0, iters_out = 0, ntried = 0;

    for (int k = 0; k < ntry; ++k) {                                  // wave-uniform
        const uint32_t wk = k == 0 ? win[0] : k == 1 ? win[1] : k == 2 ? win[2] : win[3];
        const uint32_t index = (uint32_t)__builtin_amdgcn_readfirstlane((int)(wk & 511u));
        uint64_t m0, b0;
        if (kEncoded) {
            const uint2 enc = wtab[index];
            m0 = kind_mask(enc.y >> 30);
            b0 = (uint64_t)(enc.y & 0x03FFFFFFu) << 32 | enc.x;
        } else {
            entry_words(entries[index], m0, b0);
        }
        ntried = k + 1;
        result = ap_try(cw0, has, has2_mask, toc, L, lane, max_iters, force_ieee_div, apmag, m0, kI3Mask, b0, kI3Bits, H0, H1, H2,
                        max_hard_errors, dw0, d_ldpc.crc_bit, rec32, nhard, iters_out);
        results |= (uint32_t)result << (8 * k);
        if (k < 2) idx01 |= index << (16 * k); else idx23 |= index << (16 * (k - 2));
        if (result == 1) break;
    }

    store_record(out32, in32, rec32, mine, result == 1, lane);
    if (lane == 0) {
        info32[0] = (uint32_t)result | ((uint32_t)nhard << 8) | ((uint32_t)ntried << 16) | ((uint32_t)iters_out << 24);
        info32[1] = results;
        info32[2] = idx01;
        info32[3] = idx23;
    }
}

// The product form of the table words: a pre-kernel converts every entry once per frame and call -- one lane per entry: the live
// test, the bit word -- and the candidate kernel loads 8 bytes per entry.  Measured beside the other form, which loads the 16
// bytes of an entry and converts in the wave (the A/B build keeps it, FT8GPU_AB_HINT_IN_WAVE), it is the faster one wherever the
// preselect weighs and equal where BP dominates; the figures are in profiles/hint_bench.json (tools/bench_hint.py times both
// forms) and DESIGN.md "Call hints".  Byte-identical.
__global__ __launch_bounds__(256)
void ft8_hint_encode_kernel(const ft8gpu_hint_state *__restrict__ states, uint32_t max_age, int use_phase, uint2 *__restrict__ work) {
    const int frame = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const ft8gpu_hint_state *st = states + frame;
    const uint4 e = reinterpret_cast<const uint4 *>(st->entry)[i];
    const uint32_t slot = st->slot, kind = entry_kind(e);
    bool live = entry_used(e) && kind >= 1u && kind <= 3u;
    live = live && !(max_age != 0u && (uint32_t)(slot - e.z) > max_age);
    live = live && !(use_phase != 0 && ((slot ^ entry_phase(e)) & 1u) != 0u);
    uint64_t m0, b0;
    entry_words(e, m0, b0);
    if (!live) b0 = 0ull;
    work[(size_t)frame * kHintEntries + i] = make_uint2((uint32_t)b0, (uint32_t)(b0 >> 32) | (live ? kind << 30 : 0u));
}

__global__ __launch_bounds__(256)
void ft8_hint_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                     const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                     ft8gpu_decode_status *status_out, ft8gpu_hint_info *info, int nframes, int max_candidates,
                     int max_iters, int force_ieee_div, const uint2 *__restrict__ work, int tries,
                     int max_bad_per_64, int max_hard_errors, unsigned blocks_per_frame, unsigned bpf_magic) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kWaveLds];
    hint_body<true>(s_mem, mag, cands, counts, status_in, status_out, info, nframes, max_candidates, max_iters, force_ieee_div, nullptr,
                    work, tries, max_bad_per_64, max_hard_errors, 0u, 0, blocks_per_frame, bpf_magic);
}

#ifdef FT8GPU_AB_FORMS
// the other form (FT8GPU_AB_HINT_IN_WAVE): no pre-kernel, the entries are read from the states and converted in the wave
__global__ __launch_bounds__(256)
void ft8_hint_in_wave_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                             const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                             ft8gpu_decode_status *status_out, ft8gpu_hint_info *info, int nframes, int max_candidates,
                             int max_iters, int force_ieee_div, const ft8gpu_hint_state *__restrict__ states, int tries,
                             int max_bad_per_64, int max_hard_errors, uint32_t max_age, int use_phase,
                             unsigned blocks_per_frame, unsigned bpf_magic) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kWaveLds];
    hint_body<false>(s_mem, mag, cands, counts, status_in, status_out, info, nframes, max_candidates, max_iters, force_ieee_div, states,
                     nullptr, tries, max_bad_per_64, max_hard_errors, max_age, use_phase, blocks_per_frame, bpf_magic);
}
#endif

// ---- the update rule ---------------------------------------------------------------------------------------------------

// insert(kind, a, b, phase) on the table in LDS; wave-uniform arguments, every lane takes part
__device__ __forceinline__ void hint_insert(uint4 *tab, uint32_t &cursor, uint32_t slot, uint32_t kind, uint32_t a, uint32_t b,
                                            uint32_t phase, int lane) {
    int found = -1;
#pragma unroll
    for (int r = 0; r < kHintRounds; ++r) {
        const uint4 e = tab[64 * r + lane];
        const uint64_t hit = __ballot(entry_used(e) && entry_kind(e) == kind && (e.x & kField29) == a && (e.y & kField29) == b &&
                                      entry_phase(e) == phase);
        if (found < 0 && hit != 0ull) found = 64 * r + __builtin_ctzll(hit);
    }
    if (found >= 0) {
        if (lane == 0) tab[found].z = slot;
    } else {
        const uint32_t at = cursor % (uint32_t)kHintEntries;
        if (lane == 0) tab[at] = make_uint4(a, b, slot, kind | 1u << 8 | phase << 16);
        cursor = at + 1u;
    }
    wave_lds_sync();
}

__global__ __launch_bounds__(64)
void ft8_hint_update_kernel(const ft8gpu_message *__restrict__ msgs, const int32_t *__restrict__ n_msgs, int ns,
                            ft8gpu_hint_state *state) {
    __shared__ uint4 tab[kHintEntries];
    const int lane = threadIdx.x;
    ft8gpu_hint_state *st = state + blockIdx.x;
    uint4 *entries = reinterpret_cast<uint4 *>(st->entry);
    for (int i = lane; i < kHintEntries; i += 64) tab[i] = entries[i];
    uint32_t cursor = st->cursor, slot = st->slot;
    wave_lds_sync();

    constexpr uint32_t kClear = (uint32_t)(ft8dev::NTOKENS + ft8dev::MAX22);
    for (int sl = 0; sl < ns; ++sl, ++slot) {
        const size_t f = (size_t)blockIdx.x * ns + sl;
        int n = n_msgs[f];
        n = n < 0 ? 0 : (n > kMaxMessages ? kMaxMessages : n);
        const uint32_t p = slot & 1u;
        for (int r = 0; r < n; ++r) {
            const uint4 a = reinterpret_cast<const uint4 *>(msgs + f * kMaxMessages + r)[3];      // a91[12], pad[4]: one address
            // the 77 payload bits, MSB first: bits 0..63, and bits 64..76 at the top
            const uint64_t w0 = (uint64_t)__builtin_bswap32(a.x) << 32 | __builtin_bswap32(a.y);
            const uint32_t w1 = __builtin_bswap32(a.z);
            if (((w1 >> 19) & 7u) != 1u) continue;                    // i3 = bits 74..76
            const uint32_t f1 = (uint32_t)(w0 >> 35), f2 = (uint32_t)(w0 >> 6) & kField29;
            if ((f2 >> 1) < kClear) continue;
            hint_insert(tab, cursor, slot, 2u, 0u, f2, p, lane);
            hint_insert(tab, cursor, slot, 1u, f2, 0u, p ^ 1u, lane);
            if ((f1 >> 1) < kClear) continue;
            hint_insert(tab, cursor, slot, 3u, f1, f2, p, lane);
            hint_insert(tab, cursor, slot, 3u, f2, f1, p ^ 1u, lane);
        }
    }
    for (int i = lane; i < kHintEntries; i += 64) entries[i] = tab[i];
    if (lane == 0) { st->cursor = cursor; st->slot = slot; }
}

}  // namespace

hipError_t hint_tables_init(hipStream_t s) {
    return upload_ldpc_tables(HIP_SYMBOL(d_ldpc), s);
}

hipError_t launch_hint(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                       const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_hint_info *info,
                       int nframes, int max_candidates, int ldpc_iters, int force_ieee_div, const ft8gpu_hint_state *states,
                       const ft8gpu_hint_params &q, void *work, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    if (q.tries < 1 || q.tries > FT8GPU_AP_MAX_HYPOTHESES || q.max_bad_per_64 < 0 || q.max_bad_per_64 > 64) return hipErrorInvalidValue;
    CandGrid g;
    if (cand_grid(nframes, max_candidates, g, true) != hipSuccess) return hipErrorInvalidValue;
    const unsigned magic = g.bpf == 1u ? 0u : (unsigned)((1ull << 32) / g.bpf) + 1u;
#ifdef FT8GPU_AB_FORMS
    if (!work) {                                                      // FT8GPU_AB_HINT_IN_WAVE
        hipLaunchKernelGGL(ft8_hint_in_wave_kernel, dim3(g.nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info,
                           nframes, max_candidates, ldpc_iters, force_ieee_div, states, q.tries, q.max_bad_per_64, q.max_hard_errors,
                           q.max_age, q.use_phase, g.bpf, magic);
        return hipGetLastError();
    }
#endif
    if (!work) return hipErrorInvalidValue;
    for (int f0 = 0; f0 < nframes; f0 += 65535) {                     // gridDim.y
        const int n = nframes - f0 < 65535 ? nframes - f0 : 65535;
        hipLaunchKernelGGL(ft8_hint_encode_kernel, dim3(kHintEntries / 256, (unsigned)n), dim3(256), 0, s, states + f0, q.max_age,
                           q.use_phase, (uint2 *)work + (size_t)f0 * kHintEntries);
    }
    hipLaunchKernelGGL(ft8_hint_kernel, dim3(g.nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info, nframes,
                       max_candidates, ldpc_iters, force_ieee_div, (const uint2 *)work, q.tries, q.max_bad_per_64, q.max_hard_errors,
                       g.bpf, magic);
    return hipGetLastError();
}

hipError_t launch_hint_update(const ft8gpu_message *msgs, const int32_t *n_msgs, int nrecv, int ns, ft8gpu_hint_state *state,
                              hipStream_t s) {
    if (nrecv < 1 || ns < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_hint_update_kernel, dim3((unsigned)nrecv), dim3(64), 0, s, msgs, n_msgs, ns, state);
    return hipGetLastError();
}

hipError_t launch_hint_tag(const int32_t *n_before, int stride, const int32_t *n_msgs, int nframes, ft8gpu_message *msgs,
                           hipStream_t s) {
    return launch_tag(nullptr, n_before, stride, n_msgs, nframes, msgs, TagConst<2>{ 3 }, s);    // pad[2] = 3: gained by a call hint
}
