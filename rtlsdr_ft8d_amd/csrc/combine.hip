// combine.hip -- the soft bits of undecoded candidates combined across a receiver's slots (include/ft8gpu.h "soft-bit
// memory", DESIGN.md "Soft-bit memory").  Not part of the reference's path, where every slot starts from nothing.  The rule
// is exact and restated in tests/ft8_spec_combine.py: a candidate BP failed on looks for the entries of its receiver's memory
// within one half step in time and frequency, takes the one whose hard decisions agree best with its own, adds the entry's
// running sum to its own soft bits, normalises the sum again and runs bp_decode on it; the update rule then stores the
// failing candidates' soft bits (own, or the sum where BP ran on one) into the ring.
//
//   ft8_combine_kernel         one wave64 per candidate, four per workgroup, the launch geometry of the LDPC kernel.  Partner
//                              search: lanes are table entries (128 = two rounds of 64), the position test runs per lane; the
//                              partners are few, so the wave walks the ballot: 174 floats of the entry coalesced, three sign
//                              ballots against the candidate's own three hard-decision words, popcounts.  (174 - nagree) << 9
//                              | dist << 7 | index, minimised over the walk (wave-uniform values: a scalar minimum), is the
//                              best partner with the rule's tie break.  The head of the kernel, the candidate's own soft bits,
//                              the sum's normalisation in index order, the BP iteration in its counting form, the judgement
//                              with the CRC by linearity and the record composed in LDS, and the tag of the message records
//                              are the shared device code of cand_dev.h.
//   ft8_softmem_update_kernel  one workgroup per receiver.  It reads the entry state from `old` and writes into `out`, which
//                              the host side has filled with a copy of `old`: every sum is formed from the state at entry
//                              whatever the ring overwrites.  Pass 1 marks the candidates that are stored (final status
//                              still failing, own finite) in a bit map in LDS, pass 2 gives each its ring slot, cursor plus
//                              the number of marked candidates in front of it (popcounts of the map), and writes the entry.
// The division guard of a renormalised sum: cand_dev.h, renormalise_in_order.
#include "combine.h"
#include "cand_dev.h"

namespace {

__device__ LdpcTables d_ldpc;

constexpr int kIdxBits = 7, kDistBits = 2;    // the partner key: (174 - nagree) << 9 | dist << 7 | index
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;
static_assert(kSoftmemEntries == 1 << kIdxBits && kSoftmemEntries == 128, "the key holds a table index in its low bits");
static_assert(sizeof(ft8gpu_softmem_entry) == 720 && sizeof(ft8gpu_softmem_state) == 92176 && sizeof(ft8gpu_softmem_entry) % 16 == 0,
              "memory layout");

__global__ __launch_bounds__(256)
void ft8_combine_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                        const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                        ft8gpu_decode_status *status_out, ft8gpu_combine_info *info, int nframes, int max_candidates,
                        const ft8gpu_softmem_state *__restrict__ states, uint32_t max_age, int min_agree, int max_iters,
                        int force_ieee_div, unsigned blocks_per_frame) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kWaveLds];

    static_assert(sizeof(ft8gpu_combine_info) == 8, "record sizes");
    static_assert(offsetof(ft8gpu_combine_info, nagree) == 1 && offsetof(ft8gpu_combine_info, index) == 2 &&
                  offsetof(ft8gpu_combine_info, count) == 3 && offsetof(ft8gpu_combine_info, nhard) == 4, "info layout");
    const CandWave w = cand_prologue(blockIdx.x, blocks_per_frame, 0u, counts, status_in, status_out, info, nframes, max_candidates);
    if (w.verdict != kCandRun) return;
    const int lane = w.lane, frame = w.frame;
    const size_t rec_index = w.rec_index;
    const uint32_t *in32 = w.in32, mine = w.mine, dw0 = w.dw0;
    uint32_t *out32 = w.out32, *info32 = w.info32;

    float *toc = s_mem[w.wave];
    float *llr = toc + kTocFloats;

    const ft8gpu_candidate cand = cands[rec_index];
    float own[3];
    bool has[3];
    if (!soft_bits(mag, frame, cand, llr, lane, own, has)) {          // wave-uniform: nothing is tried
        leave_record(out32, in32, info32, mine, 6u, lane);
        return;
    }
    const uint64_t has2_mask = __ballot(has[2]);         // lanes that own a third variable (n = lane + 128 < 174)
    const uint64_t O0 = __ballot(own[0] > 0.0f), O1 = __ballot(own[1] > 0.0f), O2 = __ballot(own[2] > 0.0f);

    // ---- partner search: lanes are entries, two rounds of 64; the position test per lane ------------------------------------
    const ft8gpu_softmem_state *st = states + frame;
    const uint32_t slot_now = st->slot;
    const int T = 2 * cand.time_offset + cand.time_sub, F = 2 * cand.freq_offset + cand.freq_sub;
    uint32_t best = kKeyNone;
#pragma unroll
    for (int r = 0; r < kSoftmemEntries / 64; ++r) {
        const uint4 e = *reinterpret_cast<const uint4 *>(st->entry + 64 * r + lane);      // cand, used / count / pad, stamp
        const int te = 2 * (int)(int16_t)(e.x >> 16) + (int)((e.y >> 16) & 0xFFu);
        const int fe = 2 * (int)(int16_t)(e.y & 0xFFFFu) + (int)(e.y >> 24);
        const int dt = abs(T - te), df = abs(F - fe);
        const bool live = (e.z & 0xFFu) != 0u && !(max_age != 0u && (uint32_t)(slot_now - e.w) > max_age);
        const int dist = dt + df;
        uint64_t partners = __ballot(live && dt <= 1 && df <= 1);
        while (partners != 0ull) {                                    // wave-uniform; the partners are few
            const int j = __builtin_ctzll(partners);
            partners &= partners - 1ull;
            const float *L = st->entry[64 * r + j].llr;
            const float v0 = L[lane], v1 = L[lane + 64], v2 = has[2] ? L[lane + 128] : 0.0f;
            const uint64_t E0 = __ballot(v0 > 0.0f), E1 = __ballot(v1 > 0.0f), E2 = __ballot(v2 > 0.0f);
            const int nagree = __popcll(~(E0 ^ O0)) + __popcll(~(E1 ^ O1)) + __popcll(~(E2 ^ O2) & has2_mask);
            const uint32_t d = (uint32_t)__builtin_amdgcn_readlane(dist, j);
            const uint32_t key = ((uint32_t)(kLdpcN - nagree) << (kIdxBits + kDistBits)) | (d << kIdxBits) | (uint32_t)(64 * r + j);
            best = min(best, key);
        }
    }
    if (best == kKeyNone) {                                           // no partner: result 0
        leave_record(out32, in32, info32, mine, 0u, lane);
        return;
    }
    const int index = (int)(best & (uint32_t)(kSoftmemEntries - 1));
    const int nagree = kLdpcN - (int)(best >> (kIdxBits + kDistBits));
    const ft8gpu_softmem_entry *ent = st->entry + index;
    const uint32_t ecount = (reinterpret_cast<const uint32_t *>(ent)[2] >> 8) & 0xFFu;
    const uint32_t info_lo = ((uint32_t)nagree << 8) | ((uint32_t)index << 16) | (ecount << 24);
    if (nagree < min_agree) {                                         // result 8: BP does not run
        leave_record(out32, in32, info32, mine, 8u | info_lo, lane);
        return;
    }

    // ---- s = entry.llr + own, x = ftx_normalize_logl(s) with the reference's accumulation order ---------------------------
    wave_lds_sync();                                                  // the raw soft bits have been read
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (has[r]) llr[lane + 64 * r] = ent->llr[lane + 64 * r] + own[r];
    wave_lds_sync();
    float cw[3];
    if (!renormalise_in_order(llr, has, lane, cw, force_ieee_div)) {  // wave-uniform: result 6, BP does not run
        leave_record(out32, in32, info32, mine, 6u | info_lo, lane);
        return;
    }
    const uint64_t X0 = __ballot(cw[0] > 0.0f), X1 = __ballot(cw[1] > 0.0f), X2 = __ballot(cw[2] > 0.0f);

    const BpWord bp = bp_decode_counting(cw, has, has2_mask, toc, ldpc_lane(d_ldpc, lane), lane, max_iters, force_ieee_div);

    // ---- judge the word BP left; no gate on the hard errors (kLdpcN cannot trip) -------------------------------------------
    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);            // the record is composed where the sums were
    int nhard;
    const int result = judge_bp_word(bp, X0, X1, X2, kLdpcN, dw0, d_ldpc.crc_bit, rec32, lane, nhard);
    store_record(out32, in32, rec32, mine, result == 1, lane);
    if (lane == 0) {
        info32[0] = (uint32_t)result | info_lo;
        info32[1] = (uint32_t)nhard;
    }
}

// ---- the update rule ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256)
void ft8_softmem_update_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                               const int32_t *__restrict__ counts, const ft8gpu_decode_status *__restrict__ status,
                               const ft8gpu_combine_info *__restrict__ info, int max_candidates,
                               const ft8gpu_softmem_state *__restrict__ old, ft8gpu_softmem_state *__restrict__ out,
                               int store_per_slot) {
    __shared__ unsigned long long s_flags[FT8GPU_ABS_MAX_CANDIDATES / 64];
    __shared__ __attribute__((aligned(16))) float s_llr[4][192];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int frame = blockIdx.x;
    int count = counts[frame];
    count = count < 0 ? 0 : (count > max_candidates ? max_candidates : count);
    if (threadIdx.x < FT8GPU_ABS_MAX_CANDIDATES / 64) s_flags[threadIdx.x] = 0ull;
    __syncthreads();

    float *llr = s_llr[wave];
    const ft8gpu_softmem_state *so = old + frame;
    ft8gpu_softmem_state *sn = out + frame;
    float own[3];
    bool has[3];

    // ---- pass 1: which candidates are stored -- the final record still failing, own finite --------------------------------
    if (store_per_slot > 0)
        for (int ci = wave; ci < count; ci += 4) {                    // wave-uniform
            const size_t rec_index = (size_t)frame * max_candidates + ci;
            const uint32_t *st32 = reinterpret_cast<const uint32_t *>(status + rec_index);
            if (!still_failing(st32[0], st32[2])) continue;
            wave_lds_sync();                                          // the previous candidate's reads of llr are done
            if (soft_bits(mag, frame, cands[rec_index], llr, lane, own, has) && lane == 0)
                atomicOr(&s_flags[ci >> 6], 1ull << (ci & 63));
        }
    __syncthreads();

    // ---- pass 2: ring slot = cursor + the number of stored candidates in front; sums from the state at entry -----------------
    const uint32_t cursor0 = so->cursor % (uint32_t)kSoftmemEntries, slot_now = so->slot;
    int total = 0;
    for (int w = 0; w < FT8GPU_ABS_MAX_CANDIDATES / 64; ++w) total += __popcll(s_flags[w]);
    for (int ci = wave; ci < count; ci += 4) {                        // wave-uniform
        const unsigned long long fw = s_flags[ci >> 6];
        if (((fw >> (ci & 63)) & 1ull) == 0ull) continue;
        int rank = __popcll(fw & ((1ull << (ci & 63)) - 1ull));
        for (int w = 0; w < (ci >> 6); ++w) rank += __popcll(s_flags[w]);
        if (rank >= store_per_slot) continue;
        const size_t rec_index = (size_t)frame * max_candidates + ci;
        const ft8gpu_candidate cand = cands[rec_index];
        wave_lds_sync();
        (void)soft_bits(mag, frame, cand, llr, lane, own, has);
        const uint32_t inf = reinterpret_cast<const uint32_t *>(info + rec_index)[0];
        const uint32_t res = inf & 0xFFu;
        const bool ran = res == 3u || res == 4u || res == 5u || res == 7u;    // BP ran on the sum: store the sum
        const ft8gpu_softmem_entry *pe = so->entry + ((inf >> 16) & (uint32_t)(kSoftmemEntries - 1));
        uint32_t cnt = ran ? ((inf >> 24) & 0xFFu) + 1u : 1u;
        cnt = cnt > 255u ? 255u : cnt;
        ft8gpu_softmem_entry *ne = sn->entry + ((cursor0 + (uint32_t)rank) % (uint32_t)kSoftmemEntries);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int n = lane + 64 * r;
            if (n < 176) ne->llr[n] = has[r] ? (ran ? pe->llr[n] + own[r] : own[r]) : 0.0f;
        }
        if (lane == 0) {
            const uint2 c2 = *reinterpret_cast<const uint2 *>(cands + rec_index);
            *reinterpret_cast<uint4 *>(ne) = make_uint4(c2.x, c2.y, 1u | (cnt << 8), slot_now);
        }
    }
    if (threadIdx.x == 0) {
        const int n = total < store_per_slot ? total : store_per_slot;
        if (n > 0) sn->cursor = (cursor0 + (uint32_t)n - 1u) % (uint32_t)kSoftmemEntries + 1u;
        sn->slot = slot_now + 1u;
    }
}

}  // namespace

hipError_t combine_tables_init(hipStream_t s) {
    return upload_ldpc_tables(HIP_SYMBOL(d_ldpc), s);
}

hipError_t launch_combine(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                          const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_combine_info *info,
                          int nframes, int max_candidates, const ft8gpu_softmem_state *states, uint32_t max_age, int min_agree,
                          int ldpc_iters, int force_ieee_div, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    CandGrid g;
    if (cand_grid(nframes, max_candidates, g) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ft8_combine_kernel, dim3(g.nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info,
                       nframes, max_candidates, states, max_age, min_agree, ldpc_iters, force_ieee_div, g.bpf);
    return hipGetLastError();
}

hipError_t launch_softmem_update(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                                 const ft8gpu_decode_status *status, const ft8gpu_combine_info *info, int nframes,
                                 int max_candidates, const ft8gpu_softmem_state *old, ft8gpu_softmem_state *out,
                                 int store_per_slot, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    if (max_candidates > FT8GPU_ABS_MAX_CANDIDATES || old == out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ft8_softmem_update_kernel, dim3((unsigned)nframes), dim3(256), 0, s, mag, cands, counts, status, info,
                       max_candidates, old, out, store_per_slot);
    return hipGetLastError();
}

hipError_t launch_combine_tag(const int32_t *n_before, int stride, const int32_t *n_msgs, int nframes, ft8gpu_message *msgs,
                              hipStream_t s) {
    return launch_tag(nullptr, n_before, stride, n_msgs, nframes, msgs, TagConst<2>{ 2 }, s);    // pad[2] = 2: combined
}
