// combine.hip -- the soft bits of undecoded candidates combined across a receiver's slots (include/ft8gpu.h "soft-bit
// memory", DESIGN.md "Soft-bit memory").  Not part of the reference's path, where every slot starts from nothing.  The rule
// is exact and restated in tests/ft8_spec_combine.py: a candidate BP failed on looks for the entries of its receiver's memory
// within one half step in time and frequency, takes the one whose hard decisions agree best with its own, adds the entry's
// running sum to its own soft bits, normalises the sum again and runs bp_decode on it; the update rule then stores the
// failing candidates' soft bits (own, or the sum where BP ran on one) into the ring.
//
//   ft8_combine_kernel         one wave64 per candidate, four per workgroup, the launch geometry of the LDPC kernel.  A wave
//                              whose candidate does not qualify copies the record and leaves.  Partner search: lanes are
//                              table entries (128 = two rounds of 64), the position test runs per lane; the partners are few,
//                              so the wave walks the ballot: 174 floats of the entry coalesced, three sign ballots against
//                              the candidate's own three hard-decision words, popcounts.  (174 - nagree) << 9 | dist << 7 |
//                              index, minimised over the walk (wave-uniform values: a scalar minimum), is the best partner
//                              with the rule's tie break.  The sum's normaliser accumulates in index order as the reference
//                              does -- every lane reads the 174 sums from LDS at one address and keeps the same two
//                              accumulators, so no reduction order has to be argued about.  The candidate's own soft bits,
//                              the BP iteration in its counting form, the CRC by linearity and the record composed in LDS are
//                              the shared device code of cand_dev.h.
//   ft8_softmem_update_kernel  one workgroup per receiver.  It reads the entry state from `old` and writes into `out`, which
//                              the host side has filled with a copy of `old`: every sum is formed from the state at entry
//                              whatever the ring overwrites.  Pass 1 marks the candidates that are stored (final status
//                              still failing, own finite) in a bit map in LDS, pass 2 gives each its ring slot, cursor plus
//                              the number of marked candidates in front of it (popcounts of the map), and writes the entry.
//
// The division guard.  cand_dev.h (guard_key) proves that iteration 0 needs no guard because every soft bit there is k * f / 2
// with an integer k and f >= 0.0192, and ap.hip relies on the same fact.  A renormalised sum has no such structure: x[i] is any
// finite float, 2^-90 or a subnormal next to values of ordinary size.  The soft bits enter the messages of EVERY iteration
// (x = (cwh + ah_a) + ah_b), and the argument of guard_key -- a sum of floats that are each 0 or >= 2^-59 is 0 or
// >= 2^-82, nothing is subnormal, halving commutes with every rounding -- needs cwh = -x / 2 in that set as well.  So the
// guard is evaluated ahead of iteration 0 on the candidate's own 174 soft bits, with the same key test as on the row
// products: every x[i] is 0 or |x[i]| >= 2^-58 (tested on x, not on the halved value, which may round a subnormal to zero).
// Where it holds, iteration 0 runs the fast form (x = cwh is in fast_tanh's domain) and every later iteration is guarded on
// its products (bp_decode_counting evaluates the guard after iteration 0 too); where it fails the whole candidate runs in
// the IEEE form, iteration 0 included.  That is sufficient: with all soft bits in the set, the premise of the proof for
// iteration k > 0 holds unchanged, and the IEEE form needs no premise.
#include "combine.h"
#include "cand_dev.h"

namespace {

__device__ LdpcTables d_ldpc;

constexpr int kIdxBits = 7, kDistBits = 2;    // the partner key: (174 - nagree) << 9 | dist << 7 | index
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;
static_assert(kSoftmemEntries == 1 << kIdxBits && kSoftmemEntries == 128, "the key holds a table index in its low bits");
static_assert(sizeof(ft8gpu_softmem_entry) == 720 && sizeof(ft8gpu_softmem_state) == 92176 && sizeof(ft8gpu_softmem_entry) % 16 == 0,
              "memory layout");

constexpr uint32_t kGuardMinSoft = ((127u - 58u) << 24) - 1u;   // guard_key(0x1p-58f): the soft bits, halved exactly to >= 2^-59

__global__ __launch_bounds__(256)
void ft8_combine_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                        const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                        ft8gpu_decode_status *status_out, ft8gpu_combine_info *info, int nframes, int max_candidates,
                        const ft8gpu_softmem_state *__restrict__ states, uint32_t max_age, int min_agree, int max_iters,
                        int force_ieee_div, unsigned blocks_per_frame) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kWaveLds];

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
    static_assert(sizeof(ft8gpu_decode_status) == 48 && sizeof(ft8gpu_combine_info) == 8, "record sizes");
    static_assert(offsetof(ft8gpu_combine_info, nagree) == 1 && offsetof(ft8gpu_combine_info, index) == 2 &&
                  offsetof(ft8gpu_combine_info, count) == 3 && offsetof(ft8gpu_combine_info, nhard) == 4, "info layout");

    uint32_t mine, dw0;
    if (!read_record(in32, lane, mine, dw0)) {                        // does not qualify
        leave_record(out32, in32, info32, mine, 0u, lane);
        return;
    }

    float *toc = s_mem[wave];
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
    float sum = 0.0f, sum2 = 0.0f;                                    // every lane: the same 174 values in index order
    for (int i = 0; i < 172; i += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(llr + i);
        sum = sum + v.x; sum2 = sum2 + v.x * v.x;
        sum = sum + v.y; sum2 = sum2 + v.y * v.y;
        sum = sum + v.z; sum2 = sum2 + v.z * v.z;
        sum = sum + v.w; sum2 = sum2 + v.w * v.w;
    }
    {
        const float2 v = *reinterpret_cast<const float2 *>(llr + 172);
        sum = sum + v.x; sum2 = sum2 + v.x * v.x;
        sum = sum + v.y; sum2 = sum2 + v.y * v.y;
    }
    float cw[3];
    {
        const float inv_n = 1.0f / 174;
        const float variance = (sum2 - (sum * sum * inv_n)) * inv_n;
        const float norm_factor = bpm::llr_norm_factor(variance);
        bool finite = true;
        uint32_t gk = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            cw[r] = has[r] ? llr[lane + 64 * r] * norm_factor : 0.0f;
            finite = finite && (__float_as_uint(cw[r]) & 0x7F800000u) != 0x7F800000u;
            gk = min(gk, guard_key(cw[r]));
        }
        if (!__all(finite)) {                                         // wave-uniform: result 6, BP does not run
            leave_record(out32, in32, info32, mine, 6u | info_lo, lane);
            return;
        }
        // the guard ahead of iteration 0 (head of the file): a soft bit outside the set sends every iteration to the IEEE form
        if (!__all(gk >= kGuardMinSoft)) force_ieee_div = 1;
    }
    const uint64_t X0 = __ballot(cw[0] > 0.0f), X1 = __ballot(cw[1] > 0.0f), X2 = __ballot(cw[2] > 0.0f);

    const BpWord bp = bp_decode_counting(cw, has, has2_mask, toc, ldpc_lane(d_ldpc, lane), lane, max_iters, force_ieee_div);
    const uint64_t B0 = bp.B0, B1 = bp.B1, B2 = bp.B2;

    // ---- judge the word BP left: the first failing check names the result ---------------------------------------------
    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);            // the record is composed where the sums were
    int result, nhard = 0;
    if (bp.min_errors != 0) result = 7;
    else {
        nhard = __popcll(B0 ^ X0) + __popcll(B1 ^ X1) + __popcll(B2 ^ X2);
        if ((B0 | B1 | B2) == 0ull) result = 5;                       // (bp_decode leaves at an all-zero word before it checks it)
        else {
            wave_lds_sync();                                          // the sums have been read
            result = compose_success_record(B0, B1, dw0, d_ldpc.crc_bit, rec32, lane);
        }
    }
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

__global__ __launch_bounds__(256)
void ft8_combine_tag_kernel(const int32_t *__restrict__ n_before, int stride, const int32_t *__restrict__ n_msgs, int nframes,
                            ft8gpu_message *__restrict__ msgs) {
    const int frame = blockIdx.x * 4 + (threadIdx.x >> 6), r = threadIdx.x & 63;
    if (frame >= nframes) return;
    int lo = n_before[(size_t)frame * stride], hi = n_msgs[frame];
    lo = lo < 0 ? 0 : lo;
    hi = hi > kMaxMessages ? kMaxMessages : hi;
    if (r < lo || r >= hi) return;
    msgs[(size_t)frame * kMaxMessages + r].pad[2] = 2;
}

}  // namespace

hipError_t combine_tables_init(hipStream_t s) {
    static LdpcTables h;
    fill_ldpc_tables(h);
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(d_ldpc), &h, sizeof(h), 0, hipMemcpyHostToDevice, s);
}

hipError_t launch_combine(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                          const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_combine_info *info,
                          int nframes, int max_candidates, const ft8gpu_softmem_state *states, uint32_t max_age, int min_agree,
                          int ldpc_iters, int force_ieee_div, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    const unsigned bpf = (unsigned)(max_candidates + 3) / 4;                  // blocks (of 4 candidate waves) per frame
    const unsigned long long nblocks = (unsigned long long)nframes * bpf;
    if (nblocks >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ft8_combine_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info,
                       nframes, max_candidates, states, max_age, min_agree, ldpc_iters, force_ieee_div, bpf);
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
    if (nframes < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_combine_tag_kernel, dim3((nframes + 3) / 4), dim3(256), 0, s, n_before, stride, n_msgs, nframes, msgs);
    return hipGetLastError();
}
