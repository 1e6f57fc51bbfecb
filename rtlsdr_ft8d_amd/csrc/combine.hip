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
//                              accumulators, so no reduction order has to be argued about.  The BP iteration, the CRC by
//                              linearity, unpack77 on two 64-bit words and the record composed in LDS are copies of ap.hip's
//                              counting form, so that ap.hip and decode.hip stay byte for byte what they are.
//   ft8_softmem_update_kernel  one workgroup per receiver.  It reads the entry state from `old` and writes into `out`, which
//                              the host side has filled with a copy of `old`: every sum is formed from the state at entry
//                              whatever the ring overwrites.  Pass 1 marks the candidates that are stored (final status
//                              still failing, own finite) in a bit map in LDS, pass 2 gives each its ring slot, cursor plus
//                              the number of marked candidates in front of it (popcounts of the map), and writes the entry.
//
// The division guard.  decode.hip proves that iteration 0 needs no guard because every soft bit there is k * f / 2 with an
// integer k and f >= 0.0192, and ap.hip relies on the same fact.  A renormalised sum has no such structure: x[i] is any
// finite float, 2^-90 or a subnormal next to values of ordinary size.  The soft bits enter the messages of EVERY iteration
// (x = (cwh + ah_a) + ah_b), and the argument of decode.hip's guard_key -- a sum of floats that are each 0 or >= 2^-59 is 0 or
// >= 2^-82, nothing is subnormal, halving commutes with every rounding -- needs cwh = -x / 2 in that set as well.  So the
// guard is evaluated ahead of iteration 0 on the candidate's own 174 soft bits, with the same key test as on the row
// products: every x[i] is 0 or |x[i]| >= 2^-58 (tested on x, not on the halved value, which may round a subnormal to zero).
// Where it holds, iteration 0 runs the fast form (x = cwh is in fast_tanh's domain) and every later iteration is guarded on
// its products as in decode.hip (ap.hip's form, which evaluates the guard after iteration 0 too); where it fails the whole
// candidate runs in the IEEE form, iteration 0 included.  That is sufficient: with all soft bits in the set, the premise of
// decode.hip's proof for iteration k > 0 holds unchanged, and the IEEE form needs no premise.
#include "combine.h"
#include "ft8_tables.h"
#include "unpack_dev.h"
#include "bp_math.h"
#include "ldpc_lds_layout.h"
#include <stddef.h>
#include <stdlib.h>
#include <type_traits>

namespace {

using bpm::f2;
using bpm::tanh_pair;
using bpm::tanh_one;
using bpm::atanh_pair;
using bpm::atanh_one;

struct CombineTables {
    uint16_t edge_slot[3][64][3];     // [r][lane][m_idx] -> float index of slot (m, pos) in the LDS tile
    uint64_t rowmask[2][64][3];       // [rr][lane][word] bit mask of the variables of check m = lane + 64 rr
    uint8_t  row_valid[2][64];
    uint8_t  own6[64], own7[64];      // product ownership (decode.hip)
    uint16_t crc_bit[77];             // CRC-14 (over 82 bits) of the message whose only set bit is payload bit i
};

__device__ CombineTables d_cmb;
__constant__ uint8_t c_cmb_gray[8] = { 0, 1, 3, 2, 5, 6, 4, 7 };

constexpr int kRows = 84;                     // 83 check rows + 1 spare row for idle lanes
constexpr int kTocFloats = kRows * 8;         // plane LO: [84] float4 (slots 0..3), plane HI: [84] float4 (slots 4..7)
constexpr int kWaveLds = kTocFloats + 192;    // + 174 soft bits
constexpr int kIdxBits = 7, kDistBits = 2;    // the partner key: (174 - nagree) << 9 | dist << 7 | index
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;
static_assert(kSoftmemEntries == 1 << kIdxBits && kSoftmemEntries == 128, "the key holds a table index in its low bits");
static_assert(sizeof(ft8gpu_softmem_entry) == 720 && sizeof(ft8gpu_softmem_state) == 92176 && sizeof(ft8gpu_softmem_entry) % 16 == 0,
              "memory layout");

__host__ __device__ constexpr int slot_index(int m, int pos) {
    return pos < 4 ? 4 * m + pos : 4 * kRows + 4 * m + (pos - 4);
}

__device__ __forceinline__ float min3_abs(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float add_f32(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// the division guard of decode.hip (guard_key there has the argument)
__device__ __forceinline__ uint32_t guard_key(float v) { return (__float_as_uint(v) << 1) - 1u; }
constexpr uint32_t kGuardMin = ((127u - 59u) << 24) - 1u;       // guard_key(0x1p-59f): the row products
constexpr uint32_t kGuardMinSoft = ((127u - 58u) << 24) - 1u;   // guard_key(0x1p-58f): the soft bits, halved exactly to >= 2^-59

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);   // row_mirror: every lane holds its row's sum
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);   // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t x) {
    int v = (int)x;
    v ^= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
    v ^= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
    v ^= __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
    v ^= __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
    v ^= __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);
    v ^= __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);
    return (uint32_t)__builtin_amdgcn_readlane(v, 63);
}

// own[0..173] of a candidate: ft8_extract_likelihood and ftx_normalize_logl, the LDPC kernel's arithmetic (decode.hip, as
// ap.hip and match.hip copy it).  llr: 192 floats of the wave's LDS (the raw soft bits stay there); lane l gets own[l],
// own[l + 64], own[l + 128] (0 past 173).  Returns whether every value is finite (wave-uniform).  Every lane takes part.
__device__ __forceinline__ bool own_soft_bits(const uint8_t *__restrict__ mag, int frame, const ft8gpu_candidate cand, float *llr,
                                              int lane, float (&cw)[3], bool (&has)[3]) {
    if (lane < 58) {
        const int k = lane;
        const int sym = k + ((k < 29) ? 7 : 14);
        const int block = cand.time_offset + sym;
        int l0 = 0, l1 = 0, l2 = 0;
        if (block >= 0 && block < kNumBlocks) {
            const int index = ((cand.time_offset * 2 + cand.time_sub) * 2 + cand.freq_sub) * kNumBin + cand.freq_offset;
            const uint8_t *ps = mag + (size_t)frame * kMagArray + index + sym * kBlockStride;
            int s2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) s2[j] = ps[c_cmb_gray[j]];
            l0 = max(max(s2[4], s2[5]), max(s2[6], s2[7])) - max(max(s2[0], s2[1]), max(s2[2], s2[3]));
            l1 = max(max(s2[2], s2[3]), max(s2[6], s2[7])) - max(max(s2[0], s2[1]), max(s2[4], s2[5]));
            l2 = max(max(s2[1], s2[3]), max(s2[5], s2[7])) - max(max(s2[0], s2[2]), max(s2[4], s2[6]));
        }
        llr[3 * k + 0] = (float)l0;
        llr[3 * k + 1] = (float)l1;
        llr[3 * k + 2] = (float)l2;
    }
    wave_lds_sync();
    int isum = 0, isum2 = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int n = lane + 64 * r;
        has[r] = n < kLdpcN;
        cw[r] = has[r] ? llr[n] : 0.0f;
        const int v = (int)cw[r];
        isum += v;
        isum2 += v * v;
    }
    const float sum = (float)wave_sum(isum);
    const float sum2 = (float)wave_sum(isum2);
    const float inv_n = 1.0f / 174;
    const float variance = (sum2 - (sum * sum * inv_n)) * inv_n;
    const float norm_factor = bpm::llr_norm_factor(variance);       // sqrtf(24.0f / variance), both correctly rounded (bp_math.h)
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        cw[r] = has[r] ? cw[r] * norm_factor : 0.0f;
        finite = finite && (__float_as_uint(cw[r]) & 0x7F800000u) != 0x7F800000u;
    }
    return __all(finite);
}

// ok == 0 and ldpc_errors != 0 from the record's dwords 0 and 2
__device__ __forceinline__ bool still_failing(uint32_t dw0, uint32_t dw2) { return ((dw2 >> 8) & 0xFFu) == 0u && (dw0 & 0xFFFFu) != 0u; }

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

    // ---- which candidates: ok == 0 and ldpc_errors != 0 (status_out may be status_in: read first) -------------------
    const uint32_t mine = lane < 12 ? in32[lane] : 0u;
    const uint32_t dw0 = (uint32_t)__builtin_amdgcn_readlane((int)mine, 0);
    const uint32_t dw2 = (uint32_t)__builtin_amdgcn_readlane((int)mine, 2);
    if (!still_failing(dw0, dw2)) {
        if (lane < 12 && out32 != in32) out32[lane] = mine;
        if (lane < 2) info32[lane] = 0u;
        return;
    }

    float *toc = s_mem[wave];
    float *llr = toc + kTocFloats;
    float4 *planeLO = reinterpret_cast<float4 *>(toc);
    float4 *planeHI = planeLO + kRows;

    const ft8gpu_candidate cand = cands[rec_index];
    float own[3];
    bool has[3];
    if (!own_soft_bits(mag, frame, cand, llr, lane, own, has)) {      // wave-uniform: nothing is tried
        if (lane < 12 && out32 != in32) out32[lane] = mine;
        if (lane < 2) info32[lane] = lane == 0 ? 6u : 0u;
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
        if (lane < 12 && out32 != in32) out32[lane] = mine;
        if (lane < 2) info32[lane] = 0u;
        return;
    }
    const int index = (int)(best & (uint32_t)(kSoftmemEntries - 1));
    const int nagree = kLdpcN - (int)(best >> (kIdxBits + kDistBits));
    const ft8gpu_softmem_entry *ent = st->entry + index;
    const uint32_t ecount = (reinterpret_cast<const uint32_t *>(ent)[2] >> 8) & 0xFFu;
    const uint32_t info_lo = ((uint32_t)nagree << 8) | ((uint32_t)index << 16) | (ecount << 24);
    if (nagree < min_agree) {                                         // result 8: BP does not run
        if (lane < 12 && out32 != in32) out32[lane] = mine;
        if (lane < 2) info32[lane] = lane == 0 ? (8u | info_lo) : 0u;
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
            if (lane < 12 && out32 != in32) out32[lane] = mine;
            if (lane < 2) info32[lane] = lane == 0 ? (6u | info_lo) : 0u;
            return;
        }
        // the guard ahead of iteration 0 (head of the file): a soft bit outside the set sends every iteration to the IEEE form
        if (!__all(gk >= kGuardMinSoft)) force_ieee_div = 1;
    }
    const uint64_t X0 = __ballot(cw[0] > 0.0f), X1 = __ballot(cw[1] > 0.0f), X2 = __ballot(cw[2] > 0.0f);

    // ---- per-lane constant edge / row data ---------------------------------------------------
    int slot[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int e = 0; e < 3; ++e) slot[3 * r + e] = d_cmb.edge_slot[r][lane][e];
    uint64_t rmask[2][3];
    bool rvalid[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        rvalid[rr] = d_cmb.row_valid[rr][lane] != 0;
#pragma unroll
        for (int w = 0; w < 3; ++w) rmask[rr][w] = d_cmb.rowmask[rr][lane][w];
    }
    const int row6 = d_cmb.own6[lane], row7 = d_cmb.own7[lane];
    const bool has6 = row6 != kRows - 1, has7 = row7 != kRows - 1;

    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);            // the record is composed where the sums were
    char *rec = reinterpret_cast<char *>(llr);

    // the spare row only needs finite content (idle lanes of the variable side read and write it)
    wave_lds_sync();
    if (lane < 8) toc[slot_index(kRows - 1, lane)] = 1.0f;
    wave_lds_sync();

    // ---- bp_decode: the iteration of decode.hip, counting form, as ap.hip copies it (the comments there explain the layout) --
    float cwh[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cwh[r] = cw[r] * -0.5f;
    const f2 cwh01 = { cwh[0], cwh[1] };
    int min_errors = kLdpcM;
    uint64_t B0 = 0, B1 = 0, B2 = 0;
    int iter = 0;
    bool fast_ok = !force_ieee_div;
    f2 PA[3] = { { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.0f, 0.0f } }, PB = { 0.0f, 0.0f };
    float pc = 0.0f;

    auto first_half = [&](auto fast_tag) -> bool {
        constexpr bool FAST = decltype(fast_tag)::value;
        f2 A[3], B;
        float c2;
        if (iter > 0) {                                  // wave-uniform
#pragma unroll
            for (int r = 0; r < 2; ++r) A[r] = atanh_pair<FAST>(PA[r]);
            B = atanh_pair<FAST>(PB);
            A[2] = f2{ 0.0f, 0.0f };
            c2 = 0.0f;
            if (has[2]) {
                A[2] = atanh_pair<FAST>(PA[2]);
                c2 = atanh_one<FAST>(pc);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) A[r] = f2{ 0.0f, 0.0f };
            B = f2{ 0.0f, 0.0f };
            c2 = 0.0f;
        }
        f2 X[3], Y;
        float z;
        if (FAST) {
            const f2 u01 = cwh01 + B;
            const float u2 = cwh[2] + c2;
            X[0] = f2{ u01.x, u01.x } + A[0];
            X[1] = f2{ u01.y, u01.y } + A[1];
            X[2] = f2{ u2, u2 } + A[2];
            Y.x = add_f32(add_f32(cwh[0], A[0].y), A[0].x);
            Y.y = add_f32(add_f32(cwh[1], A[1].y), A[1].x);
            z = add_f32(add_f32(cwh[2], A[2].y), A[2].x);
            B0 = __ballot((X[0].y + A[0].x) < 0.0f);
            B1 = __ballot((X[1].y + A[1].x) < 0.0f);
            B2 = __ballot((X[2].y + A[2].x) < 0.0f) & has2_mask;
        } else {
            const float ah0[3] = { B.x, B.y, c2 };
            float x0[3];
            bool bit[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float v0 = -2 * ah0[r], v1 = -2 * A[r].y, v2 = -2 * A[r].x;   // tov
                const float u = cw[r] + v0;
                bit[r] = has[r] && (((u + v1) + v2) > 0.0f);
                x0[r] = ((cw[r] + v1) + v2) * -0.5f;
                X[r].x = (u + v2) * -0.5f;
                X[r].y = (u + v1) * -0.5f;
            }
            Y.x = x0[0];
            Y.y = x0[1];
            z = x0[2];
            B0 = __ballot(bit[0]);
            B1 = __ballot(bit[1]);
            B2 = __ballot(bit[2]);
        }
        if ((B0 | B1 | B2) == 0ull) return true;        // all-zero word is prohibited

        // ldpc_check
        int errors = 0;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int par = (__popcll(B0 & rmask[rr][0]) + __popcll(B1 & rmask[rr][1]) + __popcll(B2 & rmask[rr][2])) & 1;
            errors += __popcll(__ballot(rvalid[rr] && par));
        }
        if (errors < min_errors) {
            min_errors = errors;
            if (errors == 0) return true;
        }
        if (iter + 1 >= max_iters) { iter = max_iters; return true; }

        // ---- bits -> checks: toc[m][n_idx] = fast_tanh(-Tnm / 2)
        f2 t[4];
#pragma unroll
        for (int r = 0; r < 2; ++r) t[r] = tanh_pair<FAST>(X[r]);
        t[3] = tanh_pair<FAST>(Y);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            toc[slot[3 * r + 1]] = t[r].x;
            toc[slot[3 * r + 2]] = t[r].y;
        }
        toc[slot[0]] = t[3].x;
        toc[slot[3]] = t[3].y;
        if (has[2]) {
            t[2] = tanh_pair<FAST>(X[2]);
            const float tz = tanh_one<FAST>(z);
            toc[slot[7]] = t[2].x;
            toc[slot[8]] = t[2].y;
            toc[slot[6]] = tz;
        }
        return false;
    };

    for (;; ++iter) {
        if (iter >= max_iters) break;
        const bool stop = fast_ok ? first_half(std::true_type{}) : first_half(std::false_type{});
        if (stop) break;
        wave_lds_sync();

        // ---- check rows: ordered products that skip one member, for all members ---------------
        if (has6) {
            const float4 lo = planeLO[row6], hi = planeHI[row6];
            const float v0 = lo.x, v1 = lo.y, v2 = lo.z, v3 = lo.w, v4 = hi.x, v5 = hi.y;
            const f2 o01 = (((f2{ v1, v0 } * v2) * v3) * v4) * v5;
            const float p2 = v0 * v1;
            const float p3 = p2 * v2;
            const float p4 = p3 * v3;
            const f2 o23 = (f2{ p2 * v3, p3 } * v4) * v5;
            const float o4 = p4 * v5, o5 = p4 * v4;
            planeLO[row6] = make_float4(o01.x, o01.y, o23.x, o23.y);
            *reinterpret_cast<float2 *>(planeHI + row6) = make_float2(o4, o5);
        }
        if (has7) {
            const float4 lo = planeLO[row7], hi = planeHI[row7];
            const float v0 = lo.x, v1 = lo.y, v2 = lo.z, v3 = lo.w, v4 = hi.x, v5 = hi.y, v6 = hi.z;
            const f2 o01 = ((((f2{ v1, v0 } * v2) * v3) * v4) * v5) * v6;
            const float p2 = v0 * v1;
            const float p3 = p2 * v2;
            const float p4 = p3 * v3;
            const float p5 = p4 * v4;
            const f2 o23 = ((f2{ p2 * v3, p3 } * v4) * v5) * v6;
            const f2 o45 = f2{ p4 * v5, p5 } * v6;
            const float o6 = p5 * v5;
            planeLO[row7] = make_float4(o01.x, o01.y, o23.x, o23.y);
            planeHI[row7] = make_float4(o45.x, o45.y, o6, 1.0f);
        }
        wave_lds_sync();

#pragma unroll
        for (int r = 0; r < 2; ++r) PA[r] = f2{ toc[slot[3 * r + 2]], toc[slot[3 * r + 1]] };
        PB = f2{ toc[slot[0]], toc[slot[3]] };
        PA[2] = f2{ toc[slot[8]], toc[slot[7]] };
        pc = toc[slot[6]];
        float mabs = min3_abs(pc, PA[2].x, PA[2].y);
        mabs = has[2] ? mabs : __builtin_inff();
        mabs = min3_abs(mabs, PB.x, PB.y);
        mabs = min3_abs(mabs, PA[0].x, PA[0].y);
        mabs = min3_abs(mabs, PA[1].x, PA[1].y);
        bool guard_ok = __all(mabs >= 0x1p-59f);
        if (!guard_ok) {                                              // wave-uniform
            uint32_t g2 = min(guard_key(pc), min(guard_key(PA[2].x), guard_key(PA[2].y)));
            g2 = has[2] ? g2 : 0xFFFFFFFFu;
            uint32_t gmin = min(g2, min(guard_key(PB.x), guard_key(PB.y)));
#pragma unroll
            for (int r = 0; r < 2; ++r) gmin = min(gmin, min(guard_key(PA[r].x), guard_key(PA[r].y)));
            guard_ok = __all(gmin >= kGuardMin);
        }
        fast_ok = guard_ok && !force_ieee_div;
    }

    // ---- judge the word BP left: the first failing check names the result ---------------------------------------------
    const uint64_t w0 = __brevll(B0);                                 // codeword bits 0..63, MSB first
    const uint64_t w1 = __brevll(B1) & 0xFFFFFFE000000000ull;         // bits 64..90
    int result, nhard = 0;
    if (min_errors != 0) result = 7;
    else {
        nhard = __popcll(B0 ^ X0) + __popcll(B1 ^ X1) + __popcll(B2 ^ X2);
        if ((B0 | B1 | B2) == 0ull) result = 5;                       // (bp_decode leaves at an all-zero word before it checks it)
        else {
            uint32_t c = ((B0 >> lane) & 1ull) ? d_cmb.crc_bit[lane] : 0u;
            if (lane < 13 && ((B1 >> lane) & 1ull)) c ^= d_cmb.crc_bit[64 + lane];
            const uint32_t crc_calc = wave_xor(c);
            const uint32_t crc_extracted = (uint32_t)(w1 >> 37) & 0x3FFFu;
            if (crc_extracted != crc_calc) result = 3;
            else {
                // the record of a BP success (decode.hip), iters as it was
                static_assert(offsetof(ft8gpu_decode_status, a91) == 10 && offsetof(ft8gpu_decode_status, text) == 22, "record layout");
                wave_lds_sync();                                      // the sums have been read
                if (lane < 12) {
                    const uint32_t hi0 = (uint32_t)(w0 >> 32), lo0 = (uint32_t)w0, hi1 = (uint32_t)(w1 >> 32);
                    uint32_t v = 0;
                    if (lane == 0) v = dw0 & 0xFFFF0000u;
                    else if (lane == 1) v = crc_extracted | (crc_calc << 16);
                    else if (lane == 2) v = (__builtin_bswap32(hi0) & 0xFFFFu) << 16;
                    else if (lane == 3) v = (__builtin_bswap32(hi0) >> 16) | (__builtin_bswap32(lo0) << 16);
                    else if (lane == 4) v = (__builtin_bswap32(lo0) >> 16) | (__builtin_bswap32(hi1) << 16);
                    else if (lane == 5) v = __builtin_bswap32(hi1) >> 16;
                    rec32[lane] = v;
                }
                wave_lds_sync();
                int rc = 0;
                if (lane == 0) {
                    rc = ft8dev::unpack77(w0, w1 & 0xFFF8000000000000ull, rec + offsetof(ft8gpu_decode_status, text));
                    rec[offsetof(ft8gpu_decode_status, unpack_status)] = (char)rc;
                    rec[offsetof(ft8gpu_decode_status, ok)] = 1;
                }
                rc = __builtin_amdgcn_readfirstlane(rc);
                wave_lds_sync();
                result = rc < 0 ? 4 : 1;
            }
        }
    }
    if (lane < 12 && (result == 1 || out32 != in32)) out32[lane] = result == 1 ? rec32[lane] : mine;
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
            if (own_soft_bits(mag, frame, cands[rec_index], llr, lane, own, has) && lane == 0)
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
        (void)own_soft_bits(mag, frame, cand, llr, lane, own, has);
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
    static CombineTables h;
    for (int r = 0; r < 3; ++r)
        for (int l = 0; l < 64; ++l) {
            const int n = l + 64 * r;
            for (int e = 0; e < 3; ++e) {
                if (n >= kLdpcN) { h.edge_slot[r][l][e] = (uint16_t)slot_index(kRows - 1, e); continue; }
                const int m = kFT8_Mn[n][e] - 1;
                int pos = -1;
                for (int j = 0; j < kFT8_Num_rows[m]; ++j)
                    if (kFT8_Nm[m][j] - 1 == n) pos = j;
                h.edge_slot[r][l][e] = (uint16_t)slot_index(kLdsRowPos[m], pos);
            }
        }
    for (int rr = 0; rr < 2; ++rr)
        for (int l = 0; l < 64; ++l) {
            const int m = l + 64 * rr;
            h.row_valid[rr][l] = m < kLdpcM;
            h.rowmask[rr][l][0] = h.rowmask[rr][l][1] = h.rowmask[rr][l][2] = 0;
            if (m >= kLdpcM) continue;
            for (int j = 0; j < kFT8_Num_rows[m]; ++j) {
                const int n = kFT8_Nm[m][j] - 1;
                h.rowmask[rr][l][n >> 6] |= 1ull << (n & 63);
            }
        }
    // which lane multiplies which row (ldpc_lds_layout.h; decode_tables_init checks the layout's invariants)
    for (int l = 0; l < 64; ++l) {
        h.own6[l] = h.own7[l] = (uint8_t)(kRows - 1);
        const int m6 = kOwn6Row[l], m7 = kOwn7Row[l];
        if (m6 != 255) { if (m6 >= kLdpcM || kFT8_Num_rows[m6] != 6) abort(); h.own6[l] = kLdsRowPos[m6]; }
        if (m7 != 255) { if (m7 >= kLdpcM || kFT8_Num_rows[m7] != 7) abort(); h.own7[l] = kLdsRowPos[m7]; }
    }
    for (int i = 0; i < 77; ++i) {
        // CRC-14, polynomial 0x2757, of the 82-bit message (77 payload bits, five zeros) whose only set bit is i
        uint32_t rem = 0;
        for (int bit = 0; bit < 82; ++bit) {
            if (bit == i) rem ^= 0x2000u;
            rem = (rem & 0x2000u) ? ((rem << 1) ^ 0x2757u) & 0x3FFFu : (rem << 1) & 0x3FFFu;
        }
        h.crc_bit[i] = (uint16_t)rem;
    }
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(d_cmb), &h, sizeof(h), 0, hipMemcpyHostToDevice, s);
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
