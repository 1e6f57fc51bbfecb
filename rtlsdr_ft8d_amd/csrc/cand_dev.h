// cand_dev.h -- device code of the one-wave-per-candidate kernels, kept once: the LDPC kernel (decode.hip) and the kernels
// that give its failures a second chance (osd.hip, ap.hip, match.hip, combine.hip, demod.hip, apsoft.hip).  Wave helpers, the soft bits
// of a candidate and their renormalisation in index order, the BP iteration in its counting form, the judgement and the
// record of a success, and the LDPC tables with their host-side builder and upload.  For the five second-chance kernels also
// what surrounds those: the head of the kernel (which candidate a wave has, and whether it is left alone), the launch
// geometry, and the one kernel that tags the message records a stage gained.  decode.hip takes the helpers and the table
// builders from here and keeps its own kernel body (it has forms of the iteration the counting form does not need: the
// scalar group test, registers with unspecified content, broadcast multiplies); its comments explain the layout the
// counting form shares.
// Plain functions in the translation unit's anonymous namespace; a __device__ table is instantiated by the file that uses it.
#pragma once
#include "ft8gpu_internal.h"
#include "ft8_tables.h"
#include "unpack_dev.h"
#include "bp_math.h"
#include "ldpc_lds_layout.h"
#include "wave_dev.h"
#include <stddef.h>
#include <stdlib.h>
#include <type_traits>

namespace {

using bpm::f2;
using bpm::tanh_pair;
using bpm::tanh_one;
using bpm::atanh_pair;
using bpm::atanh_one;

__constant__ uint8_t c_gray[8] = { 0, 1, 3, 2, 5, 6, 4, 7 };

constexpr int kRows = 84;                     // 83 check rows + 1 spare row for idle lanes
constexpr int kTocFloats = kRows * 8;         // plane LO: [84] float4 (slots 0..3), plane HI: [84] float4 (slots 4..7)
constexpr int kWaveLds = kTocFloats + 192;    // + 174 LLRs

__host__ __device__ constexpr int slot_index(int m, int pos) {
    return pos < 4 ? 4 * m + pos : 4 * kRows + 4 * m + (pos - 4);
}

// min(|a|, |b|, |c|) in one instruction (no canonicalising copies of the operands)
__device__ __forceinline__ float min3_abs(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// a + b as one v_add_f32 the vectoriser cannot see through
__device__ __forceinline__ float add_f32(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Guard key of a value: (bits << 1) - 1 as unsigned.  Zero maps to 0xFFFFFFFF, every other value to
// twice its magnitude bits minus one, so "minimum key over a set >= key(T)" says: each member is
// zero or at least T in magnitude.
//
// ONE guard per iteration, on the nine row products P of the lane, with T = 2^-59, covers both
// division sites of the following work:
//   * fast_atanh(P): numerator P*(945 - 735P^2 + 64P^4) with |P| <= 1.0072^6, so |numerator| >= 200|P|;
//   * the state ah = fast_atanh(P) (tov = -2*ah) then satisfies ah == 0 or |ah| >= 2^-59 (|atanh_r(P)| >= |P|),
//     and the halved LLRs cwh are 0 or >= 0.0095 (an integer times sqrt(24/variance)/2, variance <= 255^2).
//     Any sum of two or three floats that are each 0 or >= 2^-59 is 0 or >= 2^-82 (all are multiples of
//     2^-82), hence the next iteration's x is 0 or >= 2^-82, and fast_tanh's numerator x*(945 + ...) >= 945|x|.
// Both are far above v_div_scale's 2^-103 rescaling threshold.  Large, infinite and NaN values need
// no guard: |x| > 4.97 is overridden by fast_tanh's clamp in either division form, the products are
// bounded, and NaN stays NaN through both forms.  Iteration 0 starts from tov = 0.
//
// The products of iteration 0 satisfy the guard by construction, so the LDPC kernel does not evaluate it for them
// (exact-zero LLRs -- differences of bytes -- are common, and each would send the quick form on to the exact key test).  Proof:
//   * in iteration 0 every message is x = cwh + 0 + 0 = cwh = -(k * f) / 2 with an integer |k| <= 255 and
//     f = sqrtf(24 / variance).  variance = (sum2 - sum^2/174) / 174 <= sum2 / 174 <= 255^2, so f >= sqrt(24)/255 >
//     0.0192 and x is 0 or |x| >= 0.0096 > 2^-6.71 (f infinite or NaN -- variance 0 or, by rounding, below 0 -- gives
//     infinite or NaN x: no guard needed, see above);
//   * t = fast_tanh(x) = x r(x^2) with r(u) = (945 + 105 u + u^2) / (945 + 420 u + 15 u^2): zero only for x = 0.
//     r falls on u >= 0 (the numerator of r' is -297675 - 26460 u - 1155 u^2), so for |x| <= 4.97 it is at least
//     r(4.97^2) = 0.2026, hence |t| >= 0.2026 * 0.0096 > 2^-9.01; beyond 4.97 the clamp gives |t| = 1.  The handful of
//     roundings in f, x and t move these by parts in 2^-22: take |t| > 2^-9.1;
//   * a row product multiplies at most six such t (rows have six or seven members and skip one); |t| <= 1.0073, so no
//     partial product leaves the normal range, none is zero unless a factor is, and each of the five roundings loses
//     at most 2^-24 of the value: P is 0 or |P| > 2^-54.6 (1 - 2^-24)^5 > 2^-55 > 2^-59 = T.
// (What the guard of iteration k > 0 sees depends on the sums of messages and has no such bound.)
__device__ __forceinline__ uint32_t guard_key(float v) { return (__float_as_uint(v) << 1) - 1u; }
constexpr uint32_t kGuardMin = ((127u - 59u) << 24) - 1u;       // guard_key(0x1p-59f)

// sum over the 64 lanes with DPP adds (no LDS crossbar round trips); the total comes back uniform
__device__ __forceinline__ int wave_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);   // row_mirror: every lane holds its row's sum
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, true);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, true);   // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

// the same reduction with XOR (CRC contributions of the set payload bits)
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
// the smallest / largest of 64 values (once per candidate: plain butterflies)
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// ---- the soft bits of a candidate -----------------------------------------------------------------------------------------
// ft8_extract_likelihood and ftx_normalize_logl as the LDPC kernel forms them: lane k < 58 owns data symbol k, 8 waterfall
// bytes -> three max-log differences; the values are small integers, so the reference's sequential float sums are exact in
// any order and are reduced across the wave in integer arithmetic (decode.hip).  llr: 192 floats of the wave's LDS (the raw
// soft bits stay there); lane l gets llr[l], llr[l + 64], llr[l + 128] normalised (0 past 173) and has[r] = l + 64 r < 174.
// Returns whether every value is finite (wave-uniform).  Every lane takes part.
__device__ __forceinline__ bool soft_bits(const uint8_t *__restrict__ mag, int frame, const ft8gpu_candidate cand, float *llr,
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
            for (int j = 0; j < 8; ++j) s2[j] = ps[c_gray[j]];
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

// ftx_normalize_logl on 174 soft bits of any origin (a sum across slots, magnitudes of correlations): llr[0 .. 173] in the
// wave's LDS, stores published; lane l gets llr[l + 64 r] normalised into cw[r] (0 where !has[r]).  The normaliser
// accumulates in index order as the reference does -- every lane reads the 174 values at one address and keeps the same
// two accumulators, so no reduction order has to be argued about.  Returns whether every value is finite (wave-uniform);
// if so, ieee is set where the division guard below fails.
//
// The division guard.  guard_key's comment proves that iteration 0 needs no guard because every soft bit there is k * f / 2
// with an integer k and f >= 0.0192, and ap.hip relies on the same fact.  Renormalised values have no such structure: x[i] is
// any finite float, 2^-90 or a subnormal next to values of ordinary size.  The soft bits enter the messages of EVERY iteration
// (x = (cwh + ah_a) + ah_b), and the argument of guard_key -- a sum of floats that are each 0 or >= 2^-59 is 0 or
// >= 2^-82, nothing is subnormal, halving commutes with every rounding -- needs cwh = -x / 2 in that set as well.  So the
// guard is evaluated ahead of iteration 0 on the candidate's own 174 soft bits, with the same key test as on the row
// products: every x[i] is 0 or |x[i]| >= 2^-58 (tested on x, not on the halved value, which may round a subnormal to zero).
// Where it holds, iteration 0 runs the fast form (x = cwh is in fast_tanh's domain) and every later iteration is guarded on
// its products (bp_decode_counting evaluates the guard after iteration 0 too); where it fails the whole candidate runs in
// the IEEE form, iteration 0 included.  That is sufficient: with all soft bits in the set, the premise of the proof for
// iteration k > 0 holds unchanged, and the IEEE form needs no premise.
constexpr uint32_t kGuardMinSoft = ((127u - 58u) << 24) - 1u;   // guard_key(0x1p-58f): the soft bits, halved exactly to >= 2^-59
__device__ __forceinline__ bool renormalise_in_order(const float *llr, const bool (&has)[3], int lane, float (&cw)[3], int &ieee) {
    float sum = 0.0f, sum2 = 0.0f;
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
    if (!__all(finite)) return false;
    if (!__all(gk >= kGuardMinSoft)) ieee = 1;        // a soft bit outside the set sends every iteration to the IEEE form
    return true;
}

// A row of normalised soft bits another stage left in global memory (demod.hip's soft array, FT8GPU_SOFT_STRIDE floats a row:
// apsoft.hip): the 174 values go to llr[0 .. 173] of the wave's LDS, stores published, and lane l gets row[l + 64 r] into cw[r]
// (0 where !has[r]; elements 174 and 175 are not read).  Nothing is normalised again.  Returns whether the row is usable
// (wave-uniform): every value finite and apmag = max |row[i]| != 0.  The values are arbitrary finite floats, so the division
// guard is evaluated here, ahead of iteration 0, exactly as renormalise_in_order does: ieee is set where a value is neither 0
// nor >= 2^-58 in magnitude.  apmag is one of the row's own magnitudes, so values forced to +-apmag stay inside the set.
// (The copy in llr is for stages that read soft bits from LDS, as OSD and match do; the only caller so far, apsoft.hip, works
// from cw and composes its record over llr, so there the stores and the sync behind them serve nobody yet.)
__device__ __forceinline__ bool load_soft_row(const float *__restrict__ row, float *llr, const bool (&has)[3], int lane,
                                              float (&cw)[3], float &apmag, int &ieee) {
    bool finite = true;
    uint32_t gk = 0xFFFFFFFFu, amax = 0u;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        cw[r] = 0.0f;
        if (has[r]) {
            cw[r] = row[lane + 64 * r];
            llr[lane + 64 * r] = cw[r];
        }
        const uint32_t a = __float_as_uint(cw[r]) & 0x7FFFFFFFu;
        finite = finite && (a & 0x7F800000u) != 0x7F800000u;
        amax = max(amax, a);
        gk = min(gk, guard_key(cw[r]));
    }
    wave_lds_sync();
    if (!__all(finite)) return false;
    apmag = __uint_as_float(wave_max(amax));                          // non-negative floats order as their bit patterns
    if (apmag == 0.0f) return false;
    if (!__all(gk >= kGuardMinSoft)) ieee = 1;
    return true;
}

// hard decision (llr > 0, on the bit pattern) and 8-bit weight of a soft bit; neither where the position does not exist
__device__ __forceinline__ void hard_and_weight(uint32_t bits, bool valid, bool &hbit, int &w) {
    const float a = __uint_as_float(bits & 0x7FFFFFFFu);
    hbit = valid && (bits >> 31) == 0u && (bits & 0x7FFFFFFFu) != 0u;
    w = a >= 32.0f ? 255 : (int)(a * 8.0f);
    w = valid ? w : 0;
}
// sum of the weights over the set bits of x: 8-bit weights as eight bit planes (osd.hip, match.hip)
__device__ __forceinline__ uint32_t metric_of(const uint64_t x[3], const uint64_t (&P)[8][3]) {
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b)
        m += (uint32_t)(__popcll(x[0] & P[b][0]) + __popcll(x[1] & P[b][1]) + __popcll(x[2] & P[b][2])) << b;
    return m;
}

// ---- a wave and its candidate's record ------------------------------------------------------------------------------------
static_assert(sizeof(ft8gpu_decode_status) == 48, "record is 12 dwords");
static_assert(offsetof(ft8gpu_decode_status, a91) == 10 && offsetof(ft8gpu_decode_status, text) == 22, "record layout");

// ok == 0 and ldpc_errors != 0 from the record's dwords 0 and 2
__device__ __forceinline__ bool still_failing(uint32_t dw0, uint32_t dw2) { return ((dw2 >> 8) & 0xFFu) == 0u && (dw0 & 0xFFFFu) != 0u; }

// the record's 12 dwords, one per lane (status_out may be status_in: read first), dword 0 for every lane, and whether the
// candidate qualifies for a second chance
__device__ __forceinline__ bool read_record(const uint32_t *in32, int lane, uint32_t &mine, uint32_t &dw0) {
    mine = lane < 12 ? in32[lane] : 0u;
    dw0 = (uint32_t)__builtin_amdgcn_readlane((int)mine, 0);
    return still_failing(dw0, (uint32_t)__builtin_amdgcn_readlane((int)mine, 2));
}
// the wave leaves its candidate as it is: the record copied, info = { code, 0 } (demod.hip: { code, 0, 0, 0 })
__device__ __forceinline__ void leave_record(uint32_t *out32, const uint32_t *in32, uint32_t *info32, uint32_t mine, uint32_t code,
                                             int lane, int info_dwords = 2) {
    if (lane < 12 && out32 != in32) out32[lane] = mine;
    if (lane < info_dwords) info32[lane] = lane == 0 ? code : 0u;
}

// The head of a second-chance kernel: one wave64 per candidate, four per workgroup, the launch geometry of the LDPC kernel.
// vb is the workgroup's place in frame order (blockIdx.x, or what ap.hip's XCD renumbering makes of it; kMulHigh: ap.hip's
// division by the launcher's magic, and none at all for one block per frame).  The verdict, wave-uniform:
//   gone  outside the bounds or behind the frame's count: nothing is read or written, records behind the count keep their
//         bytes, and nothing of the struct but the verdict is set (zeros would cost a gone wave moves: a launch of gone
//         waves only took 2 % longer with them);
//   left  the candidate does not qualify for a second chance (marked: or the select kernel's mark in dword 0 of its info
//         record is 0, demod.hip): its record is copied, its info record zeroed;
//   run   status_out may be status_in, so `mine` holds the record as it was.
// (match.hip carries these lines written out; its kernel says why.)
enum CandVerdict { kCandGone, kCandLeft, kCandRun };
struct CandWave {
    int lane, wave, frame, ci;
    size_t rec_index;
    const uint32_t *in32;
    uint32_t *out32, *info32;
    uint32_t mine, dw0;
    CandVerdict verdict;
};
template <bool kMulHigh = false, class Info>
__device__ __forceinline__ CandWave cand_prologue(unsigned vb, unsigned blocks_per_frame, unsigned bpf_magic, const int32_t *counts,
                                                  const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, Info *info,
                                                  int nframes, int max_candidates, bool marked = false) {
    static_assert(sizeof(ft8gpu_decode_status) == 48 && sizeof(Info) % 4 == 0, "record sizes");
    CandWave w;
    w.lane = threadIdx.x & 63;
    w.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    w.frame = !kMulHigh ? (int)(vb / blocks_per_frame) : (blocks_per_frame == 1u ? (int)vb : (int)__umulhi(vb, bpf_magic));
    w.ci = (int)(vb - (unsigned)w.frame * blocks_per_frame) * 4 + w.wave;
    w.verdict = kCandGone;
    if (w.frame >= nframes || w.ci >= max_candidates) return w;
    if (w.ci >= counts[w.frame]) return w;
    w.rec_index = (size_t)w.frame * max_candidates + w.ci;
    w.in32 = reinterpret_cast<const uint32_t *>(status_in + w.rec_index);
    w.out32 = reinterpret_cast<uint32_t *>(status_out + w.rec_index);
    w.info32 = reinterpret_cast<uint32_t *>(info + w.rec_index);
    bool run = read_record(w.in32, w.lane, w.mine, w.dw0);
    if (marked) run = (uint32_t)__builtin_amdgcn_readfirstlane((int)w.info32[0]) != 0u && run;
    w.verdict = run ? kCandRun : kCandLeft;
    if (!run) leave_record(w.out32, w.in32, w.info32, w.mine, 0u, w.lane, (int)(sizeof(Info) / 4));
    return w;
}
// the wave's last store: the composed record of a success, the record as it was otherwise
__device__ __forceinline__ void store_record(uint32_t *out32, const uint32_t *in32, const uint32_t *rec32, uint32_t mine,
                                             bool accepted, int lane) {
    if (lane < 12 && (accepted || out32 != in32)) out32[lane] = accepted ? rec32[lane] : mine;
}

// The record of a BP success for the word (B0, B1) (codeword bit i is bit i & 63 of B{i >> 6}), ldpc_errors 0 and iters as
// dw0 has it, composed in 12 dwords of LDS by lanes 0..5 (a91[k] = byte k of (w0, w1) in big-endian order; record byte
// 10 + k); unpack77 on lane 0 works on the two 64-bit words and stores its characters straight into the record's text.
// Nothing of it lives in private memory.  Returns unpack77's status (wave-uniform); ok = 1 either way, the caller stores the
// record only where the status is not negative.
__device__ __forceinline__ int compose_record(uint64_t B0, uint64_t B1, uint32_t dw0, uint32_t crc_extracted, uint32_t crc_calc,
                                              uint32_t *rec32, int lane) {
    const uint64_t w0 = __brevll(B0);                                 // codeword bits 0..63, MSB first
    const uint64_t w1 = __brevll(B1) & 0xFFFFFFE000000000ull;         // bits 64..90
    char *rec = reinterpret_cast<char *>(rec32);
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
    return rc;
}
// CRC-14 by linearity (init 0, no final XOR: the CRC of a message is the XOR of the CRCs of its set bits, crc_bit[i] that of
// payload bit i; lane l holds payload bits l and, for l < 13, 64 + l), then the record.  The result code of the word:
// 3 CRC mismatch, 4 unpack77 failed, 1 accepted.
__device__ __forceinline__ int compose_success_record(uint64_t B0, uint64_t B1, uint32_t dw0, const uint16_t *crc_bit,
                                                      uint32_t *rec32, int lane) {
    uint32_t c = ((B0 >> lane) & 1ull) ? crc_bit[lane] : 0u;
    if (lane < 13 && ((B1 >> lane) & 1ull)) c ^= crc_bit[64 + lane];
    const uint32_t crc_calc = wave_xor(c);
    const uint32_t crc_extracted = (uint32_t)(__brevll(B1) >> 37) & 0x3FFFu;          // bits 77..90
    if (crc_extracted != crc_calc) return 3;
    return compose_record(B0, B1, dw0, crc_extracted, crc_calc, rec32, lane) < 0 ? 4 : 1;
}
// The judgement of a word with nhard hard errors, the first failing check names the result: 5 all-zero, 2 more hard errors
// than the gate allows, then CRC and unpack77 as above.
__device__ __forceinline__ int judge_word(uint64_t B0, uint64_t B1, uint64_t B2, int nhard, int max_hard_errors, uint32_t dw0,
                                          const uint16_t *crc_bit, uint32_t *rec32, int lane) {
    if ((B0 | B1 | B2) == 0ull) return 5;
    if (nhard > max_hard_errors) return 2;
    return compose_success_record(B0, B1, dw0, crc_bit, rec32, lane);
}

// ---- the LDPC tables ------------------------------------------------------------------------------------------------------
struct LdpcTables {
    uint16_t edge_slot[3][64][3];     // [r][lane][m_idx] -> float index of slot (m, pos) in the LDS tile
    uint64_t rowmask[2][64][3];       // [rr][lane][word] bit mask of the variables of check m = lane + 64 rr
    uint8_t  row_valid[2][64];
    uint8_t  own6[64], own7[64];      // product ownership: lane l computes the products of 6-member row own6[l] (59 rows) and of
                                      // 7-member row own7[l] (24 rows); kRows - 1 (the spare row) = none
    uint16_t crc_bit[77];             // CRC-14 (over 82 bits) of the message whose only set bit is payload bit i
};

// ftx_compute_crc(a91 with bits 77.. cleared, 82 bits): CRC-14, polynomial 0x2757.  Bit-serial
// restatement (only the first 77 bits can be set; five zero bits follow).  Runs on the host when the tables are
// built: the kernels use the linearity of the CRC, so each lane contributes the table entries of the payload bits it
// holds and one DPP reduction replaces 82 dependent shift/xor steps on a single lane.
__host__ __device__ inline uint32_t crc14_82(const uint8_t *msg) {
    uint32_t rem = 0;
    int idx_byte = 0;
    for (int bit = 0; bit < 82; ++bit) {
        if ((bit & 7) == 0) rem ^= (uint32_t)msg[idx_byte++] << 6;
        if (rem & 0x2000u) rem = ((rem << 1) ^ 0x2757u) & 0xFFFFu;
        else rem = (rem << 1) & 0xFFFFu;
    }
    return rem & 0x3FFFu;
}

// host side: the tables' fields from ft8_tables.h and the generated layout (ldpc_lds_layout.h, whose invariants
// decode_tables_init checks when a context is created, ahead of every other use)
inline void fill_edge_slots(uint16_t (&edge_slot)[3][64][3]) {
    for (int r = 0; r < 3; ++r)
        for (int l = 0; l < 64; ++l) {
            const int n = l + 64 * r;
            for (int e = 0; e < 3; ++e) {
                if (n >= kLdpcN) { edge_slot[r][l][e] = (uint16_t)slot_index(kRows - 1, e); continue; }
                const int m = kFT8_Mn[n][e] - 1;
                int pos = -1;
                for (int j = 0; j < kFT8_Num_rows[m]; ++j)
                    if (kFT8_Nm[m][j] - 1 == n) pos = j;
                // the row's place in the LDS tile comes from the conflict-minimising layout; its members keep their order
                edge_slot[r][l][e] = (uint16_t)slot_index(kLdsRowPos[m], pos);
            }
        }
}
inline void fill_rowmasks(uint64_t (&rowmask)[2][64][3], uint8_t (&row_valid)[2][64]) {
    for (int rr = 0; rr < 2; ++rr)
        for (int l = 0; l < 64; ++l) {
            const int m = l + 64 * rr;
            row_valid[rr][l] = m < kLdpcM;
            rowmask[rr][l][0] = rowmask[rr][l][1] = rowmask[rr][l][2] = 0;
            if (m >= kLdpcM) continue;
            for (int j = 0; j < kFT8_Num_rows[m]; ++j) {
                const int n = kFT8_Nm[m][j] - 1;
                rowmask[rr][l][n >> 6] |= 1ull << (n & 63);
            }
        }
}
// which lane multiplies which row: also from the layout search (the float4 accesses of the owners want distinct positions
// mod 16 within their lane groups)
inline void fill_owners(uint8_t (&own6)[64], uint8_t (&own7)[64]) {
    for (int l = 0; l < 64; ++l) {
        const int m6 = kOwn6Row[l], m7 = kOwn7Row[l];
        own6[l] = m6 != 255 ? kLdsRowPos[m6] : (uint8_t)(kRows - 1);
        own7[l] = m7 != 255 ? kLdsRowPos[m7] : (uint8_t)(kRows - 1);
    }
}
inline void fill_crc_bits(uint16_t (&crc_bit)[77]) {
    for (int i = 0; i < 77; ++i) {
        uint8_t m[12] = { 0 };
        m[i >> 3] = (uint8_t)(0x80u >> (i & 7));                 // payload bit i, MSB first (pack_bits order)
        crc_bit[i] = (uint16_t)crc14_82(m);
    }
}
inline void fill_ldpc_tables(LdpcTables &h) {
    fill_edge_slots(h.edge_slot);
    fill_rowmasks(h.rowmask, h.row_valid);
    fill_owners(h.own6, h.own7);
    fill_crc_bits(h.crc_bit);
}
// the tables into a translation unit's own __device__ LdpcTables (symbol = HIP_SYMBOL of it; the copy reads a static object)
inline hipError_t upload_ldpc_tables(const LdpcTables &symbol, hipStream_t s) {
    static LdpcTables h;
    fill_ldpc_tables(h);
    return hipMemcpyToSymbolAsync(symbol, &h, sizeof(h), 0, hipMemcpyHostToDevice, s);
}

// ---- bp_decode, counting form -------------------------------------------------------------------------------------------
// the per-lane constants of the iteration: the LDS slots of the lane's nine edges, the masks of its two check rows, the rows
// whose products it forms
struct LdpcLane {
    int slot[9];
    uint64_t rmask[2][3];
    bool rvalid[2];
    int row6, row7;
    bool has6, has7;
};
__device__ __forceinline__ LdpcLane ldpc_lane(const LdpcTables &t, int lane) {
    LdpcLane L;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int e = 0; e < 3; ++e) L.slot[3 * r + e] = t.edge_slot[r][lane][e];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        L.rvalid[rr] = t.row_valid[rr][lane] != 0;
#pragma unroll
        for (int w = 0; w < 3; ++w) L.rmask[rr][w] = t.rowmask[rr][lane][w];
    }
    L.row6 = t.own6[lane];
    L.row7 = t.own7[lane];
    L.has6 = L.row6 != kRows - 1;
    L.has7 = L.row7 != kRows - 1;
    return L;
}

// the word BP leaves (codeword bit i is bit i & 63 of B{i >> 6}), ldpc_check's smallest error count and the exit iteration
struct BpWord {
    uint64_t B0, B1, B2;
    int min_errors, iter;
};

// bp_decode (ft8_lib ldpc.c) on the soft bits cw (lane l: variables l, l + 64, l + 128), the iteration of the LDPC kernel
// with ldpc_check's exact error count on every iteration (ft8_decode_kernel<true, 1>; the comments of decode.hip explain the
// half domain, the register layout and the check-row products).  toc: the wave's kTocFloats floats of LDS; the spare row is
// seeded here, behind a sync that ends the caller's earlier reads of the tile.  Every lane takes part.
// The division guard (guard_key has the argument): both division streams sit behind one wave-uniform branch per iteration,
// fast_ok chooses, and it is evaluated on the row products after EVERY iteration, iteration 0 included -- decode.hip's
// proof that iteration 0 needs none rests on soft bits that are k * f / 2, and these callers alter them.  A caller whose
// soft bits may lie outside { 0, |x| >= 2^-58 } passes force_ieee_div (combine.hip); a-priori values of the candidate's own
// largest magnitude stay inside (ap.hip).
__device__ __forceinline__ BpWord bp_decode_counting(const float (&cw)[3], const bool (&has)[3], uint64_t has2_mask, float *toc,
                                                     const LdpcLane &L, int lane, int max_iters, int force_ieee_div) {
    float4 *planeLO = reinterpret_cast<float4 *>(toc);
    float4 *planeHI = planeLO + kRows;
    // the spare row only needs finite content (idle lanes of the variable side read and write it)
    wave_lds_sync();
    if (lane < 8) toc[slot_index(kRows - 1, lane)] = 1.0f;
    wave_lds_sync();

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
            const int par = (__popcll(B0 & L.rmask[rr][0]) + __popcll(B1 & L.rmask[rr][1]) + __popcll(B2 & L.rmask[rr][2])) & 1;
            errors += __popcll(__ballot(L.rvalid[rr] && par));
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
            toc[L.slot[3 * r + 1]] = t[r].x;
            toc[L.slot[3 * r + 2]] = t[r].y;
        }
        toc[L.slot[0]] = t[3].x;
        toc[L.slot[3]] = t[3].y;
        if (has[2]) {
            t[2] = tanh_pair<FAST>(X[2]);
            const float tz = tanh_one<FAST>(z);
            toc[L.slot[7]] = t[2].x;
            toc[L.slot[8]] = t[2].y;
            toc[L.slot[6]] = tz;
        }
        // The sync that publishes the stores to the check rows' owners sits here, inside, on purpose: the branch on has[2]
        // is the only divergent one of this function, and with nothing behind it the compiler merges its join into the
        // block where the loop's exits meet -- iter, min_errors and the ballot words then count as divergent, the loop
        // runs under EXEC masks and unpack77 moves from the scalar unit to the vector unit (a combine launch that runs BP
        // on every candidate then takes 6 % longer).
        wave_lds_sync();
        return false;
    };

    for (;; ++iter) {
        if (iter >= max_iters) break;
        const bool stop = fast_ok ? first_half(std::true_type{}) : first_half(std::false_type{});
        if (stop) break;                                 // (first_half has synchronised the wave's LDS accesses)

        // ---- check rows: ordered products that skip one member, for all members ---------------
        if (L.has6) {
            const float4 lo = planeLO[L.row6], hi = planeHI[L.row6];
            const float v0 = lo.x, v1 = lo.y, v2 = lo.z, v3 = lo.w, v4 = hi.x, v5 = hi.y;
            const f2 o01 = (((f2{ v1, v0 } * v2) * v3) * v4) * v5;
            const float p2 = v0 * v1;
            const float p3 = p2 * v2;
            const float p4 = p3 * v3;
            const f2 o23 = (f2{ p2 * v3, p3 } * v4) * v5;
            const float o4 = p4 * v5, o5 = p4 * v4;
            planeLO[L.row6] = make_float4(o01.x, o01.y, o23.x, o23.y);
            *reinterpret_cast<float2 *>(planeHI + L.row6) = make_float2(o4, o5);
        }
        if (L.has7) {
            const float4 lo = planeLO[L.row7], hi = planeHI[L.row7];
            const float v0 = lo.x, v1 = lo.y, v2 = lo.z, v3 = lo.w, v4 = hi.x, v5 = hi.y, v6 = hi.z;
            const f2 o01 = ((((f2{ v1, v0 } * v2) * v3) * v4) * v5) * v6;
            const float p2 = v0 * v1;
            const float p3 = p2 * v2;
            const float p4 = p3 * v3;
            const float p5 = p4 * v4;
            const f2 o23 = ((f2{ p2 * v3, p3 } * v4) * v5) * v6;
            const f2 o45 = f2{ p4 * v5, p5 } * v6;
            const float o6 = p5 * v5;
            planeLO[L.row7] = make_float4(o01.x, o01.y, o23.x, o23.y);
            planeHI[L.row7] = make_float4(o45.x, o45.y, o6, 1.0f);
        }
        wave_lds_sync();

#pragma unroll
        for (int r = 0; r < 2; ++r) PA[r] = f2{ toc[L.slot[3 * r + 2]], toc[L.slot[3 * r + 1]] };
        PB = f2{ toc[L.slot[0]], toc[L.slot[3]] };
        PA[2] = f2{ toc[L.slot[8]], toc[L.slot[7]] };
        pc = toc[L.slot[6]];
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
    return BpWord{ B0, B1, B2, min_errors, iter };
}
// The word BP left on soft bits whose hard decisions are X, judged: 7 no codeword (nhard stays 0), then judge_word on its
// hard errors.  The record is composed where the soft bits were (combine.hip, demod.hip): the sync ends their reads.
__device__ __forceinline__ int judge_bp_word(const BpWord &bp, uint64_t X0, uint64_t X1, uint64_t X2, int max_hard_errors,
                                             uint32_t dw0, const uint16_t *crc_bit, uint32_t *rec32, int lane, int &nhard) {
    nhard = 0;
    if (bp.min_errors != 0) return 7;
    nhard = __popcll(bp.B0 ^ X0) + __popcll(bp.B1 ^ X1) + __popcll(bp.B2 ^ X2);
    wave_lds_sync();
    return judge_word(bp.B0, bp.B1, bp.B2, nhard, max_hard_errors, dw0, crc_bit, rec32, lane);   // (BP leaves at an all-zero word unchecked)
}

// One a-priori hypothesis on a candidate (ap.hip, hint.hip; include/ft8gpu.h "a-priori decoding"): the masked positions
// (m0, m1 over codeword positions 0..63 and 64..127, bits b0, b1) become +-apmag, BP runs on the result, and the word it
// leaves is judged against the candidate's hard decisions (H0, H1, H2) -- 7 no codeword, 8 it differs from the hypothesis on a
// masked position, then judge_word on the hard errors of the unmasked positions.  The record of an accepted word is composed
// in rec32.  Wave-uniform arguments but cw0 / has; returns the result code.
// (ap.hip carries these lines written out in its loop: called from there, the routine gives the same results but moves the
// kernel's blocks and registers, and ft8_ap_kernel is kept instruction for instruction what it was.)
__device__ __forceinline__ int ap_try(const float (&cw0)[3], const bool (&has)[3], uint64_t has2_mask, float *toc, const LdpcLane &L,
                                      int lane, int max_iters, int force_ieee_div, float apmag, uint64_t m0, uint64_t m1, uint64_t b0,
                                      uint64_t b1, uint64_t H0, uint64_t H1, uint64_t H2, int max_hard_errors, uint32_t dw0,
                                      const uint16_t *crc_bit, uint32_t *rec32, int &nhard, int &iters_out) {
    float cw[3];
    {
        const bool f0 = ((m0 >> lane) & 1ull) != 0ull, f1 = ((m1 >> lane) & 1ull) != 0ull;
        cw[0] = f0 ? (((b0 >> lane) & 1ull) ? apmag : -apmag) : cw0[0];
        cw[1] = f1 ? (((b1 >> lane) & 1ull) ? apmag : -apmag) : cw0[1];
        cw[2] = cw0[2];
    }
    const BpWord bp = bp_decode_counting(cw, has, has2_mask, toc, L, lane, max_iters, force_ieee_div);
    const uint64_t B0 = bp.B0, B1 = bp.B1, B2 = bp.B2;
    iters_out = bp.iter < 255 ? bp.iter : 255;
    // hard errors: unmasked positions at which the word differs from h (the mask covers payload positions only)
    nhard = __popcll((B0 ^ H0) & ~m0) + __popcll((B1 ^ H1) & ~m1) + __popcll(B2 ^ H2);
    int result;
    if (bp.min_errors != 0) result = 7;
    else if ((((B0 ^ b0) & m0) | ((B1 ^ b1) & m1)) != 0ull) result = 8;
    else result = judge_word(B0, B1, B2, nhard, max_hard_errors, dw0, crc_bit, rec32, lane);
    return result;
}

// ---- launch geometry and the tags of what a stage gained ----------------------------------------------------------------
// one workgroup per 4 candidates: bpf blocks (of 4 candidate waves) per frame, frame after frame.  mul_high: ap.hip's
// tighter bound, which keeps its multiply-high division exact.
struct CandGrid { unsigned bpf, nblocks; };
inline hipError_t cand_grid(int nframes, int max_candidates, CandGrid &g, bool mul_high = false) {
    g.bpf = (unsigned)(max_candidates + 3) / 4;
    const unsigned long long nblocks = (unsigned long long)nframes * g.bpf;
    g.nblocks = (unsigned)nblocks;
    return nblocks >= (1ull << 31) || (mul_high && nblocks * g.bpf >= (1ull << 32)) ? hipErrorInvalidValue : hipSuccess;
}

// What a tag writes into a message record.  TagConst: pad[kPad] = v.  TagInfo: pad[kPad] = kAdd + the byte kField of the info
// record of the message's candidate, [slot][max_candidates]; where cand_index is out of range nothing, or 0 with kElseZero.
template <int kPad>
struct TagConst {
    uint8_t v;
    __device__ void operator()(ft8gpu_message *m, int) const { m->pad[kPad] = v; }
};
template <int kPad, class Info, uint8_t Info::*kField, int kAdd = 0, bool kElseZero = false>
struct TagInfo {
    const Info *info;
    int max_candidates;
    __device__ void operator()(ft8gpu_message *m, int slot) const {
        const int ci = m->cand_index;
        if (ci < max_candidates) m->pad[kPad] = (uint8_t)(kAdd + info[(size_t)slot * max_candidates + ci].*kField);
        else if (kElseZero) m->pad[kPad] = 0;
    }
};
// The message records the append step added to a frame, n_before[frame * stride] <= r < n_msgs[frame], get the stage's tag.
// One wave per slot of the pass, four per workgroup; slot -> frame through map, or the slot itself (map == nullptr).
template <class Tag>
__global__ __launch_bounds__(256)
void ft8_tag_kernel(const int32_t *__restrict__ map, const int32_t *__restrict__ n_before, int stride,
                    const int32_t *__restrict__ n_msgs, int nslots, ft8gpu_message *__restrict__ msgs, Tag tag) {
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), r = threadIdx.x & 63;
    if (slot >= nslots) return;
    const int frame = map ? map[slot] : slot;
    int lo = n_before[(size_t)frame * stride], hi = n_msgs[frame];
    lo = lo < 0 ? 0 : lo;
    hi = hi > kMaxMessages ? kMaxMessages : hi;
    if (r < lo || r >= hi) return;
    tag(msgs + (size_t)frame * kMaxMessages + r, slot);
}
template <class Tag>
inline hipError_t launch_tag(const int32_t *map, const int32_t *n_before, int stride, const int32_t *n_msgs, int nslots,
                             ft8gpu_message *msgs, Tag tag, hipStream_t s) {
    if (nslots < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_tag_kernel<Tag>, dim3((nslots + 3) / 4), dim3(256), 0, s, map, n_before, stride, n_msgs, nslots, msgs, tag);
    return hipGetLastError();
}

}  // namespace
