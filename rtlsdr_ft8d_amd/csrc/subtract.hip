// subtract.hip -- subtraction in the I/Q samples: every record's waveform rebuilt and taken out of the frame (the rule is in
// include/ft8gpu.h "subtraction in the I/Q samples", restated in tests/ft8_spec_subtract.py; DESIGN.md "Subtraction in the I/Q
// samples").
//
//   ft8_subtract_estimate_kernel   one wave per record, four per workgroup (the geometry of refine.hip).
//     frequency search, per symbol: the 512 samples at S_0 go through LDS; lanes (d, segment) dechirp d = -2 .. 1 at once,
//       lanes 0..15 then d = 2; lanes 0..4 add their 16 segment sums and keep the running powers.
//     time search, per symbol: 768 samples from S_0 - 32; lanes (t, segment), t = -2, -1, 1, 2, read their 32 samples at
//       32 + 8 t + 32 segment; t = 0 is the frequency search's best and is not formed again.
//     amplitude, two symbols at a time: lane (symbol, segment) < 32 writes G(q) into a ring of 64 segments; lane l < 32 then
//       adds G(q - 8 .. q + 8) for q = 32 c - 8 + l, multiplies by inv[n] and stores A(q).
//     Every sum of the rule is formed by one lane in the stated order; no value crosses lanes except through LDS.
//   ft8_subtract_apply_kernel      six workgroups per frame, each thread four consecutive aligned samples of I and Q at a time
//     (float4 loads and stores).  S* is a multiple of 8, so the four samples share a record's segment and symbol.  The thread
//     walks the frame's records in order; no atomics.  w4 sits in LDS as 4096 float2 in table order (the lanes' indices are
//     unrelated, so no layout avoids conflicts; one 8-byte read per sample took a third off the kernel against two 4-byte reads
//     of separate planes, and reading the table through L2 instead was slower by 40 %).
//
// LDS of the estimate kernel (72 448 bytes per workgroup, two workgroups per CU): w4 as two planes of 4096 floats, entry i at
// ((i & 31) << 7) | (i >> 5) -- the lanes of a dechirp step read w4[(A + 32 K l) & 4095] for one A, bank ((A >> 5) + K l) & 31: all different for odd K, and
// lanes that share a bank for even K read the same entry; per wave the I and Q planes of 32 segments at 33 floats (sample o at
// o + (o >> 5)), the ring, 160 segment sums and the 80 tones.  No scratch memory.
// Phases: Theta_m = (512 m k4) mod 4096 (the tones' share of the recurrence is whole turns) and every product is formed in
// uint32, which is exact modulo 4096.
//
// Shapes (include/ft8gpu.h "GFSK reference").  Both kernels exist twice, the bodies templated on the shape; the CPFSK kernels
// keep their names, arithmetic and geometry.  ft8_subtract_estimate_gfsk_kernel and ft8_subtract_apply_gfsk_kernel look every
// sample's phase up: phi = (k4 << 20) n' + e[m] Q[k + 1024] + e[m + 1] Q[k + 512] + e[m + 2] Q[k] in wrapping uint32, rounded to
// the w4 table.  Nothing assumes Q linear inside a symbol.  The estimate kernel holds Q in LDS at k + (k >> 5) (1585 dwords,
// 78 788 bytes per workgroup with the rest, still two workgroups per CU): a lane's 32 samples are Q[32 seg + i] and its two
// neighbours 512 apart, so the 16 segments of a dechirp step fall on 16 different banks and lanes of different hypotheses
// read the same entry.  The apply kernel holds Q in table order and reads a thread's four samples as one 16-byte word per
// pulse term (S* is a multiple of 8 and j of 4), and the 64-entry ramp beside it; only the first and last 64 samples of a
// record take the ramp's two extra products.
#include "subtract.h"
#include "span_dev.h"
#include "tone_dev.h"
#include "wave_dev.h"
#include <stddef.h>

namespace {

constexpr int kTab = FT8GPU_SUBTRACT_TABLE;
constexpr uint32_t kTabMask = kTab - 1;
constexpr int kSeg = 32;
constexpr int kSymSegs = 16;
constexpr int kSmooth = FT8GPU_SUBTRACT_SMOOTH;
constexpr int kHyp = 2 * FT8GPU_SUBTRACT_RANGE + 1;            // 5 hypotheses per search
constexpr int kPlaneSegs = 32;
constexpr int kPlane = kPlaneSegs * kStagePitch;               // 1056 floats, stage_span's layout (span_dev.h)
constexpr int kTimeSpanSegs = 24, kFreqSpanSegs = 16, kAmpSpanSegs = 32;   // what the two searches and the amplitude step stage at a time
static_assert(kSeg == kStageSeg && kTimeSpanSegs <= kPlaneSegs && kFreqSpanSegs <= kPlaneSegs && kAmpSpanSegs <= kPlaneSegs, "a staged span fits a plane");
constexpr int kRing = 64;
constexpr int kWaves = 4;
constexpr int kBlocksPerFrame = (kMaxMessages + kWaves - 1) / kWaves;
constexpr int kSpan = FT8GPU_NN * 512;                         // samples of a record
constexpr int kParts = 6;                                      // apply: workgroups per frame
constexpr int kPartSamples = kNSamples / kParts;               // 8000
constexpr int kPulse = 3 * FT8GPU_GFSK_SPS_IQ + 1;                // 1537 entries of Q
constexpr int kPulseSlots = kPulse - 1 + ((kPulse - 1) >> 5) + 1;  // 1585: entry k at k + (k >> 5)
constexpr int kRamp = FT8GPU_GFSK_SPS_IQ / 8;                      // 64 samples of ramp at either end of a record
constexpr uint32_t kHalfStep = 1u << 19;                           // rounds a 2^-32 turn phase to the 4096 steps of w4
static_assert(kPulse <= (int)(sizeof(SubGfskTables::q) / sizeof(uint32_t)) && kRamp == (int)(sizeof(SubGfskTables::ramp) / sizeof(float)), "GFSK tables");
static_assert(kSpan % 4 == 0 && kRamp % 4 == 0, "a thread's four samples share a side of the ramp's ends");
static_assert(kHyp == 5 && kSmooth == 8 && FT8GPU_SUBTRACT_TSTEP == 8 && kTab == 4096, "lane assignment");
static_assert(kPartSamples * kParts == kNSamples && kPartSamples % 4 == 0, "apply parts");
static_assert(sizeof(ft8gpu_message) == 64 && sizeof(ft8gpu_refined) == 48 && sizeof(ft8gpu_subtract_info) == 64, "record sizes");

__device__ __forceinline__ int tab_slot(uint32_t idx) { return (int)((idx & 31u) << 7 | idx >> 5); }

// the sum of z over the 32 staged samples from offset o0 (sample o sits at o + (o >> 5)), whose first phase index is theta and
// whose step is K: sequential from +0
__device__ __forceinline__ void seg_sum(const float *s_i, const float *s_q, const float *s_wr, const float *s_wi, int o0, uint32_t theta,
                                        uint32_t K, float &re, float &im) {
    uint32_t idx = theta & kTabMask;
    float ar = 0.0f, ai = 0.0f;
#pragma unroll 8
    for (int i = 0; i < kSeg; ++i) {
        const int o = o0 + i;
        const int a = o + (o >> 5);
        const float xr = s_i[a], xi = s_q[a];
        const int p = tab_slot(idx);
        const float wr = s_wr[p], wi = s_wi[p];
        ar = ar + (xr * wr - xi * wi);
        ai = ai + (xr * wi + xi * wr);
        idx = (idx + K) & kTabMask;
    }
    re = ar;
    im = ai;
}

// the GFSK phases: the tones around symbol m as e[m], e[m + 1], e[m + 2] (the first and the last tone once more at the ends)
struct Pulse3 {
    uint32_t e0, e1, e2;
};

__device__ __forceinline__ Pulse3 pulse_tones(const int *tone, int m) {
    Pulse3 e;
    e.e0 = (uint32_t)tone[m > 0 ? m - 1 : 0];
    e.e1 = (uint32_t)tone[m];
    e.e2 = (uint32_t)tone[m < FT8GPU_NN - 1 ? m + 1 : FT8GPU_NN - 1];
    return e;
}

// seg_sum with the GFSK phase: the 32 samples are the local samples 512 m + 32 seg + i of a record, phi_lin = step * (512 m +
// 32 seg) and s_pulse holds Q[k] at k + (k >> 5), so Q[32 seg + i] sits at 33 seg + i.  Every sample is looked up.
__device__ __forceinline__ void seg_sum_gfsk(const float *s_i, const float *s_q, const float *s_wr, const float *s_wi,
                                             const uint32_t *s_pulse, int o0, uint32_t phi_lin, uint32_t step, Pulse3 e, int seg,
                                             float &re, float &im) {
    const uint32_t *qc = s_pulse + 33 * seg, *qb = qc + 512 + 16, *qa = qc + 1024 + 32;
    float ar = 0.0f, ai = 0.0f;
#pragma unroll 8
    for (int i = 0; i < kSeg; ++i) {
        const int o = o0 + i;
        const int a = o + (o >> 5);
        const float xr = s_i[a], xi = s_q[a];
        const uint32_t phi = phi_lin + e.e0 * qa[i] + e.e1 * qb[i] + e.e2 * qc[i];
        const int p = tab_slot((phi + kHalfStep) >> 20);
        const float wr = s_wr[p], wi = s_wi[p];
        ar = ar + (xr * wr - xi * wi);
        ai = ai + (xr * wi + xi * wr);
        phi_lin += step;
    }
    re = ar;
    im = ai;
}

struct WaveLds {
    float plane[2][kPlane];
    float ring[2][kRing];
    float sum[2][kHyp * kSymSegs];
    int tone[80];
};

// the powers of the hypotheses of one search.  Frequency: base index k4_base + h - 2, hypothesis h on the lanes 16 h .. 16 h + 15
// of a first round and h = 4 on the lanes 0 .. 15 of a second one.  Time: start S_0 + 8 (h - 2) for h = 0, 1, 3, 4 in one round
// (h = 2 is the frequency search's best, the same sums over the same samples, and is not formed again).
// lane h < 5 returns P of hypothesis h (+0 for h = 2 of the time search).
template <bool kTime, int kShape>
__device__ __forceinline__ float search(const float *__restrict__ pi, const float *__restrict__ pq, WaveLds &L, const float *s_wr,
                                        const float *s_wi, const uint32_t *s_pulse, int S0, int k4_base, int lane) {
    const int grp = lane >> 4, seg = lane & 15;
    float P = 0.0f;
    for (int m = 0; m < FT8GPU_NN; ++m) {
        [[maybe_unused]] const uint32_t tone8 = 8u * (uint32_t)L.tone[m];
        if (kTime) stage_span<kTimeSpanSegs>(pi, pq, S0 - kSeg + 512 * m, L.plane[0], L.plane[1], lane);
        else stage_span<kFreqSpanSegs>(pi, pq, S0 + 512 * m, L.plane[0], L.plane[1], lane);
        wave_lds_sync();
#pragma unroll
        for (int round = 0; round < (kTime ? 1 : 2); ++round) {
            const int h = kTime ? (grp < 2 ? grp : grp + 1) : (round == 0 ? grp : 4);
            if (round == 0 || lane < kSymSegs) {
                const uint32_t k4 = (uint32_t)(kTime ? k4_base : k4_base + h - FT8GPU_SUBTRACT_RANGE);
                const int o0 = kTime ? kSeg + FT8GPU_SUBTRACT_TSTEP * (h - FT8GPU_SUBTRACT_RANGE) + kSeg * seg : kSeg * seg;
                float re, im;
                if constexpr (kShape == FT8GPU_SUBTRACT_GFSK) {
                    const uint32_t step = k4 << 20;
                    seg_sum_gfsk(L.plane[0], L.plane[1], s_wr, s_wi, s_pulse, o0, step * (uint32_t)(512 * m + kSeg * seg), step,
                                 pulse_tones(L.tone, m), seg, re, im);
                } else {
                    const uint32_t K = k4 + tone8;
                    seg_sum(L.plane[0], L.plane[1], s_wr, s_wi, o0, 512u * (uint32_t)m * k4 + K * (uint32_t)(kSeg * seg), K, re, im);
                }
                L.sum[0][kSymSegs * h + seg] = re;
                L.sum[1][kSymSegs * h + seg] = im;
            }
        }
        wave_lds_sync();
        if (lane < kHyp && !(kTime && lane == FT8GPU_SUBTRACT_RANGE)) {
            float cr = 0.0f, ci = 0.0f;
#pragma unroll
            for (int t = 0; t < kSymSegs; ++t) {
                cr = cr + L.sum[0][kSymSegs * lane + t];
                ci = ci + L.sum[1][kSymSegs * lane + t];
            }
            P = P + (cr * cr + ci * ci);
        }
        wave_lds_sync();
    }
    return P;
}

// the first strictly greatest of the five powers held by lanes 0..4, scanned by every lane alike (through L.sum[0][0..4]);
// best: that power
__device__ __forceinline__ int first_max(WaveLds &L, float P, int lane, float &best) {
    if (lane < kHyp) L.sum[0][lane] = P;
    wave_lds_sync();
    best = L.sum[0][0];
    int at = 0;
    for (int h = 1; h < kHyp; ++h) {
        const float v = L.sum[0][h];
        if (v > best) {
            best = v;
            at = h;
        }
    }
    wave_lds_sync();
    return __builtin_amdgcn_readfirstlane(at);
}

// the estimate kernel of either shape (its LDS belongs to the one kernel that calls the instantiation); s_pulse: Q of the GFSK
// shape, neither read nor allocated for CPFSK
template <int kShape>
__device__ __forceinline__ void estimate_body(const float *__restrict__ iq, const ft8gpu_message *__restrict__ msgs,
                                              const ft8gpu_refined *__restrict__ refined, const int32_t *__restrict__ first,
                                              const int32_t *__restrict__ n_msgs, int nframes, const SubTables *__restrict__ tab,
                                              const SubGfskTables *__restrict__ gtab, const MsgTables *__restrict__ mtab,
                                              uint32_t *__restrict__ scratch, ft8gpu_subtract_info *info) {
    __shared__ float s_wr[kTab], s_wi[kTab];
    __shared__ uint32_t s_pulse[kShape == FT8GPU_SUBTRACT_GFSK ? kPulseSlots : 1];
    __shared__ __attribute__((aligned(16))) WaveLds s_wave[kWaves];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int frame = (int)(blockIdx.x / (unsigned)kBlocksPerFrame);
    const int blk = (int)(blockIdx.x - (unsigned)frame * kBlocksPerFrame) * kWaves;
    if (frame >= nframes) return;
    int lo = first[frame], hi = n_msgs[frame];
    lo = lo < 0 ? 0 : (lo > kMaxMessages ? kMaxMessages : lo);
    hi = hi < 0 ? 0 : (hi > kMaxMessages ? kMaxMessages : hi);
    if (blk + kWaves <= lo || blk >= hi) return;                      // workgroup-uniform: nothing of this block is touched

    for (int i = threadIdx.x; i < kTab; i += 256) {
        const float2 w = tab->w4[i];
        const int p = tab_slot((uint32_t)i);
        s_wr[p] = w.x;
        s_wi[p] = w.y;
    }
    if constexpr (kShape == FT8GPU_SUBTRACT_GFSK)
        for (int i = threadIdx.x; i < kPulse; i += 256) s_pulse[i + (i >> 5)] = gtab->q[i];
    __syncthreads();
    const int mi = blk + wave;
    if (mi < lo || mi >= hi) return;                                  // wave-uniform: records outside [first, n_msgs) are not touched

    WaveLds &L = s_wave[wave];
    const size_t ri = (size_t)frame * kMaxMessages + mi;
    const uint32_t *rec32 = reinterpret_cast<const uint32_t *>(msgs + ri);
    const uint32_t *ref32 = reinterpret_cast<const uint32_t *>(refined + ri);
    uint32_t *out = scratch + ri * kSubStride;
    uint32_t *info32 = info ? reinterpret_cast<uint32_t *>(info + ri) : nullptr;
    const uint32_t r0 = ref32[0];
    if (((r0 >> 16) & 0xFFu) == 0u) {                                 // R.valid == 0: skipped, the info record all zero
        if (lane == 0) out[kSubHdr + 2] = 0u;
        if (info32 && lane < 16) info32[lane] = 0u;
        return;
    }
    const uint32_t c0 = rec32[10], c1 = rec32[11], a0 = rec32[12], a1 = rec32[13], a2 = rec32[14];
    const int T = 2 * (int)(int16_t)(c0 >> 16) + (int)((c1 >> 16) & 0xFFu);
    const int F = 2 * (int)(int16_t)(c1 & 0xFFFFu) + (int)(c1 >> 24);
    const float *pi = iq + (size_t)frame * 2 * kNSamples, *pq = pi + kNSamples;

    // the 79 tones, through LDS: the amplitude pass reads them per lane
    const uint32_t tone_lo = tone_of_symbol(a0, a1, a2, mtab, lane);
    L.tone[lane] = (int)tone_lo;
    if (lane < 80 - 64) L.tone[64 + lane] = lane < FT8GPU_NN - 64 ? (int)tone_of_symbol(a0, a1, a2, mtab, 64 + lane) : 0;

    // u*: the first largest of R.pf[1 .. 3]
    const float pf1 = __uint_as_float(ref32[5]), pf2 = __uint_as_float(ref32[6]), pf3 = __uint_as_float(ref32[7]);
    int us = 1;
    float pbest = pf1;
    if (pf2 > pbest) { us = 2; pbest = pf2; }
    if (pf3 > pbest) us = 3;
    const int S0 = 256 * T + FT8GPU_REFINE_LEAD + 32 * (int)(int16_t)(r0 & 0xFFFFu);
    const int k4_0 = 4 * (F + us - 2);
    wave_lds_sync();

    // ---- (c) the fine search: frequency, then time -----------------------------------------------------------------------------
    float pf_best, pt_best;
    const float Pf = search<false, kShape>(pi, pq, L, s_wr, s_wi, s_pulse, S0, k4_0, lane);
    const int di = first_max(L, Pf, lane, pf_best);
    const int k4 = k4_0 + di - FT8GPU_SUBTRACT_RANGE;
    const float Pt4 = search<true, kShape>(pi, pq, L, s_wr, s_wi, s_pulse, S0, k4, lane);
    const float Pt = lane == FT8GPU_SUBTRACT_RANGE ? pf_best : Pt4;   // pt[2] = P(S_0, k4*) = pf[d* + 2]
    const int ti = first_max(L, Pt, lane, pt_best);
    const int S = S0 + FT8GPU_SUBTRACT_TSTEP * (ti - FT8GPU_SUBTRACT_RANGE);

    // ---- (d) the amplitude: G(q) two symbols at a time, A(q) behind it by eight segments ---------------------------------------
    float2 *A = reinterpret_cast<float2 *>(out);
    for (int c = 0; c < (kSubSegs + 31) / 32; ++c) {
        stage_span<kAmpSpanSegs>(pi, pq, S + 1024 * c, L.plane[0], L.plane[1], lane);
        wave_lds_sync();
        const int m = 2 * c + (lane >> 4), seg = lane & 15;
        if (lane < 32 && m < FT8GPU_NN) {
            float re, im;
            if constexpr (kShape == FT8GPU_SUBTRACT_GFSK) {
                const uint32_t step = (uint32_t)k4 << 20;
                seg_sum_gfsk(L.plane[0], L.plane[1], s_wr, s_wi, s_pulse, kSeg * lane, step * (uint32_t)(512 * m + kSeg * seg), step,
                             pulse_tones(L.tone, m), seg, re, im);
            } else {
                const uint32_t K = (uint32_t)k4 + 8u * (uint32_t)L.tone[m];
                seg_sum(L.plane[0], L.plane[1], s_wr, s_wi, kSeg * lane, 512u * (uint32_t)m * (uint32_t)k4 + K * (uint32_t)(kSeg * seg), K, re, im);
            }
            L.ring[0][(32 * c + lane) & (kRing - 1)] = re;
            L.ring[1][(32 * c + lane) & (kRing - 1)] = im;
        }
        wave_lds_sync();
        const int q = 32 * c - kSmooth + lane;
        if (lane < 32 && q >= 0 && q < kSubSegs) {
            const int p_lo = q - kSmooth < 0 ? 0 : q - kSmooth;
            const int p_hi = q + kSmooth > kSubSegs - 1 ? kSubSegs - 1 : q + kSmooth;
            float ar = 0.0f, ai = 0.0f;
            for (int p = p_lo; p <= p_hi; ++p) {
                ar = ar + L.ring[0][p & (kRing - 1)];
                ai = ai + L.ring[1][p & (kRing - 1)];
            }
            const float w = tab->inv[p_hi - p_lo + 1];
            A[q] = make_float2(ar * w, ai * w);
        }
        wave_lds_sync();
    }

    // ---- what the apply kernel reads: S*, k4*, valid, the tones ---------------------------------------------------------------------
    if (lane == 0) out[kSubHdr] = (uint32_t)S;
    if (lane == 1) out[kSubHdr + 1] = (uint32_t)k4;
    if (lane == 2) out[kSubHdr + 2] = 1u;
    if (lane == 3) out[kSubHdr + 3] = 0u;
    if (lane < 20)
        out[kSubTones + lane] = (uint32_t)L.tone[4 * lane] | (uint32_t)L.tone[4 * lane + 1] << 8 | (uint32_t)L.tone[4 * lane + 2] << 16 |
                                (uint32_t)L.tone[4 * lane + 3] << 24;

    // ---- the info record: 16 dwords, one lane each --------------------------------------------------------------------------------
    if (info32) {
        if (lane < kHyp) {                                            // lanes 0..4 still hold the powers of both searches
            info32[3 + lane] = __float_as_uint(Pf);
            info32[8 + lane] = __float_as_uint(Pt);
        } else if (lane == 5) {
            info32[0] = (uint32_t)k4;
        } else if (lane == 6) {
            info32[1] = (uint32_t)S;
        } else if (lane == 7) {
            info32[2] = (uint32_t)(uint8_t)(int8_t)(di - FT8GPU_SUBTRACT_RANGE) | (uint32_t)(uint8_t)(int8_t)(ti - FT8GPU_SUBTRACT_RANGE) << 8 | 1u << 16;
        } else if (lane < 11) {
            info32[5 + lane] = 0u;                                    // 13, 14, 15: the zero padding
        }
    }
}

__global__ __launch_bounds__(256)
void ft8_subtract_estimate_kernel(const float *__restrict__ iq, const ft8gpu_message *__restrict__ msgs,
                                  const ft8gpu_refined *__restrict__ refined, const int32_t *__restrict__ first,
                                  const int32_t *__restrict__ n_msgs, int nframes, const SubTables *__restrict__ tab,
                                  const MsgTables *__restrict__ mtab, uint32_t *__restrict__ scratch, ft8gpu_subtract_info *info) {
    estimate_body<FT8GPU_SUBTRACT_CPFSK>(iq, msgs, refined, first, n_msgs, nframes, tab, nullptr, mtab, scratch, info);
}

__global__ __launch_bounds__(256)
void ft8_subtract_estimate_gfsk_kernel(const float *__restrict__ iq, const ft8gpu_message *__restrict__ msgs,
                                       const ft8gpu_refined *__restrict__ refined, const int32_t *__restrict__ first,
                                       const int32_t *__restrict__ n_msgs, int nframes, const SubTables *__restrict__ tab,
                                       const SubGfskTables *__restrict__ gtab, const MsgTables *__restrict__ mtab,
                                       uint32_t *__restrict__ scratch, ft8gpu_subtract_info *info) {
    estimate_body<FT8GPU_SUBTRACT_GFSK>(iq, msgs, refined, first, n_msgs, nframes, tab, gtab, mtab, scratch, info);
}

// ---- apply ------------------------------------------------------------------------------------------------------------------
struct ApplyHdr {
    int S[kMaxMessages];
    uint32_t k4[kMaxMessages];
    uint32_t tones[kMaxMessages][20];
};

__device__ __forceinline__ uint32_t hdr_tone(const uint32_t *tones, int m) { return (tones[m >> 2] >> (8 * (m & 3))) & 0xFFu; }

// the apply kernel of either shape; s_q (Q in table order) and s_ramp: the GFSK shape's, neither read nor allocated for CPFSK
template <int kShape>
__device__ __forceinline__ void apply_body(const float *iq, float *out, const int32_t *__restrict__ first, const int32_t *__restrict__ n_msgs,
                                           int nframes, const SubTables *__restrict__ tab, const SubGfskTables *__restrict__ gtab,
                                           const uint32_t *__restrict__ scratch) {
    __shared__ float2 s_w[kTab];                                      // 32 KB: one 8-byte read per sample and record
    __shared__ ApplyHdr s_hdr;
    __shared__ __attribute__((aligned(16))) uint32_t s_q[kShape == FT8GPU_SUBTRACT_GFSK ? kPulse + 3 : 4];
    __shared__ float s_ramp[kShape == FT8GPU_SUBTRACT_GFSK ? kRamp : 1];

    const int frame = (int)(blockIdx.x / (unsigned)kParts);
    const int part = (int)(blockIdx.x - (unsigned)frame * kParts);
    if (frame >= nframes) return;
    int lo = first[frame], hi = n_msgs[frame];
    lo = lo < 0 ? 0 : (lo > kMaxMessages ? kMaxMessages : lo);
    hi = hi < 0 ? 0 : (hi > kMaxMessages ? kMaxMessages : hi);
    const int cnt = hi > lo ? hi - lo : 0;                            // workgroup-uniform
    const size_t base = (size_t)frame * 2 * kNSamples + (size_t)part * kPartSamples;
    const float4 *src_i = reinterpret_cast<const float4 *>(iq + base), *src_q = reinterpret_cast<const float4 *>(iq + base + kNSamples);
    float4 *dst_i = reinterpret_cast<float4 *>(out + base), *dst_q = reinterpret_cast<float4 *>(out + base + kNSamples);
    if (cnt == 0) {
        if (out != iq)
            for (int v = threadIdx.x; v < kPartSamples / 4; v += 256) {
                dst_i[v] = src_i[v];
                dst_q[v] = src_q[v];
            }
        return;
    }

    for (int i = threadIdx.x; i < kTab; i += 256) {
        s_w[i] = tab->w4[i];
    }
    if constexpr (kShape == FT8GPU_SUBTRACT_GFSK) {
        for (int i = threadIdx.x; i < kPulse; i += 256) s_q[i] = gtab->q[i];
        if (threadIdx.x < kRamp) s_ramp[threadIdx.x] = gtab->ramp[threadIdx.x];
    }
    const uint32_t *fs = scratch + ((size_t)frame * kMaxMessages + lo) * kSubStride;
    for (int i = threadIdx.x; i < cnt * 22; i += 256) {
        const int r = i / 22, k = i - 22 * r;
        const uint32_t *h = fs + (size_t)r * kSubStride;
        if (k == 0) s_hdr.S[r] = h[kSubHdr + 2] != 0u ? (int)h[kSubHdr] : 0x40000000;     // a skipped record covers no sample
        else if (k == 1) s_hdr.k4[r] = h[kSubHdr + 1];
        else s_hdr.tones[r][k - 2] = h[kSubTones + k - 2];
    }
    __syncthreads();

    for (int v = threadIdx.x; v < kPartSamples / 4; v += 256) {
        const int j = part * kPartSamples + 4 * v;
        float4 a = src_i[v], b = src_q[v];
        for (int r = 0; r < cnt; ++r) {
            const int rel = j - s_hdr.S[r];
            if ((unsigned)rel >= (unsigned)kSpan) continue;           // S* is a multiple of 8: all four samples or none
            const int m = rel >> 9;
            const uint32_t k4 = s_hdr.k4[r];
            if constexpr (kShape == FT8GPU_SUBTRACT_GFSK) {
                // (b') the four phases from Q, one 16-byte word per pulse term; (e') the ramp over a record's first and last 64 samples
                const int k = rel & 511;
                const uint32_t *tones = s_hdr.tones[r];
                const uint32_t e0 = hdr_tone(tones, m > 0 ? m - 1 : 0), e1 = hdr_tone(tones, m);
                const uint32_t e2 = hdr_tone(tones, m < FT8GPU_NN - 1 ? m + 1 : FT8GPU_NN - 1);
                const uint4 qa = *reinterpret_cast<const uint4 *>(s_q + k + 1024), qb = *reinterpret_cast<const uint4 *>(s_q + k + 512);
                const uint4 qc = *reinterpret_cast<const uint4 *>(s_q + k);
                const uint32_t step = k4 << 20, lin = step * (uint32_t)rel;
                const uint32_t i0 = (lin + e0 * qa.x + e1 * qb.x + e2 * qc.x + kHalfStep) >> 20;
                const uint32_t i1 = (lin + step + e0 * qa.y + e1 * qb.y + e2 * qc.y + kHalfStep) >> 20;
                const uint32_t i2 = (lin + 2u * step + e0 * qa.z + e1 * qb.z + e2 * qc.z + kHalfStep) >> 20;
                const uint32_t i3 = (lin + 3u * step + e0 * qa.w + e1 * qb.w + e2 * qc.w + kHalfStep) >> 20;
                const float2 A = reinterpret_cast<const float2 *>(fs + (size_t)r * kSubStride)[rel >> 5];
                float2 A0 = A, A1 = A, A2 = A, A3 = A;
                if (rel < kRamp || rel >= kSpan - kRamp) {
                    const bool head = rel < kRamp;
                    const float v0 = s_ramp[head ? rel : kSpan - 1 - rel], v1 = s_ramp[head ? rel + 1 : kSpan - 2 - rel];
                    const float v2 = s_ramp[head ? rel + 2 : kSpan - 3 - rel], v3 = s_ramp[head ? rel + 3 : kSpan - 4 - rel];
                    A0 = make_float2(A.x * v0, A.y * v0);
                    A1 = make_float2(A.x * v1, A.y * v1);
                    A2 = make_float2(A.x * v2, A.y * v2);
                    A3 = make_float2(A.x * v3, A.y * v3);
                }
                float2 w;
                w = s_w[i0];
                a.x = a.x - (A0.x * w.x + A0.y * w.y);
                b.x = b.x - (A0.y * w.x - A0.x * w.y);
                w = s_w[i1];
                a.y = a.y - (A1.x * w.x + A1.y * w.y);
                b.y = b.y - (A1.y * w.x - A1.x * w.y);
                w = s_w[i2];
                a.z = a.z - (A2.x * w.x + A2.y * w.y);
                b.z = b.z - (A2.y * w.x - A2.x * w.y);
                w = s_w[i3];
                a.w = a.w - (A3.x * w.x + A3.y * w.y);
                b.w = b.w - (A3.y * w.x - A3.x * w.y);
                continue;
            }
            const uint32_t tone = (s_hdr.tones[r][m >> 2] >> (8 * (m & 3))) & 0xFFu;
            const uint32_t K = k4 + 8u * tone;
            uint32_t idx = (512u * (uint32_t)m * k4 + K * (uint32_t)(rel & 511)) & kTabMask;
            const float2 A = reinterpret_cast<const float2 *>(fs + (size_t)r * kSubStride)[rel >> 5];
            float2 w;
            w = s_w[idx]; idx = (idx + K) & kTabMask;
            a.x = a.x - (A.x * w.x + A.y * w.y);
            b.x = b.x - (A.y * w.x - A.x * w.y);
            w = s_w[idx]; idx = (idx + K) & kTabMask;
            a.y = a.y - (A.x * w.x + A.y * w.y);
            b.y = b.y - (A.y * w.x - A.x * w.y);
            w = s_w[idx]; idx = (idx + K) & kTabMask;
            a.z = a.z - (A.x * w.x + A.y * w.y);
            b.z = b.z - (A.y * w.x - A.x * w.y);
            w = s_w[idx];
            a.w = a.w - (A.x * w.x + A.y * w.y);
            b.w = b.w - (A.y * w.x - A.x * w.y);
        }
        dst_i[v] = a;
        dst_q[v] = b;
    }
}

__global__ __launch_bounds__(256)
void ft8_subtract_apply_kernel(const float *iq, float *out, const int32_t *__restrict__ first, const int32_t *__restrict__ n_msgs,
                               int nframes, const SubTables *__restrict__ tab, const uint32_t *__restrict__ scratch) {
    apply_body<FT8GPU_SUBTRACT_CPFSK>(iq, out, first, n_msgs, nframes, tab, nullptr, scratch);
}

__global__ __launch_bounds__(256)
void ft8_subtract_apply_gfsk_kernel(const float *iq, float *out, const int32_t *__restrict__ first, const int32_t *__restrict__ n_msgs,
                                    int nframes, const SubTables *__restrict__ tab, const SubGfskTables *__restrict__ gtab,
                                    const uint32_t *__restrict__ scratch) {
    apply_body<FT8GPU_SUBTRACT_GFSK>(iq, out, first, n_msgs, nframes, tab, gtab, scratch);
}

// ---- the pass loop's bookkeeping ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void ft8_subtract_active_kernel(const int32_t *__restrict__ prev, const int32_t *__restrict__ n_msgs, int nframes,
                                int32_t *__restrict__ n_ref, int32_t *__restrict__ n_active) {
    __shared__ int s_count;
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int f = threadIdx.x; f < nframes; f += 256) {
        const int n = n_msgs[f];
        const bool active = prev[f] < n && n < kMaxMessages;
        n_ref[f] = active ? n : 0;
        mine += active ? 1 : 0;
    }
    if (mine) atomicAdd(&s_count, mine);                              // an integer count: the order does not matter
    __syncthreads();
    if (threadIdx.x == 0) *n_active = s_count;
}

__global__ __launch_bounds__(256)
void ft8_subtract_gate_kernel(const int32_t *__restrict__ n_ref, int nframes, int32_t *__restrict__ counts) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < nframes && n_ref[f] == 0) counts[f] = 0;
}

}  // namespace

hipError_t launch_subtract_estimate(const float *iq, const ft8gpu_message *msgs, const ft8gpu_refined *refined, const int32_t *first,
                                    const int32_t *n_msgs, int nframes, int shape, const SubTables *tab, const SubGfskTables *gtab,
                                    const MsgTables *mtab, uint32_t *scratch, ft8gpu_subtract_info *info, hipStream_t s) {
    if (shape != FT8GPU_SUBTRACT_CPFSK && (shape != FT8GPU_SUBTRACT_GFSK || !gtab)) return hipErrorInvalidValue;
    if (nframes <= 0) return hipSuccess;
    const dim3 grid((unsigned)nframes * kBlocksPerFrame);
    if (shape == FT8GPU_SUBTRACT_GFSK)
        ft8_subtract_estimate_gfsk_kernel<<<grid, dim3(256), 0, s>>>(iq, msgs, refined, first, n_msgs, nframes, tab, gtab, mtab, scratch, info);
    else
        ft8_subtract_estimate_kernel<<<grid, dim3(256), 0, s>>>(iq, msgs, refined, first, n_msgs, nframes, tab, mtab, scratch, info);
    return hipGetLastError();
}

hipError_t launch_subtract_apply(const float *iq, float *out, const int32_t *first, const int32_t *n_msgs, int nframes, int shape,
                                 const SubTables *tab, const SubGfskTables *gtab, const uint32_t *scratch, hipStream_t s) {
    if (shape != FT8GPU_SUBTRACT_CPFSK && (shape != FT8GPU_SUBTRACT_GFSK || !gtab)) return hipErrorInvalidValue;
    if (nframes <= 0) return hipSuccess;
    const dim3 grid((unsigned)nframes * kParts);
    if (shape == FT8GPU_SUBTRACT_GFSK)
        ft8_subtract_apply_gfsk_kernel<<<grid, dim3(256), 0, s>>>(iq, out, first, n_msgs, nframes, tab, gtab, scratch);
    else
        ft8_subtract_apply_kernel<<<grid, dim3(256), 0, s>>>(iq, out, first, n_msgs, nframes, tab, scratch);
    return hipGetLastError();
}

hipError_t launch_subtract_active(const int32_t *prev, const int32_t *n_msgs, int nframes, int32_t *n_ref, int32_t *n_active,
                                  hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    ft8_subtract_active_kernel<<<dim3(1), dim3(256), 0, s>>>(prev, n_msgs, nframes, n_ref, n_active);
    return hipGetLastError();
}

hipError_t launch_subtract_gate(const int32_t *n_ref, int nframes, int32_t *counts, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    ft8_subtract_gate_kernel<<<dim3((unsigned)(nframes + 255) / 256), dim3(256), 0, s>>>(n_ref, nframes, counts);
    return hipGetLastError();
}
