// refine.hip -- refined time and frequency: every message record correlated with the frame's I/Q samples (the rule is in
// include/ft8gpu.h "refined time and frequency", restated in tests/ft8_spec_refine.py; DESIGN.md "Refined time and frequency").
//
//   ft8_refine_kernel   one wave per record, four per workgroup (the geometry of match.hip and combine.hip).
//     stage 1, per symbol: the 1536 samples that cover the 33 offsets go through LDS (float4 loads, 64 lanes side by side);
//       lanes 0..47 each dechirp one segment of 32 samples, sequentially in j; lanes 0..32 each add the 16 segment sums of
//       their own offset, sequentially in q, and keep P(0, e) as a running sum over the symbols.
//     e_best: every lane scans the 33 powers (LDS broadcast), so the result is wave-uniform without a reduction tree.
//     stage 2, per symbol: the 512 samples at e_best; lanes (u, segment) dechirp the four neighbours u = -2, -1, 1, 2 at once,
//       lanes 0..15 the empty tone; lanes 0..4 add their 16 segment sums and keep the running sums.
//   Every sum of the rule is formed by one lane in the stated order; no value crosses lanes except through LDS.
//
// LDS (61 440 bytes per workgroup, two workgroups per CU):
//   twiddles, shared: two planes of 1024 floats, entry i at ((i & 31) << 5) | (i >> 5).  The lanes of a dechirp step read
//     w[(A + 32 k l) & 1023] for one A: transposed, lane l's bank is ((A >> 5) + k l) & 31 -- all different for odd k, and lanes
//     that share a bank for even k read the same entry (broadcast).
//   samples, per wave: I and Q planes, segment s at 33 s (one float of padding): lane l reads 33 l + i, bank (l + i) & 31,
//     conflict-free; the float4 of lane v lands at 4 v + (v >> 3), banks 4 (v & 7) + (v >> 3) + c, conflict-free.
//   segment sums, per wave: two planes of 80 floats.
// No scratch.  Indices: (k * j) mod 1024 is formed in uint32, which is exact for every int32 k and j.
#include "refine.h"
#include "span_dev.h"
#include "tone_dev.h"
#include "wave_dev.h"
#include <stddef.h>

namespace {

constexpr int kSeg = FT8GPU_REFINE_STEP;                       // samples per segment
constexpr int kSymSegs = 512 / kSeg;                           // 16 segments per symbol
constexpr int kRange = FT8GPU_REFINE_RANGE;
constexpr int kOffsets = 2 * kRange + 1;                       // 33
constexpr int kSpanSegs = kSymSegs + 2 * kRange;               // 48 segments cover every offset of a symbol
constexpr int kSegPitch = kStagePitch;                         // stage_span's layout (span_dev.h)
constexpr int kPlane = kSpanSegs * kSegPitch;                  // 1584 floats
constexpr int kSums = 80;                                      // 4 neighbours x 16 segments + 16 of the empty tone
constexpr int kWaves = 4;
constexpr int kBlocksPerFrame = (kMaxMessages + kWaves - 1) / kWaves;
static_assert(kSeg == kStageSeg && kSpanSegs <= 64 && kOffsets <= 64 && kSpanSegs <= kSums, "lane assignment");
static_assert(sizeof(ft8gpu_message) == 64 && sizeof(ft8gpu_refined) == 48, "record sizes");

// g(k, q) of the segment staged at `seg`, whose first sample is j: sequential in j from +0
__device__ __forceinline__ void seg_sum(const float *s_i, const float *s_q, const float *s_twr, const float *s_twi, int seg, int k, int j,
                                        float &re, float &im) {
    const float *xi_ = s_i + seg * kSegPitch, *xq_ = s_q + seg * kSegPitch;
    uint32_t idx = ((uint32_t)k * (uint32_t)j) & 1023u;
    float ar = 0.0f, ai = 0.0f;
#pragma unroll 8
    for (int i = 0; i < kSeg; ++i) {
        const float xr = xi_[i], xi = xq_[i];
        const uint32_t p = (idx & 31u) << 5 | idx >> 5;
        const float wr = s_twr[p], wi = s_twi[p];
        ar = ar + (xr * wr - xi * wi);
        ai = ai + (xr * wi + xi * wr);
        idx = (idx + (uint32_t)k) & 1023u;
    }
    re = ar;
    im = ai;
}

__global__ __launch_bounds__(256)
void ft8_refine_kernel(const float *__restrict__ iq, const ft8gpu_message *__restrict__ msgs, const int32_t *__restrict__ n_msgs,
                       int nframes, const Ft8Tables *__restrict__ tab, const MsgTables *__restrict__ mtab, ft8gpu_refined *refined) {
    __shared__ float s_twr[kNfft], s_twi[kNfft];
    __shared__ __attribute__((aligned(16))) float s_plane[kWaves][2][kPlane];
    __shared__ float s_sum[kWaves][2][kSums];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int frame = (int)(blockIdx.x / (unsigned)kBlocksPerFrame);
    const int first = (int)(blockIdx.x - (unsigned)frame * kBlocksPerFrame) * kWaves;
    if (frame >= nframes) return;
    int n = n_msgs[frame];
    n = n < 0 ? 0 : (n > kMaxMessages ? kMaxMessages : n);
    if (first >= n) return;                                           // workgroup-uniform: nothing of this block is touched

    for (int i = threadIdx.x; i < kNfft; i += 256) {
        const float2 w = tab->tw[i];
        const int p = (i & 31) << 5 | i >> 5;
        s_twr[p] = w.x;
        s_twi[p] = w.y;
    }
    __syncthreads();
    const int mi = first + wave;
    if (mi >= n) return;                                              // wave-uniform: records behind the count are not touched

    const ft8gpu_message *rec = msgs + (size_t)frame * kMaxMessages + mi;
    const uint32_t *rec32 = reinterpret_cast<const uint32_t *>(rec);
    const uint32_t c0 = rec32[10], c1 = rec32[11], a0 = rec32[12], a1 = rec32[13], a2 = rec32[14];
    const int T = 2 * (int)(int16_t)(c0 >> 16) + (int)((c1 >> 16) & 0xFFu);
    const int F = 2 * (int)(int16_t)(c1 & 0xFFFFu) + (int)(c1 >> 24);
    const float *pi = iq + (size_t)frame * 2 * kNSamples, *pq = pi + kNSamples;
    float *s_i = s_plane[wave][0], *s_q = s_plane[wave][1];
    float *s_re = s_sum[wave][0], *s_im = s_sum[wave][1];

    // the 79 tones: lane m holds tone[m] and tone[64 + m]; the symbol loops fetch them with v_readlane
    const uint32_t tone_lo = tone_of_symbol(a0, a1, a2, mtab, lane);
    const uint32_t tone_hi = lane < FT8GPU_NN - 64 ? tone_of_symbol(a0, a1, a2, mtab, 64 + lane) : 0u;

    // ---- stage 1: P(0, e) for the 33 offsets ------------------------------------------------------------------------
    const int base0 = 256 * T + FT8GPU_REFINE_LEAD;                   // s_0(0)
    float P = 0.0f;
    for (int m = 0; m < FT8GPU_NN; ++m) {
        const int tone = m < 64 ? __builtin_amdgcn_readlane((int)tone_lo, m & 63) : __builtin_amdgcn_readlane((int)tone_hi, m & 63);
        const int k = F + 2 * tone;
        const int j0 = base0 + 512 * m - kSeg * kRange;               // s_m(-16)
        stage_span<kSpanSegs>(pi, pq, j0, s_i, s_q, lane);
        wave_lds_sync();
        if (lane < kSpanSegs) {
            float re, im;
            seg_sum(s_i, s_q, s_twr, s_twi, lane, k, j0 + kSeg * lane, re, im);
            s_re[lane] = re;
            s_im[lane] = im;
        }
        wave_lds_sync();
        if (lane < kOffsets) {
            float cr = 0.0f, ci = 0.0f;
#pragma unroll
            for (int t = 0; t < kSymSegs; ++t) {
                cr = cr + s_re[lane + t];
                ci = ci + s_im[lane + t];
            }
            P = P + (cr * cr + ci * ci);
        }
        wave_lds_sync();
    }

    // ---- e_best: the first strictly greatest, scanned by every lane alike ----------------------------------------------
    if (lane < kOffsets) s_re[lane] = P;
    wave_lds_sync();
    float best = s_re[0];
    int eb = 0;
    for (int e = 1; e < kOffsets; ++e) {
        const float v = s_re[e];
        if (v > best) {
            best = v;
            eb = e;
        }
    }
    eb = __builtin_amdgcn_readfirstlane(eb);
    const float pt0 = eb >= 1 ? s_re[eb - 1] : 0.0f;
    const float pt2 = eb + 1 < kOffsets ? s_re[eb + 1] : 0.0f;
    wave_lds_sync();

    // ---- stage 2: the four neighbours and the empty tone at e_best ----------------------------------------------------
    const int grp = lane >> 4, seg = lane & 15;
    const int u = grp < 2 ? grp - 2 : grp - 1;                         // -2, -1, 1, 2
    float Q = 0.0f;
    for (int m = 0; m < FT8GPU_NN; ++m) {
        const int tone = m < 64 ? __builtin_amdgcn_readlane((int)tone_lo, m & 63) : __builtin_amdgcn_readlane((int)tone_hi, m & 63);
        const int j1 = base0 + 512 * m + kSeg * (eb - kRange);        // s_m(e_best)
        stage_span<kSymSegs>(pi, pq, j1, s_i, s_q, lane);
        wave_lds_sync();
        {
            float re, im;
            seg_sum(s_i, s_q, s_twr, s_twi, seg, F + 2 * tone + u, j1 + kSeg * seg, re, im);
            s_re[lane] = re;
            s_im[lane] = im;
        }
        if (lane < kSymSegs) {
            float re, im;
            seg_sum(s_i, s_q, s_twr, s_twi, seg, F + 2 * ((tone + 4) & 7), j1 + kSeg * seg, re, im);
            s_re[64 + lane] = re;
            s_im[64 + lane] = im;
        }
        wave_lds_sync();
        if (lane < 5) {
            float cr = 0.0f, ci = 0.0f;
#pragma unroll
            for (int t = 0; t < kSymSegs; ++t) {
                cr = cr + s_re[kSymSegs * lane + t];
                ci = ci + s_im[kSymSegs * lane + t];
            }
            Q = Q + (cr * cr + ci * ci);
        }
        wave_lds_sync();
    }

    // ---- the record: 12 dwords, one lane each ---------------------------------------------------------------------------
    uint32_t *out32 = reinterpret_cast<uint32_t *>(refined + (size_t)frame * kMaxMessages + mi);
    int slot;
    uint32_t val;
    if (lane < 5) {                                                   // pf[0], pf[1], pf[3], pf[4], noise
        slot = lane < 2 ? 4 + lane : (lane < 4 ? 5 + lane : 9);
        val = __float_as_uint(Q);
    } else if (lane == 5) {
        slot = 0;
        val = (uint32_t)(uint16_t)(int16_t)(eb - kRange) | 1u << 16;
    } else if (lane == 6) {
        slot = 1;
        val = __float_as_uint(pt0);
    } else if (lane == 7) {
        slot = 2;
        val = __float_as_uint(best);
    } else if (lane == 8) {
        slot = 3;
        val = __float_as_uint(pt2);
    } else if (lane == 9) {
        slot = 6;                                                     // pf[2] is P(0, e_best)
        val = __float_as_uint(best);
    } else {
        slot = lane;                                                  // 10, 11: the zero padding
        val = 0u;
    }
    if (lane < 12) out32[slot] = val;
}

}  // namespace

hipError_t launch_refine(const float *iq, const ft8gpu_message *msgs, const int32_t *n_msgs, int nframes, const Ft8Tables *tab,
                         const MsgTables *mtab, ft8gpu_refined *refined, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    ft8_refine_kernel<<<dim3((unsigned)nframes * kBlocksPerFrame), dim3(256), 0, s>>>(iq, msgs, n_msgs, nframes, tab, mtab, refined);
    return hipGetLastError();
}
