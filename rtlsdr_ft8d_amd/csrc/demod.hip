// demod.hip -- undecoded candidates demodulated again from the I/Q samples (the rule is in include/ft8gpu.h "demodulation from
// the I/Q samples", restated in tests/ft8_spec_demod.py; DESIGN.md "Demodulation from the I/Q samples").  Not part of the
// reference's path: a fine Costas sync, a matched 512-sample correlation per tone, and max-log soft bits over blocks of one, two
// and three symbols, each set tried with bp_decode.
//
//   ft8_demod_select_kernel   one wave per frame: which candidates are attempted (ok == 0, ldpc_errors != 0, fewer than
//                             max_per_frame such candidates in front), as a 0 / 1 mark in dword 0 of the info record.  A launch
//                             of its own because status_out may be status_in: the main kernel's waves overwrite records other
//                             waves would count.
//   ft8_demod_kernel          one wave per candidate, four per workgroup, the launch geometry of the LDPC kernel.  A wave whose
//                             candidate is not marked copies the record and leaves (cand_dev.h's head of the kernel, with
//                             the mark); no workgroup-wide step exists, so a workgroup without a marked candidate never
//                             touches LDS.
//     symbol correlation: lane l loads the samples l + 64 a, a < 8, of a symbol straight from global memory (64 consecutive
//       floats per load), multiplies each by its base-frequency entry of w4 (read through the cache: the 64 indices of a load
//       are k4 apart, no LDS layout serves every k4), forms the 8-point DFT over a in registers and applies its eight twiddles
//       w4[8 t l], which it holds for the whole candidate.  The 64 lanes' values are added by the rule's xor butterfly: four DPP
//       steps (after the quad steps a quad is uniform, so row_half_mirror and row_mirror deliver the xor-4 and xor-8 partners'
//       values) and two ds_bpermute steps.
//     fine sync: 13 hypotheses x 21 Costas symbols, one tone each (only that tone's two floats are reduced).
//     spectra: 79 symbols, eight tones each, into the wave's LDS as two planes with a row pitch of 9 floats.
//     soft bits: set 1 on lanes 0..57, one data symbol each (rows 9 apart: conflict-free but for the three lanes of the second
//       half that share a bank with the first within 32 lanes); sets 2 and 3 with lanes as tone tuples (b1, b2) and, for a
//       triple, a loop over b3 -- the Z reads are eight distinct addresses in eight distinct banks, the rest broadcast.  The
//       maxima are taken on the bit patterns (the magnitudes are non-negative), so their order does not matter.
//     normalisation in index order by every lane alike with the guard ahead of iteration 0, bp_decode, the judgement with the
//       CRC and the record: cand_dev.h's code, as for combine.hip.
//   ft8_demod_soft_kernel     the same body (demod_body, a template on "emits") that also writes x, the normalised soft bits
//                             bp_decode ran on, of every set it reached into soft [frame][candidate][3][176], and zero rows
//                             for everything else below the count: what apsoft.hip (AP on these soft bits) reads.
//   launch_demod_tag          pad[3] of the records the append step added = the accepted set (cand_dev.h's tag kernel).
//
// LDS: 9 152 bytes per wave (the BP tile and the soft bits of cand_dev.h, 3 456, and Z, 5 696), 36 608 per workgroup.  No
// scratch.  Indices: (k4 * n) mod 4096 is formed in uint32, which is exact for every int32 k4.
#include "demod.h"
#include "cand_dev.h"

namespace {

__device__ LdpcTables d_ldpc;

constexpr int kTab = FT8GPU_SUBTRACT_TABLE;
constexpr uint32_t kTabMask = kTab - 1;
constexpr int kZPitch = 9;                                      // floats per symbol row of a Z plane
constexpr int kZPlane = 712;                                    // 79 rows of 9
constexpr int kDemodLds = kWaveLds + 2 * kZPlane;
constexpr int kHyp = 2 * FT8GPU_DEMOD_TRANGE + 1 + 2 * FT8GPU_DEMOD_FRANGE;    // 9 time offsets, then d = -2, -1, 1, 2
static_assert(FT8GPU_NN * kZPitch <= kZPlane && kTab == 4096 && kHyp == 13, "layout");
static_assert(sizeof(ft8gpu_demod_info) == 16 && sizeof(ft8gpu_message) == 64, "record sizes");

__constant__ uint8_t c_costas[7] = { 3, 1, 4, 0, 6, 5, 2 };
// the Gray map {0,1,3,2,5,6,4,7} of a bit pattern, one nibble each (a per-lane index into a table would be a memory read)
__device__ __forceinline__ int gray_of(int b) { return (int)((0x74652310u >> (4 * b)) & 7u); }

// one level of the butterfly with a DPP control
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// the rule's xor butterfly, levels 1, 2, 4, 8, 16, 32; every lane ends with the same sum
__device__ __forceinline__ float wave_bfly_add(float v) {
    v = dpp_add<0xB1>(v);                                       // quad_perm [1,0,3,2]: xor 1
    v = dpp_add<0x4E>(v);                                       // quad_perm [2,3,0,1]: xor 2
    v = dpp_add<0x141>(v);                                      // row_half_mirror: the other quad of eight (uniform)
    v = dpp_add<0x140>(v);                                      // row_mirror: the other eight of a row (uniform)
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 32);
    return v;
}

// the 4-point DFT of the rule
__device__ __forceinline__ void dft4(float v0r, float v0i, float v1r, float v1i, float v2r, float v2i, float v3r, float v3i,
                                     float (&outr)[4], float (&outi)[4]) {
    const float e0r = v0r + v2r, e0i = v0i + v2i, e1r = v0r - v2r, e1i = v0i - v2i;
    const float o0r = v1r + v3r, o0i = v1i + v3i, o1r = v1r - v3r, o1i = v1i - v3i;
    outr[0] = e0r + o0r; outi[0] = e0i + o0i;
    outr[1] = e1r + o1i; outi[1] = e1i - o1r;
    outr[2] = e0r - o0r; outi[2] = e0i - o0i;
    outr[3] = e1r - o1i; outi[3] = e1i + o1r;
}

// V_t of lane `lane` for the symbol whose first sample is s0 and whose first phase count is n0 = 512 m
__device__ __forceinline__ void symbol_dft(const float *__restrict__ pi, const float *__restrict__ pq, const float2 *__restrict__ w4,
                                           int s0, uint32_t n0, uint32_t k4, int lane, const float (&twr)[8], const float (&twi)[8],
                                           float (&vr)[8], float (&vi)[8]) {
    float yr[8], yi[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int j = s0 + lane + 64 * a;
        float xr = 0.0f, xi = 0.0f;
        if ((unsigned)j < (unsigned)kNSamples) {                      // samples outside the frame are zero, not read
            xr = pi[j];
            xi = pq[j];
        }
        const float2 w = w4[(k4 * (n0 + (uint32_t)(lane + 64 * a))) & kTabMask];
        yr[a] = xr * w.x - xi * w.y;
        yi[a] = xr * w.y + xi * w.x;
    }
    const float c8 = 0x1.6a09e6p-1f;                                  // the float of cos(pi / 4)
    float pr[4], pim[4], qr[4], qi[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        pr[a] = yr[a] + yr[a + 4]; pim[a] = yi[a] + yi[a + 4];
        qr[a] = yr[a] - yr[a + 4]; qi[a] = yi[a] - yi[a + 4];
    }
    const float q1r = (qr[1] + qi[1]) * c8, q1i = (qi[1] - qr[1]) * c8;
    const float q2r = qi[2], q2i = -qr[2];
    const float q3r = (qi[3] - qr[3]) * c8, q3i = -((qr[3] + qi[3]) * c8);
    float er[4], ei[4], dr[4], di[4];
    dft4(pr[0], pim[0], pr[1], pim[1], pr[2], pim[2], pr[3], pim[3], er, ei);
    dft4(qr[0], qi[0], q1r, q1i, q2r, q2i, q3r, q3i, dr, di);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        vr[2 * s] = er[s] * twr[2 * s] - ei[s] * twi[2 * s];
        vi[2 * s] = er[s] * twi[2 * s] + ei[s] * twr[2 * s];
        vr[2 * s + 1] = dr[s] * twr[2 * s + 1] - di[s] * twi[2 * s + 1];
        vi[2 * s + 1] = dr[s] * twi[2 * s + 1] + di[s] * twr[2 * s + 1];
    }
}

__device__ __forceinline__ uint32_t mag_bits(float re, float im) { return __float_as_uint(__builtin_sqrtf(re * re + im * im)); }
__device__ __forceinline__ bool not_finite(uint32_t bits) { return (bits & 0x7F800000u) == 0x7F800000u; }

// the soft bits of one block of B symbols from m0 into llr[bit0 ..]; lanes are the tuples (b1, b2) of bit patterns, a third
// symbol is walked per lane.  Returns whether a magnitude of this lane is not finite.
template <int B>
__device__ __forceinline__ bool block_bits(const float *zr, const float *zi, int m0, float *llr, int bit0, int lane) {
    const int b1 = B == 1 ? (lane & 7) : (lane >> 3), b2 = lane & 7;
    const bool active = B != 1 || lane < 8;
    float re = zr[kZPitch * m0 + gray_of(b1)], im = zi[kZPitch * m0 + gray_of(b1)];
    if (B >= 2) {
        re = re + zr[kZPitch * (m0 + 1) + gray_of(b2)];
        im = im + zi[kZPitch * (m0 + 1) + gray_of(b2)];
    }
    bool bad = false;
    uint32_t all = 0u, set3[3] = { 0u, 0u, 0u }, clr3[3] = { 0u, 0u, 0u };
    if (B == 3) {
#pragma unroll
        for (int b3 = 0; b3 < 8; ++b3) {
            const float r3 = re + zr[kZPitch * (m0 + 2) + gray_of(b3)], i3 = im + zi[kZPitch * (m0 + 2) + gray_of(b3)];
            const uint32_t a = mag_bits(r3, i3);
            bad = bad || not_finite(a);
            all = max(all, a);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if ((b3 >> (2 - k)) & 1) set3[k] = max(set3[k], a);
                else clr3[k] = max(clr3[k], a);
            }
        }
    } else {
        all = mag_bits(re, im);
        bad = active && not_finite(all);
        all = active ? all : 0u;
    }
    constexpr int kLaneBits = B == 1 ? 3 : 6;
#pragma unroll
    for (int k = 0; k < kLaneBits; ++k) {
        const bool bit = (lane >> (kLaneBits - 1 - k)) & 1;
        const uint32_t s = wave_max(bit ? all : 0u), c = wave_max(bit ? 0u : all);
        if (lane == 0) llr[bit0 + k] = __uint_as_float(s) - __uint_as_float(c);
    }
    if (B == 3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t s = wave_max(set3[k]), c = wave_max(clr3[k]);
            if (lane == 0) llr[bit0 + 6 + k] = __uint_as_float(s) - __uint_as_float(c);
        }
    }
    return bad;
}

// set n of the soft bits into llr[0 .. 173]; returns whether every magnitude was finite (wave-uniform)
__device__ __forceinline__ bool set_bits(int n, const float *zr, const float *zi, float *llr, int lane) {
    bool bad = false;
    if (n == 1) {
        if (lane < 58) {
            const int m = lane + (lane < 29 ? 7 : 14);
            uint32_t a[8];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                a[b] = mag_bits(zr[kZPitch * m + gray_of(b)], zi[kZPitch * m + gray_of(b)]);
                bad = bad || not_finite(a[b]);
            }
            const float hi0 = __uint_as_float(max(max(a[4], a[5]), max(a[6], a[7]))), lo0 = __uint_as_float(max(max(a[0], a[1]), max(a[2], a[3])));
            const float hi1 = __uint_as_float(max(max(a[2], a[3]), max(a[6], a[7]))), lo1 = __uint_as_float(max(max(a[0], a[1]), max(a[4], a[5])));
            const float hi2 = __uint_as_float(max(max(a[1], a[3]), max(a[5], a[7]))), lo2 = __uint_as_float(max(max(a[0], a[2]), max(a[4], a[6])));
            llr[3 * lane + 0] = hi0 - lo0;
            llr[3 * lane + 1] = hi1 - lo1;
            llr[3 * lane + 2] = hi2 - lo2;
        }
    } else {
        for (int half = 0; half < 2; ++half) {                        // wave-uniform loops
            const int first = half == 0 ? 7 : 43, bit_half = 87 * half;
            if (n == 2) {
                for (int i = 0; i < 28; i += 2) bad = block_bits<2>(zr, zi, first + i, llr, bit_half + 3 * i, lane) || bad;
                bad = block_bits<1>(zr, zi, first + 28, llr, bit_half + 84, lane) || bad;
            } else {
                for (int i = 0; i < 27; i += 3) bad = block_bits<3>(zr, zi, first + i, llr, bit_half + 3 * i, lane) || bad;
                bad = block_bits<2>(zr, zi, first + 27, llr, bit_half + 81, lane) || bad;
            }
        }
    }
    return !__any(bad);
}

__global__ __launch_bounds__(64)
void ft8_demod_select_kernel(const int32_t *__restrict__ counts, const ft8gpu_decode_status *__restrict__ status_in,
                             ft8gpu_demod_info *info, int max_candidates, int max_per_frame) {
    const int lane = threadIdx.x, frame = blockIdx.x;
    int count = counts[frame];
    count = count < 0 ? 0 : (count > max_candidates ? max_candidates : count);
    int base = 0;
    for (int c0 = 0; c0 < count; c0 += 64) {                          // wave-uniform
        const int ci = c0 + lane;
        bool q = false;
        const size_t rec_index = (size_t)frame * max_candidates + ci;
        if (ci < count) {
            const uint32_t *in32 = reinterpret_cast<const uint32_t *>(status_in + rec_index);
            q = still_failing(in32[0], in32[2]);
        }
        const uint64_t qs = __ballot(q);
        const int rank = base + __popcll(qs & ((1ull << lane) - 1ull));
        if (ci < count) reinterpret_cast<uint32_t *>(info + rec_index)[0] = (q && rank < max_per_frame) ? 1u : 0u;
        base += __popcll(qs);
    }
}

// Row n - 1 of a candidate's soft[3][FT8GPU_SOFT_STRIDE]: lane l stores the values l + 64 r it owns (elements 174 and 175 are
// +0 in cw[2] already), or 176 times +0.
constexpr int kSoftStride = FT8GPU_SOFT_STRIDE;
static_assert(kSoftStride == 176 && kSoftStride >= kLdpcN && kSoftStride % 4 == 0, "soft rows");
__device__ __forceinline__ void emit_row(float *rows, int n, const float (&cw)[3], int lane) {
    float *row = rows + (n - 1) * kSoftStride;
    row[lane] = cw[0];
    row[lane + 64] = cw[1];
    if (lane + 128 < kSoftStride) row[lane + 128] = cw[2];
}
__device__ __forceinline__ void zero_row(float *rows, int n, int lane) {
    if (lane < kSoftStride / 4) reinterpret_cast<float4 *>(rows + (n - 1) * kSoftStride)[lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// The body of both kernels, written once.  kEmit: the normalised soft bits of every set BP ran on go to soft (the rule is in
// include/ft8gpu.h at ft8gpu_demod_soft); nothing else differs, and without it soft is not touched.
template <bool kEmit>
__device__ __forceinline__ void demod_body(float (*s_mem)[kDemodLds], const float *__restrict__ iq,
                                           const ft8gpu_candidate *__restrict__ cands, const int32_t *__restrict__ counts,
                                           const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out,
                                           ft8gpu_demod_info *info, float *soft, int nframes, int max_candidates,
                                           const SubTables *__restrict__ tab, int sets, int max_hard_errors, int max_iters,
                                           int force_ieee_div, unsigned blocks_per_frame) {
    // not marked by the select kernel: not attempted, the record copied, the four dwords of the info record zero
    const CandWave w = cand_prologue(blockIdx.x, blocks_per_frame, 0u, counts, status_in, status_out, info, nframes, max_candidates, true);
    if (kEmit && w.verdict == kCandLeft) {                            // its three rows are zero (a gone wave writes nothing)
        float *rows = soft + w.rec_index * (3 * kSoftStride);
        for (int n = 1; n <= 3; ++n) zero_row(rows, n, w.lane);
    }
    if (w.verdict != kCandRun) return;
    const int lane = w.lane, frame = w.frame;
    const size_t rec_index = w.rec_index;
    const uint32_t *in32 = w.in32, mine = w.mine, dw0 = w.dw0;
    uint32_t *out32 = w.out32, *info32 = w.info32;

    float *toc = s_mem[w.wave];
    float *llr = toc + kTocFloats;
    float *zr = toc + kWaveLds, *zi = zr + kZPlane;

    const ft8gpu_candidate cand = cands[rec_index];
    const int T = 2 * cand.time_offset + cand.time_sub, F = 2 * cand.freq_offset + cand.freq_sub;
    const float *pi = iq + (size_t)frame * 2 * kNSamples, *pq = pi + kNSamples;
    const float2 *w4 = tab->w4;

    float twr[8], twi[8];                                             // w4[8 t l]: the lane's twiddles, for the whole candidate
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float2 w = w4[(8u * (uint32_t)t * (uint32_t)lane) & kTabMask];
        twr[t] = w.x;
        twi[t] = w.y;
    }

    // ---- fine sync: e = -4 .. 4 at d = 0, then d = -2, -1, 1, 2 at e* (d = 0 is the time search's best) -----------------------
    const int S0 = 256 * T + FT8GPU_REFINE_LEAD;
    int e_best = -FT8GPU_DEMOD_TRANGE, d_best = -FT8GPU_DEMOD_FRANGE;
    float pt_best = 0.0f, pf_best = 0.0f;
#pragma unroll 1
    for (int h = 0; h < kHyp; ++h) {
        const int nt = 2 * FT8GPU_DEMOD_TRANGE + 1;
        const int e = h < nt ? h - FT8GPU_DEMOD_TRANGE : e_best;
        const int d = h < nt ? 0 : (h - nt < FT8GPU_DEMOD_FRANGE ? h - nt - FT8GPU_DEMOD_FRANGE : h - nt - FT8GPU_DEMOD_FRANGE + 1);
        const int S = S0 + FT8GPU_DEMOD_TSTEP * e;
        const uint32_t k4 = (uint32_t)(4 * F + d);
        float P = 0.0f;
#pragma unroll 1
        for (int i = 0; i < 21; ++i) {
            const int g = i / 7, k = i - 7 * g;
            const int m = 36 * g + k, tone = c_costas[k];
            float vr[8], vi[8];
            symbol_dft(pi, pq, w4, S + 512 * m, 512u * (uint32_t)m, k4, lane, twr, twi, vr, vi);
            float sr = vr[0], si = vi[0];
#pragma unroll
            for (int t = 1; t < 8; ++t) {
                sr = tone == t ? vr[t] : sr;
                si = tone == t ? vi[t] : si;
            }
            sr = wave_bfly_add(sr);
            si = wave_bfly_add(si);
            P = P + (sr * sr + si * si);
        }
        P = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(P)));
        if (h < nt) {
            if (h == 0 || P > pt_best) {
                pt_best = P;
                e_best = e;
            }
        } else {
            if (h == nt || P > pf_best) {
                pf_best = P;
                d_best = d;
            }
            if (h == nt + FT8GPU_DEMOD_FRANGE - 1 && pt_best > pf_best) {   // d = 0 takes its turn behind d = -1
                pf_best = pt_best;
                d_best = 0;
            }
        }
    }
    if (pf_best != pf_best) pf_best = __uint_as_float(0x7FC00000u);   // one NaN, whatever the operations left

    // ---- spectra: Z[m][t] at (e*, d*) ----------------------------------------------------------------------------------------
    {
        const int S = S0 + FT8GPU_DEMOD_TSTEP * e_best;
        const uint32_t k4 = (uint32_t)(4 * F + d_best);
#pragma unroll 1
        for (int m = 0; m < FT8GPU_NN; ++m) {
            float vr[8], vi[8];
            symbol_dft(pi, pq, w4, S + 512 * m, 512u * (uint32_t)m, k4, lane, twr, twi, vr, vi);
            float mr = 0.0f, mi = 0.0f;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float sr = wave_bfly_add(vr[t]), si = wave_bfly_add(vi[t]);
                mr = lane == t ? sr : mr;
                mi = lane == t ? si : mi;
            }
            if (lane < 8) {
                zr[kZPitch * m + lane] = mr;
                zi[kZPitch * m + lane] = mi;
            }
        }
    }
    wave_lds_sync();

    // ---- the sets in ascending n: soft bits, normalisation, bp_decode, the checks ---------------------------------------------
    const bool has[3] = { true, true, lane + 128 < kLdpcN };
    const uint64_t has2_mask = __ballot(has[2]);
    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);              // the record is composed where the soft bits were
    float *rows = kEmit ? soft + rec_index * (3 * kSoftStride) : nullptr;
    int result = 0, nhard = 0, set = 0;
#pragma unroll 1
    for (int n = 1; n <= 3; ++n) {
        if (((sets >> (n - 1)) & 1) == 0) {                           // wave-uniform
            if (kEmit) zero_row(rows, n, lane);
            continue;
        }
        set = n;
        nhard = 0;
        wave_lds_sync();                                              // the last set's reads of llr are done
        const bool finite_mag = set_bits(n, zr, zi, llr, lane);
        wave_lds_sync();
        if (!finite_mag) {
            result = 6;
            if (kEmit) zero_row(rows, n, lane);
            continue;
        }
        float cw[3];
        int ieee = force_ieee_div ? 1 : 0;                            // and the guard ahead of iteration 0 (cand_dev.h)
        if (!renormalise_in_order(llr, has, lane, cw, ieee)) {        // wave-uniform: BP does not run
            result = 6;
            if (kEmit) zero_row(rows, n, lane);
            continue;
        }
        if (kEmit) emit_row(rows, n, cw, lane);                       // x as bp_decode gets it
        const uint64_t X0 = __ballot(cw[0] > 0.0f), X1 = __ballot(cw[1] > 0.0f), X2 = __ballot(cw[2] > 0.0f);

        const BpWord bp = bp_decode_counting(cw, has, has2_mask, toc, ldpc_lane(d_ldpc, lane), lane, max_iters, ieee);
        result = judge_bp_word(bp, X0, X1, X2, max_hard_errors, dw0, d_ldpc.crc_bit, rec32, lane, nhard);
        if (result == 1) {
            if (kEmit) for (int m = n + 1; m <= 3; ++m) zero_row(rows, m, lane);   // the sets not reached
            break;
        }
    }
    store_record(out32, in32, rec32, mine, result == 1, lane);
    if (lane < 4) {
        uint32_t v = 0u;
        if (lane == 0) v = (uint32_t)result | (uint32_t)set << 8 | (uint32_t)nhard << 16 | (uint32_t)(uint8_t)(int8_t)e_best << 24;
        else if (lane == 1) v = (uint32_t)(uint8_t)(int8_t)d_best;
        else if (lane == 2) v = __float_as_uint(pf_best);
        info32[lane] = v;
    }
}

__global__ __launch_bounds__(256)
void ft8_demod_kernel(const float *__restrict__ iq, const ft8gpu_candidate *__restrict__ cands, const int32_t *__restrict__ counts,
                      const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, int nframes,
                      int max_candidates, const SubTables *__restrict__ tab, int sets, int max_hard_errors, int max_iters,
                      int force_ieee_div, unsigned blocks_per_frame) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kDemodLds];
    demod_body<false>(s_mem, iq, cands, counts, status_in, status_out, info, nullptr, nframes, max_candidates, tab, sets,
                      max_hard_errors, max_iters, force_ieee_div, blocks_per_frame);
}

// the same with the soft bits of the sets written out: soft [nframes][max_candidates][3][FT8GPU_SOFT_STRIDE]
__global__ __launch_bounds__(256)
void ft8_demod_soft_kernel(const float *__restrict__ iq, const ft8gpu_candidate *__restrict__ cands, const int32_t *__restrict__ counts,
                           const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_demod_info *info,
                           float *soft, int nframes, int max_candidates, const SubTables *__restrict__ tab, int sets,
                           int max_hard_errors, int max_iters, int force_ieee_div, unsigned blocks_per_frame) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kDemodLds];
    demod_body<true>(s_mem, iq, cands, counts, status_in, status_out, info, soft, nframes, max_candidates, tab, sets,
                     max_hard_errors, max_iters, force_ieee_div, blocks_per_frame);
}

}  // namespace

hipError_t demod_tables_init(hipStream_t s) {
    return upload_ldpc_tables(HIP_SYMBOL(d_ldpc), s);
}

hipError_t launch_demod(const float *iq, const ft8gpu_candidate *cands, const int32_t *counts, const ft8gpu_decode_status *status_in,
                        ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, float *soft, int nframes, int max_candidates,
                        const SubTables *tab, int sets, int max_hard_errors, int max_per_frame, int ldpc_iters, int force_ieee_div,
                        hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    CandGrid g;
    if (cand_grid(nframes, max_candidates, g) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ft8_demod_select_kernel, dim3((unsigned)nframes), dim3(64), 0, s, counts, status_in, info, max_candidates,
                       max_per_frame);
    if (soft)
        hipLaunchKernelGGL(ft8_demod_soft_kernel, dim3(g.nblocks), dim3(256), 0, s, iq, cands, counts, status_in, status_out, info, soft,
                           nframes, max_candidates, tab, sets, max_hard_errors, ldpc_iters, force_ieee_div, g.bpf);
    else
        hipLaunchKernelGGL(ft8_demod_kernel, dim3(g.nblocks), dim3(256), 0, s, iq, cands, counts, status_in, status_out, info,
                           nframes, max_candidates, tab, sets, max_hard_errors, ldpc_iters, force_ieee_div, g.bpf);
    return hipGetLastError();
}

hipError_t launch_demod_tag(const int32_t *n_before, const int32_t *n_msgs, int nframes, const ft8gpu_demod_info *info,
                            int max_candidates, ft8gpu_message *msgs, hipStream_t s) {
    // pad[3] of the records the append step added: the accepted set, 0 where cand_index is out of range
    return launch_tag(nullptr, n_before, 1, n_msgs, nframes, msgs,
                      TagInfo<3, ft8gpu_demod_info, &ft8gpu_demod_info::set, 0, true>{ info, max_candidates }, s);
}
