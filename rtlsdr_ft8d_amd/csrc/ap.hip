// ap.hip -- a-priori decoding of the candidates belief propagation gives up on (DESIGN.md "A-priori decoding").  Not part
// of the reference's path: a candidate whose status record says ok == 0 and ldpc_errors != 0 runs BP again with the soft
// bits of known message bits (a hypothesis: 77 payload bits and a mask, e.g. the 32 constant bits of "CQ CALL GRID") fixed
// at the candidate's largest magnitude.  The rule is exact and restated in tests/ft8_spec_ap.py (include/ft8gpu.h has it
// in full):
//   llr = the soft bits the LDPC kernel starts from (ft8_extract_likelihood, ftx_normalize_logl of ft8_lib decode.c, reached
//   through ft8_decode, rtlsdr_ft8d.c:1476); h = llr > 0; apmag = max |llr|; per hypothesis, in table order: masked
//   positions become +-apmag, bp_decode (ft8_lib ldpc.c) runs on the result, and the word is judged -- no codeword (7),
//   disagrees with the hypothesis (8), all-zero (5), hard errors on the unmasked positions (2), CRC (3), unpack77 (4),
//   accepted (1).  The first accepted hypothesis wins.
//
// One wave64 per candidate, four per workgroup, the launch geometry of the LDPC kernel (decode.hip), whose arithmetic this
// file keeps as a copy in its counting form -- the soft bits, the BP iteration with both division streams behind the
// per-iteration guard, the CRC by linearity, unpack77 on two 64-bit words, the record composed in LDS -- so that decode.hip
// stays byte for byte what it is.  What is new around it: the early exit of a candidate that does not qualify, apmag by a
// wave maximum, the hypothesis loop inside the wave (masks and bits arrive as kernel arguments: scalar registers), and the
// judgement.  The guard's premise holds for the forced values too: apmag is one of the candidate's own magnitudes, so a
// halved LLR is still 0 or >= 0.0095 (decode.hip, guard_key).
#include "ft8gpu_internal.h"
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

struct ApTables {
    uint16_t edge_slot[3][64][3];     // [r][lane][m_idx] -> float index of slot (m, pos) in the LDS tile
    uint64_t rowmask[2][64][3];       // [rr][lane][word] bit mask of the variables of check m = lane + 64 rr
    uint8_t  row_valid[2][64];
    uint8_t  own6[64], own7[64];      // product ownership (decode.hip)
    uint16_t crc_bit[77];             // CRC-14 (over 82 bits) of the message whose only set bit is payload bit i
};

__device__ ApTables d_ap;
__constant__ uint8_t c_ap_gray[8] = { 0, 1, 3, 2, 5, 6, 4, 7 };

constexpr int kRows = 84;                     // 83 check rows + 1 spare row for idle lanes
constexpr int kTocFloats = kRows * 8;         // plane LO: [84] float4 (slots 0..3), plane HI: [84] float4 (slots 4..7)
constexpr int kWaveLds = kTocFloats + 192;    // + 174 LLRs

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
constexpr uint32_t kGuardMin = ((127u - 59u) << 24) - 1u;       // guard_key(0x1p-59f)

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
// the largest of 64 non-negative values (once per candidate: plain butterflies)
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

}  // namespace

// the hypotheses as the kernel wants them: masks and bits over codeword positions 0..63 and 64..127 (payload bit i is
// bit i & 63 of word i >> 6; only 0..76 can be set)
struct ApHypSet {
    uint64_t mask[FT8GPU_AP_MAX_HYPOTHESES][2];
    uint64_t bits[FT8GPU_AP_MAX_HYPOTHESES][2];
};

namespace {

__global__ __launch_bounds__(256)
void ft8_ap_kernel(const uint8_t *__restrict__ mag, const ft8gpu_candidate *__restrict__ cands,
                   const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                   ft8gpu_decode_status *status_out, ft8gpu_ap_info *info, int nframes, int max_candidates,
                   int max_iters, int force_ieee_div, int nhyp, int max_hard_errors, ApHypSet hyps,
                   unsigned blocks_per_frame, unsigned bpf_magic) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kWaveLds];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the LDPC kernel's block order and frame / candidate split (decode.hip: XCD-aware renumbering; one multiply-high, and
    // no division at all for one block per frame, where the constant does not exist)
    const unsigned nb = gridDim.x, per = nb >> 3, main_blocks = per << 3;
    const unsigned vb = blockIdx.x < main_blocks ? (blockIdx.x & 7u) * per + (blockIdx.x >> 3) : blockIdx.x;
    const int frame = blocks_per_frame == 1u ? (int)vb : (int)__umulhi(vb, bpf_magic);
    const int ci = (int)(vb - (unsigned)frame * blocks_per_frame) * 4 + wave;
    if (frame >= nframes || ci >= max_candidates) return;
    if (ci >= counts[frame]) return;                                  // wave-uniform: records behind the count are not touched

    const size_t rec_index = (size_t)frame * max_candidates + ci;
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(status_in + rec_index);
    uint32_t *out32 = reinterpret_cast<uint32_t *>(status_out + rec_index);
    uint32_t *info32 = reinterpret_cast<uint32_t *>(info + rec_index);
    static_assert(sizeof(ft8gpu_decode_status) == 48 && sizeof(ft8gpu_ap_info) == 8, "record sizes");
    static_assert(offsetof(ft8gpu_ap_info, nhard) == 1 && offsetof(ft8gpu_ap_info, hyp) == 2 && offsetof(ft8gpu_ap_info, iters) == 3 &&
                  offsetof(ft8gpu_ap_info, results) == 4, "info layout");

    // ---- which candidates: ok == 0 and ldpc_errors != 0 (status_out may be status_in: read first) -------------------
    const uint32_t mine = lane < 12 ? in32[lane] : 0u;
    const uint32_t dw0 = (uint32_t)__builtin_amdgcn_readlane((int)mine, 0);
    const uint32_t dw2 = (uint32_t)__builtin_amdgcn_readlane((int)mine, 2);
    const bool attempt = ((dw2 >> 8) & 0xFFu) == 0u && (dw0 & 0xFFFFu) != 0u;
    if (!attempt) {
        if (lane < 12 && out32 != in32) out32[lane] = mine;
        if (lane < 2) info32[lane] = 0u;
        return;
    }

    float *toc = s_mem[wave];
    float *llr = toc + kTocFloats;
    float4 *planeLO = reinterpret_cast<float4 *>(toc);
    float4 *planeHI = planeLO + kRows;

    const ft8gpu_candidate cand = cands[rec_index];

    // ---- ft8_extract_likelihood ------------------------------------------------------------
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
            for (int j = 0; j < 8; ++j) s2[j] = ps[c_ap_gray[j]];
            l0 = max(max(s2[4], s2[5]), max(s2[6], s2[7])) - max(max(s2[0], s2[1]), max(s2[2], s2[3]));
            l1 = max(max(s2[2], s2[3]), max(s2[6], s2[7])) - max(max(s2[0], s2[1]), max(s2[4], s2[5]));
            l2 = max(max(s2[1], s2[3]), max(s2[5], s2[7])) - max(max(s2[0], s2[2]), max(s2[4], s2[6]));
        }
        llr[3 * k + 0] = (float)l0;
        llr[3 * k + 1] = (float)l1;
        llr[3 * k + 2] = (float)l2;
    }
    wave_lds_sync();

    // ---- ftx_normalize_logl ----------------------------------------------------------------
    float cw0[3];
    bool has[3];
    int isum = 0, isum2 = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int n = lane + 64 * r;
        has[r] = n < kLdpcN;
        cw0[r] = has[r] ? llr[n] : 0.0f;
        const int v = (int)cw0[r];
        isum += v;
        isum2 += v * v;
    }
    const float sum = (float)wave_sum(isum);
    const float sum2 = (float)wave_sum(isum2);
    const float inv_n = 1.0f / 174;
    const float variance = (sum2 - (sum * sum * inv_n)) * inv_n;
    const float norm_factor = bpm::llr_norm_factor(variance);       // sqrtf(24.0f / variance), both correctly rounded (bp_math.h)
    bool finite = true;
    uint32_t amax = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        cw0[r] = has[r] ? cw0[r] * norm_factor : 0.0f;
        const uint32_t a = __float_as_uint(cw0[r]) & 0x7FFFFFFFu;
        finite = finite && a < 0x7F800000u;
        amax = max(amax, a);
    }
    const bool all_finite = __all(finite);
    const float apmag = __uint_as_float(wave_max(amax));              // non-negative floats order as their bit patterns
    if (!all_finite || apmag == 0.0f) {                               // wave-uniform: nothing is tried
        if (lane < 12 && out32 != in32) out32[lane] = mine;
        if (lane < 2) info32[lane] = lane == 0 ? 6u : 0u;
        return;
    }
    // h = llr > 0, as ballot words over the codeword positions
    const uint64_t H0 = __ballot(cw0[0] > 0.0f), H1 = __ballot(cw0[1] > 0.0f), H2 = __ballot(cw0[2] > 0.0f);

    // ---- per-lane constant edge / row data ---------------------------------------------------
    int slot[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int e = 0; e < 3; ++e) slot[3 * r + e] = d_ap.edge_slot[r][lane][e];
    uint64_t rmask[2][3];
    bool rvalid[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        rvalid[rr] = d_ap.row_valid[rr][lane] != 0;
#pragma unroll
        for (int w = 0; w < 3; ++w) rmask[rr][w] = d_ap.rowmask[rr][lane][w];
    }
    const int row6 = d_ap.own6[lane], row7 = d_ap.own7[lane];
    const bool has6 = row6 != kRows - 1, has7 = row7 != kRows - 1;
    const uint64_t has2_mask = __ballot(has[2]);         // lanes that own a third variable (n = lane + 128 < 174)

    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);            // the record is composed where the raw soft bits were
    char *rec = reinterpret_cast<char *>(llr);
    uint32_t results = 0;
    int result = 0, nhard = 0, iters_out = 0, hyp = 0;

    for (int k = 0; k < nhyp; ++k) {                                  // wave-uniform
        const uint64_t m0 = hyps.mask[k][0], m1 = hyps.mask[k][1], b0 = hyps.bits[k][0], b1 = hyps.bits[k][1];
        // ---- the hypothesis's soft bits: +-apmag on the masked positions ------------------------------------------------
        float cw[3];
        {
            const bool f0 = ((m0 >> lane) & 1ull) != 0ull, f1 = ((m1 >> lane) & 1ull) != 0ull;
            cw[0] = f0 ? (((b0 >> lane) & 1ull) ? apmag : -apmag) : cw0[0];
            cw[1] = f1 ? (((b1 >> lane) & 1ull) ? apmag : -apmag) : cw0[1];
            cw[2] = cw0[2];
        }
        // the spare row only needs finite content (idle lanes of the variable side read and write it)
        wave_lds_sync();                                              // the previous hypothesis's reads of the tile are done
        if (lane < 8) toc[slot_index(kRows - 1, lane)] = 1.0f;
        wave_lds_sync();

        // ---- bp_decode: the iteration of decode.hip, counting form (the comments there explain the layout) ---------------
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
        hyp = k;
        iters_out = iter < 255 ? iter : 255;
        // hard errors: unmasked positions at which the word differs from h (the mask covers payload positions only)
        nhard = __popcll((B0 ^ H0) & ~m0) + __popcll((B1 ^ H1) & ~m1) + __popcll(B2 ^ H2);
        const uint64_t w0 = __brevll(B0);                                 // codeword bits 0..63, MSB first
        const uint64_t w1 = __brevll(B1) & 0xFFFFFFE000000000ull;         // bits 64..90
        if (min_errors != 0) result = 7;
        else if ((((B0 ^ b0) & m0) | ((B1 ^ b1) & m1)) != 0ull) result = 8;
        else if ((B0 | B1 | B2) == 0ull) result = 5;                      // (bp_decode leaves at an all-zero word before it checks it)
        else if (nhard > max_hard_errors) result = 2;
        else {
            uint32_t c = ((B0 >> lane) & 1ull) ? d_ap.crc_bit[lane] : 0u;
            if (lane < 13 && ((B1 >> lane) & 1ull)) c ^= d_ap.crc_bit[64 + lane];
            const uint32_t crc_calc = wave_xor(c);
            const uint32_t crc_extracted = (uint32_t)(w1 >> 37) & 0x3FFFu;
            if (crc_extracted != crc_calc) result = 3;
            else {
                // the record of a BP success (decode.hip), iters as it was
                static_assert(offsetof(ft8gpu_decode_status, a91) == 10 && offsetof(ft8gpu_decode_status, text) == 22, "record layout");
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
        results |= (uint32_t)result << (8 * k);
        if (result == 1) break;
    }

    if (lane < 12 && (result == 1 || out32 != in32)) out32[lane] = result == 1 ? rec32[lane] : mine;
    if (lane == 0) {
        info32[0] = (uint32_t)result | ((uint32_t)nhard << 8) | ((uint32_t)hyp << 16) | ((uint32_t)iters_out << 24);
        info32[1] = results;
    }
}

// pad[1] of the message records AP gained: 1 + the accepted hypothesis.  One wave per slot of the pass.
__global__ __launch_bounds__(256)
void ft8_ap_tag_kernel(const ft8gpu_ap_info *__restrict__ info, const int32_t *__restrict__ map,
                       const int32_t *__restrict__ n_before, const int32_t *__restrict__ n_msgs, int nslots,
                       int max_candidates, ft8gpu_message *__restrict__ msgs) {
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), r = threadIdx.x & 63;
    if (slot >= nslots) return;
    const int frame = map ? map[slot] : slot;
    int lo = n_before[frame], hi = n_msgs[frame];
    lo = lo < 0 ? 0 : lo;
    hi = hi > kMaxMessages ? kMaxMessages : hi;
    if (r < lo || r >= hi) return;
    ft8gpu_message *m = msgs + (size_t)frame * kMaxMessages + r;
    const int ci = m->cand_index;
    if (ci < max_candidates) m->pad[1] = (uint8_t)(1 + info[(size_t)slot * max_candidates + ci].hyp);
}

}  // namespace

hipError_t ap_tables_init(hipStream_t s) {
    static ApTables h;
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
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(d_ap), &h, sizeof(h), 0, hipMemcpyHostToDevice, s);
}

hipError_t launch_ap(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                     const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_ap_info *info,
                     int nframes, int max_candidates, int ldpc_iters, int force_ieee_div,
                     const ft8gpu_ap_hypothesis *hyps, int nhyp, int max_hard_errors, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    if (nhyp < 1 || nhyp > FT8GPU_AP_MAX_HYPOTHESES) return hipErrorInvalidValue;
    ApHypSet set = {};
    for (int k = 0; k < nhyp; ++k)
        for (int i = 0; i < 77; ++i) {
            const unsigned sh = 7u - (unsigned)(i & 7);
            if ((hyps[k].mask[i >> 3] >> sh) & 1u) set.mask[k][i >> 6] |= 1ull << (i & 63);
            if ((hyps[k].bits[i >> 3] >> sh) & 1u) set.bits[k][i >> 6] |= 1ull << (i & 63);
        }
    const unsigned bpf = (unsigned)(max_candidates + 3) / 4;                  // blocks (of 4 candidate waves) per frame
    const unsigned long long nblocks = (unsigned long long)nframes * bpf;
    if (nblocks * bpf >= (1ull << 32)) return hipErrorInvalidValue;           // keeps the multiply-high division exact
    const unsigned magic = bpf == 1u ? 0u : (unsigned)((1ull << 32) / bpf) + 1u;
    hipLaunchKernelGGL(ft8_ap_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info,
                       nframes, max_candidates, ldpc_iters, force_ieee_div, nhyp, max_hard_errors, set, bpf, magic);
    return hipGetLastError();
}

hipError_t launch_ap_tag(const ft8gpu_ap_info *info, const int32_t *map, const int32_t *n_before, const int32_t *n_msgs,
                         int nslots, int max_candidates, ft8gpu_message *msgs, hipStream_t s) {
    if (nslots < 1) return hipSuccess;
    hipLaunchKernelGGL(ft8_ap_tag_kernel, dim3((nslots + 3) / 4), dim3(256), 0, s, info, map, n_before, n_msgs, nslots,
                       max_candidates, msgs);
    return hipGetLastError();
}
