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
// One wave64 per candidate, four per workgroup, the launch geometry of the LDPC kernel (decode.hip).  The head of the kernel,
// the soft bits, the BP iteration in its counting form with both division streams behind the per-iteration guard, the tail
// of the judgement (all-zero, hard errors, the CRC by linearity, the record composed in LDS) and the kernel that tags the
// message records are the shared device code of cand_dev.h.  What is this file's own: the block order, apmag by a wave
// maximum, the hypothesis loop inside the wave (masks and bits arrive as kernel arguments: scalar registers), rules 7 and 8
// and the hard errors on the unmasked positions.  The
// guard's premise holds for the forced values too: apmag is one of the candidate's own magnitudes, so a halved LLR is
// still 0 or >= 0.0095 (cand_dev.h, guard_key).
#include "cand_dev.h"

namespace {

__device__ LdpcTables d_ldpc;

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

    static_assert(sizeof(ft8gpu_ap_info) == 8, "record sizes");
    static_assert(offsetof(ft8gpu_ap_info, nhard) == 1 && offsetof(ft8gpu_ap_info, hyp) == 2 && offsetof(ft8gpu_ap_info, iters) == 3 &&
                  offsetof(ft8gpu_ap_info, results) == 4, "info layout");
    // the LDPC kernel's block order and frame / candidate split (decode.hip: XCD-aware renumbering; one multiply-high, and
    // no division at all for one block per frame, where the constant does not exist)
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
        leave_record(out32, in32, info32, mine, 6u, lane);
        return;
    }
    // h = llr > 0, as ballot words over the codeword positions
    const uint64_t H0 = __ballot(cw0[0] > 0.0f), H1 = __ballot(cw0[1] > 0.0f), H2 = __ballot(cw0[2] > 0.0f);

    const LdpcLane L = ldpc_lane(d_ldpc, lane);
    const uint64_t has2_mask = __ballot(has[2]);         // lanes that own a third variable (n = lane + 128 < 174)

    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);            // the record is composed where the raw soft bits were
    uint32_t results = 0;
    int result = 0, nhard = 0, iters_out = 0, hyp = 0;

    for (int k = 0; k < nhyp; ++k) {                                  // wave-uniform
        const uint64_t m0 = hyps.mask[k][0], m1 = hyps.mask[k][1], b0 = hyps.bits[k][0], b1 = hyps.bits[k][1];
        // (These lines, down to the judgement, exist a second time as cand_dev.h's ap_try, which hint.hip calls: change both.
        // tests/test_gpu_hint.py holds the hint stage to this kernel candidate by candidate.)
        // ---- the hypothesis's soft bits: +-apmag on the masked positions ------------------------------------------------
        float cw[3];
        {
            const bool f0 = ((m0 >> lane) & 1ull) != 0ull, f1 = ((m1 >> lane) & 1ull) != 0ull;
            cw[0] = f0 ? (((b0 >> lane) & 1ull) ? apmag : -apmag) : cw0[0];
            cw[1] = f1 ? (((b1 >> lane) & 1ull) ? apmag : -apmag) : cw0[1];
            cw[2] = cw0[2];
        }
        const BpWord bp = bp_decode_counting(cw, has, has2_mask, toc, L, lane, max_iters, force_ieee_div);
        const uint64_t B0 = bp.B0, B1 = bp.B1, B2 = bp.B2;

        // ---- judge the word BP left: the first failing check names the result ---------------------------------------------
        hyp = k;
        iters_out = bp.iter < 255 ? bp.iter : 255;
        // hard errors: unmasked positions at which the word differs from h (the mask covers payload positions only)
        nhard = __popcll((B0 ^ H0) & ~m0) + __popcll((B1 ^ H1) & ~m1) + __popcll(B2 ^ H2);
        if (bp.min_errors != 0) result = 7;
        else if ((((B0 ^ b0) & m0) | ((B1 ^ b1) & m1)) != 0ull) result = 8;
        else result = judge_word(B0, B1, B2, nhard, max_hard_errors, dw0, d_ldpc.crc_bit, rec32, lane);
        results |= (uint32_t)result << (8 * k);
        if (result == 1) break;
    }

    store_record(out32, in32, rec32, mine, result == 1, lane);
    if (lane == 0) {
        info32[0] = (uint32_t)result | ((uint32_t)nhard << 8) | ((uint32_t)hyp << 16) | ((uint32_t)iters_out << 24);
        info32[1] = results;
    }
}

}  // namespace

hipError_t ap_tables_init(hipStream_t s) {
    return upload_ldpc_tables(HIP_SYMBOL(d_ldpc), s);
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
    CandGrid g;
    if (cand_grid(nframes, max_candidates, g, true) != hipSuccess) return hipErrorInvalidValue;
    const unsigned magic = g.bpf == 1u ? 0u : (unsigned)((1ull << 32) / g.bpf) + 1u;
    hipLaunchKernelGGL(ft8_ap_kernel, dim3(g.nblocks), dim3(256), 0, s, mag, cands, counts, status_in, status_out, info,
                       nframes, max_candidates, ldpc_iters, force_ieee_div, nhyp, max_hard_errors, set, g.bpf, magic);
    return hipGetLastError();
}

hipError_t launch_ap_tag(const ft8gpu_ap_info *info, const int32_t *map, const int32_t *n_before, const int32_t *n_msgs,
                         int nslots, int max_candidates, ft8gpu_message *msgs, hipStream_t s) {
    // pad[1] of the message records AP gained: 1 + the accepted hypothesis
    return launch_tag(map, n_before, 1, n_msgs, nslots, msgs, TagInfo<1, ft8gpu_ap_info, &ft8gpu_ap_info::hyp, 1>{ info, max_candidates }, s);
}
