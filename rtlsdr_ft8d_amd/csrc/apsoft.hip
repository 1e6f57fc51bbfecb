// apsoft.hip -- a-priori decoding on a soft-bit array (DESIGN.md "A-priori decoding on the demodulated soft bits"; the rule is in
// include/ft8gpu.h at ft8gpu_ap_soft_candidates, restated in tests/ft8_spec_apsoft.py).  Not part of the reference's path.
// demod.hip leaves, per candidate, up to three rows of normalised soft bits (one per set of the demodulation from the I/Q
// samples); a candidate that is still undecoded runs ap.hip's per-hypothesis rule on each usable row, as it stands.
//
//   ft8_ap_soft_kernel   one wave64 per candidate, four per workgroup, cand_dev.h's head of the kernel and launch geometry.
//                        The set loop and the hypothesis loop run inside the wave: a row is loaded once (load_soft_row: the
//                        finite test, apmag by a wave maximum, the division guard ahead of iteration 0 -- the rows are
//                        arbitrary finite floats, so the guard cannot be argued from their structure as ap.hip does), the
//                        hypotheses' masks and bits arrive as kernel arguments, and each hypothesis is cand_dev.h's ap_try.
//                        Which division ran never shows: the output is bp_decode's.
//   launch_ap_soft_tag   pad[1] = 1 + hypothesis, pad[3] = set of the records the append step added (cand_dev.h's tag kernel).
//
// LDS: 3 456 bytes per wave (the BP tile and the row, where the record of a success is composed), 13 824 per workgroup.
#include "apsoft.h"
#include "cand_dev.h"

namespace {

__device__ LdpcTables d_ldpc;

constexpr int kSoftStride = FT8GPU_SOFT_STRIDE;
static_assert(kSoftStride >= kLdpcN && (3 * kSoftStride * sizeof(float)) % 16 == 0, "soft rows");
static_assert(sizeof(ft8gpu_apsoft_info) == 20 && offsetof(ft8gpu_apsoft_info, set) == 4 && offsetof(ft8gpu_apsoft_info, results) == 8,
              "info layout");

// the hypotheses as the kernel wants them: masks and bits over codeword positions 0..63 and 64..127 (payload bit i is bit
// i & 63 of word i >> 6; only 0..76 can be set)
struct ApSoftHyps {
    uint64_t mask[FT8GPU_AP_MAX_HYPOTHESES][2];
    uint64_t bits[FT8GPU_AP_MAX_HYPOTHESES][2];
};

__global__ __launch_bounds__(256)
void ft8_ap_soft_kernel(const float *__restrict__ soft, const int32_t *__restrict__ counts, const ft8gpu_decode_status *status_in,
                        ft8gpu_decode_status *status_out, ft8gpu_apsoft_info *info, int nframes, int max_candidates, int max_iters,
                        int force_ieee_div, int sets, int nhyp, int max_hard_errors, ApSoftHyps hyps, unsigned blocks_per_frame) {
    __shared__ __attribute__((aligned(16))) float s_mem[4][kWaveLds];

    // does not qualify: the record copied, the five dwords of the info record zero
    const CandWave w = cand_prologue(blockIdx.x, blocks_per_frame, 0u, counts, status_in, status_out, info, nframes, max_candidates);
    if (w.verdict != kCandRun) return;
    const int lane = w.lane;
    const uint32_t *in32 = w.in32, mine = w.mine, dw0 = w.dw0;
    uint32_t *out32 = w.out32, *info32 = w.info32;

    float *toc = s_mem[w.wave];
    float *llr = toc + kTocFloats;
    const float *rows = soft + w.rec_index * (3 * kSoftStride);

    const bool has[3] = { true, true, lane + 128 < kLdpcN };
    const uint64_t has2_mask = __ballot(has[2]);
    const LdpcLane L = ldpc_lane(d_ldpc, lane);

    uint32_t *rec32 = reinterpret_cast<uint32_t *>(llr);              // the record is composed where the row was
    uint32_t res0 = 0u, res1 = 0u, res2 = 0u;                         // results[n - 1] as a dword each (no indexed registers)
    int result = 6, nhard = 0, iters_out = 0, hyp = 0, set = 0;      // what stays when no set is usable
#pragma unroll 1
    for (int n = 1; n <= 3; ++n) {
        if (((sets >> (n - 1)) & 1) == 0) continue;                   // wave-uniform
        wave_lds_sync();                                              // the last set's reads of the record's dwords are done
        float cw0[3], apmag = 0.0f;
        int ieee = force_ieee_div ? 1 : 0;                            // and the guard ahead of iteration 0 (cand_dev.h)
        if (!load_soft_row(rows + (n - 1) * kSoftStride, llr, has, lane, cw0, apmag, ieee)) {   // wave-uniform: nothing is tried
            res0 = n == 1 ? 6u : res0;
            res1 = n == 2 ? 6u : res1;
            res2 = n == 3 ? 6u : res2;
            continue;
        }
        set = n;
        uint32_t res = 0u;
        // h = row > 0, as ballot words over the codeword positions
        const uint64_t H0 = __ballot(cw0[0] > 0.0f), H1 = __ballot(cw0[1] > 0.0f), H2 = __ballot(cw0[2] > 0.0f);
        for (int k = 0; k < nhyp; ++k) {                              // wave-uniform
            hyp = k;
            result = ap_try(cw0, has, has2_mask, toc, L, lane, max_iters, ieee, apmag, hyps.mask[k][0], hyps.mask[k][1], hyps.bits[k][0],
                            hyps.bits[k][1], H0, H1, H2, max_hard_errors, dw0, d_ldpc.crc_bit, rec32, nhard, iters_out);
            res |= (uint32_t)result << (8 * k);
            if (result == 1) break;
        }
        res0 = n == 1 ? res : res0;
        res1 = n == 2 ? res : res1;
        res2 = n == 3 ? res : res2;
        if (result == 1) break;
    }

    store_record(out32, in32, rec32, mine, result == 1, lane);
    if (lane < 5) {
        uint32_t v = (uint32_t)result | ((uint32_t)nhard << 8) | ((uint32_t)hyp << 16) | ((uint32_t)iters_out << 24);
        if (lane == 1) v = (uint32_t)set;
        else if (lane == 2) v = res0;
        else if (lane == 3) v = res1;
        else if (lane == 4) v = res2;
        info32[lane] = v;
    }
}

}  // namespace

hipError_t apsoft_tables_init(hipStream_t s) {
    return upload_ldpc_tables(HIP_SYMBOL(d_ldpc), s);
}

hipError_t launch_ap_soft(const float *soft, const int32_t *counts, const ft8gpu_decode_status *status_in,
                          ft8gpu_decode_status *status_out, ft8gpu_apsoft_info *info, int nframes, int max_candidates, int ldpc_iters,
                          int force_ieee_div, int sets, const ft8gpu_ap_hypothesis *hyps, int nhyp, int max_hard_errors, hipStream_t s) {
    if (nframes < 1) return hipSuccess;
    if (nhyp < 1 || nhyp > FT8GPU_AP_MAX_HYPOTHESES || sets < 1 || sets > 7) return hipErrorInvalidValue;
    ApSoftHyps set = {};
    for (int k = 0; k < nhyp; ++k)
        for (int i = 0; i < 77; ++i) {
            const unsigned sh = 7u - (unsigned)(i & 7);
            if ((hyps[k].mask[i >> 3] >> sh) & 1u) set.mask[k][i >> 6] |= 1ull << (i & 63);
            if ((hyps[k].bits[i >> 3] >> sh) & 1u) set.bits[k][i >> 6] |= 1ull << (i & 63);
        }
    CandGrid g;
    if (cand_grid(nframes, max_candidates, g) != hipSuccess) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ft8_ap_soft_kernel, dim3(g.nblocks), dim3(256), 0, s, soft, counts, status_in, status_out, info, nframes,
                       max_candidates, ldpc_iters, force_ieee_div, sets, nhyp, max_hard_errors, set, g.bpf);
    return hipGetLastError();
}

hipError_t launch_ap_soft_tag(const int32_t *n_before, const int32_t *n_msgs, int nframes, const ft8gpu_apsoft_info *info,
                              int max_candidates, ft8gpu_message *msgs, hipStream_t s) {
    const hipError_t e = launch_tag(nullptr, n_before, 1, n_msgs, nframes, msgs,
                                    TagInfo<1, ft8gpu_apsoft_info, &ft8gpu_apsoft_info::hyp, 1>{ info, max_candidates }, s);
    if (e != hipSuccess) return e;
    return launch_tag(nullptr, n_before, 1, n_msgs, nframes, msgs,
                      TagInfo<3, ft8gpu_apsoft_info, &ft8gpu_apsoft_info::set, 0>{ info, max_candidates }, s);
}
