// api_ap.hip -- host side of a-priori decoding: the lazily allocated buffers, the stage entry ft8gpu_ap_candidates, the AP
// rescue step and ft8gpu_decode_messages_ap, which runs AP, then OSD (api_osd.hip), behind every pass of the masking whole
// path (api_multipass.hip; DESIGN.md "A-priori decoding").
#include "ft8gpu_ctx.h"

namespace {

constexpr int kApMaxHard = kLdpcN, kOsdMaxOrder = 2;

// the constant tables, the info records and the host form's staging of status_out, on the first AP call
// (ft8gpu_create's footprint is unchanged)
int ensure_ap_buffers(ft8gpu_ctx *c) {
    if (tables_once(c, &c->ap_tables, ap_tables_init)) return -1;
    if (c->mem.once(&c->d_nap, (size_t)c->max_frames * sizeof(int32_t), "the counts before AP")) return -1;
    return follow_cap(c, &c->d_ap_info, &c->d_ap_out, &c->ap_cap, "the AP records");
}

int popcount8(unsigned v) { int n = 0; for (; v; v &= v - 1) ++n; return n; }

}  // namespace

int check_ap_args(const ft8gpu_ap_hypothesis *hyps, int nhyp, int max_hard_errors) {
    if (nhyp < 1 || nhyp > FT8GPU_AP_MAX_HYPOTHESES) return ft8_fail("nhyp %d out of range [1, %d]", nhyp, FT8GPU_AP_MAX_HYPOTHESES);
    if (max_hard_errors < 0 || max_hard_errors > kApMaxHard)
        return ft8_fail("max_hard_errors %d out of range [0, %d]", max_hard_errors, kApMaxHard);
    if (!hyps) return ft8_fail("hyps is NULL");
    for (int k = 0; k < nhyp; ++k) {
        int masked = 0;
        for (int j = 0; j < 10; ++j) {
            if (hyps[k].bits[j] & ~hyps[k].mask[j]) return ft8_fail("hypothesis %d has bits outside its mask", k);
            masked += popcount8(hyps[k].mask[j]);
        }
        if (hyps[k].mask[9] & 7u) return ft8_fail("hypothesis %d masks bits past the 77 payload bits", k);
        if (masked < 1) return ft8_fail("hypothesis %d masks no bit", k);
    }
    return 0;
}

namespace {

// AP on a pass's failures, in place, then the append step and the tags of what it gained; its count goes to column col
int ap_step(const Chunk &k, const PassSet &f, int col, const ft8gpu_ap_params *q) {
    ft8gpu_ctx *c = k.c;
    const ft8gpu_params &p = c->params;
    const int mc = p.max_candidates;
    HIP_TRY(hipMemcpyAsync(c->d_nap, k.n_msgs, (size_t)k.n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(launch_ap(f.mag, f.cands, f.counts, f.status, f.status, c->d_ap_info, f.nslots, mc, p.ldpc_iters, force_ieee(c), q->hyps,
                      q->nhyp, q->ap_max_hard_errors, c->stream));
    HIP_TRY(launch_append(f.mag, c->d_base, f.cands, f.counts, f.status, c->d_msgtab, f.map, f.nslots, mc, p.min_score, k.msgs, k.n_msgs,
                          c->stream));
    HIP_TRY(launch_ap_tag(c->d_ap_info, f.map, c->d_nap, k.n_msgs, f.nslots, mc, k.msgs, c->stream));
    return k.counts_to(col);
}

}  // namespace

extern "C" {

int ft8gpu_ap_candidates(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                         const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_ap_hypothesis *hyps, int nhyp,
                         int max_hard_errors, ft8gpu_decode_status *status_out, ft8gpu_ap_info *info, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_ap_args(hyps, nhyp, max_hard_errors)) return -1;
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status_in || !status_out || !info) return ft8_fail("NULL array argument");
    if (ensure_ap_buffers(c)) return -1;
    const int mc = c->params.max_candidates;
    StageArg a[kCandRows];
    cand_stage_rows(a, c, { mag, c->d_mag, kMagArray, kIn }, cands, counts, status_in, status_out, c->d_ap_out, info, c->d_ap_info,
                    sizeof(ft8gpu_ap_info));
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        HIP_TRY(launch_ap((const uint8_t *)p[0], (const ft8gpu_candidate *)p[1], (const int32_t *)p[2],
                          (const ft8gpu_decode_status *)p[3], (ft8gpu_decode_status *)p[4], (ft8gpu_ap_info *)p[5], n, mc,
                          c->params.ldpc_iters, force_ieee(c), hyps, nhyp, max_hard_errors, c->stream));
        return 0;
    });
}

int ft8gpu_decode_messages_ap(ft8gpu_ctx *c, const float *iq, int nframes, const ft8gpu_ap_params *params,
                              ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags) {
    CHECK_COMMON(c, nframes);
    if (!params) return ft8_fail("params is NULL");
    const int passes = params->passes, order = params->osd_order, nhyp = params->nhyp;
    if (passes < 1 || passes > FT8GPU_MAX_PASSES) return ft8_fail("passes %d out of range [1, %d]", passes, FT8GPU_MAX_PASSES);
    if (nhyp < 0 || nhyp > FT8GPU_AP_MAX_HYPOTHESES) return ft8_fail("nhyp %d out of range [0, %d]", nhyp, FT8GPU_AP_MAX_HYPOTHESES);
    if (nhyp > 0 && check_ap_args(params->hyps, nhyp, params->ap_max_hard_errors)) return -1;
    if (order < -1 || order > kOsdMaxOrder) return ft8_fail("osd_order %d out of range [-1, %d]", order, kOsdMaxOrder);
    if (order >= 0 && check_osd_args(order, params->osd_max_hard_errors)) return -1;
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    if (ensure_multipass_buffers(c)) return -1;
    if (nhyp > 0 && ensure_ap_buffers(c)) return -1;
    if (order >= 0 && ensure_osd_buffers(c)) return -1;
    return decode_messages_masked(c, iq, nframes, passes, 3, msgs, n_msgs, n_by_stage, flags, [=](const Chunk &k, const PassSet &f, int col) {
        if (nhyp > 0 && ap_step(k, f, col, params)) return -1;
        return order >= 0 ? osd_step(k, f, col + 1, order, params->osd_max_hard_errors) : 0;
    });
}

}  // extern "C"
