// api_osd.hip -- host side of ordered-statistics decoding: the lazily allocated buffers, the stage entry
// ft8gpu_osd_candidates, the OSD rescue step and ft8gpu_decode_messages_deep, which runs that step behind every pass of the
// masking whole path (api_multipass.hip; DESIGN.md "Ordered-statistics decoding").
#include "ft8gpu_ctx.h"

namespace {

constexpr int kOsdMaxOrder = 2, kOsdMaxHard = kLdpcM;

}  // namespace

// the constant tables, the info records and the host form's staging of status_out, on the first OSD call
// (ft8gpu_create's footprint is unchanged)
int ensure_osd_buffers(ft8gpu_ctx *c) {
    if (tables_once(c, &c->osd_tables, osd_tables_init)) return -1;
    if (c->mem.once(&c->d_nosd, (size_t)c->max_frames * sizeof(int32_t), "the counts before OSD")) return -1;
    return follow_cap(c, &c->d_osd_info, &c->d_osd_out, &c->osd_cap, "the OSD records");
}

int check_osd_args(int order, int max_hard_errors) {
    if (order < 0 || order > kOsdMaxOrder) return ft8_fail("order %d out of range [0, %d]", order, kOsdMaxOrder);
    if (max_hard_errors < 0 || max_hard_errors > kOsdMaxHard)
        return ft8_fail("max_hard_errors %d out of range [0, %d]", max_hard_errors, kOsdMaxHard);
    return 0;
}

// OSD on a pass's failures, in place, then the append step and the nhard tags of what it gained
int osd_step(const Chunk &k, const PassSet &f, int col, int order, int max_hard_errors) {
    ft8gpu_ctx *c = k.c;
    const int mc = c->params.max_candidates;
    HIP_TRY(hipMemcpyAsync(c->d_nosd, k.n_msgs, (size_t)k.n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(launch_osd(f.mag, f.cands, f.counts, f.status, f.status, c->d_osd_info, f.nslots, mc, order, max_hard_errors, c->stream));
    HIP_TRY(launch_append(f.mag, c->d_base, f.cands, f.counts, f.status, c->d_msgtab, f.map, f.nslots, mc, c->params.min_score, k.msgs,
                          k.n_msgs, c->stream));
    HIP_TRY(launch_osd_tag(c->d_osd_info, f.map, c->d_nosd, k.n_msgs, f.nslots, mc, k.msgs, c->stream));
    return k.counts_to(col);
}

extern "C" {

int ft8gpu_osd_candidates(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                          const ft8gpu_decode_status *status_in, int nframes, int order, int max_hard_errors,
                          ft8gpu_decode_status *status_out, ft8gpu_osd_info *info, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_osd_args(order, max_hard_errors)) return -1;
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status_in || !status_out || !info) return ft8_fail("NULL array argument");
    if (ensure_osd_buffers(c)) return -1;
    const int mc = c->params.max_candidates;
    StageArg a[kCandRows];
    cand_stage_rows(a, c, { mag, c->d_mag, kMagArray, kIn }, cands, counts, status_in, status_out, c->d_osd_out, info, c->d_osd_info,
                    sizeof(ft8gpu_osd_info));
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        HIP_TRY(launch_osd((const uint8_t *)p[0], (const ft8gpu_candidate *)p[1], (const int32_t *)p[2],
                           (const ft8gpu_decode_status *)p[3], (ft8gpu_decode_status *)p[4], (ft8gpu_osd_info *)p[5], n, mc, order,
                           max_hard_errors, c->stream));
        return 0;
    });
}

int ft8gpu_decode_messages_deep(ft8gpu_ctx *c, const float *iq, int nframes, const ft8gpu_deep_params *params,
                                ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags) {
    CHECK_COMMON(c, nframes);
    if (!params) return ft8_fail("params is NULL");
    const int passes = params->passes, order = params->osd_order;
    if (passes < 1 || passes > FT8GPU_MAX_PASSES) return ft8_fail("passes %d out of range [1, %d]", passes, FT8GPU_MAX_PASSES);
    if (order < -1 || order > kOsdMaxOrder) return ft8_fail("osd_order %d out of range [-1, %d]", order, kOsdMaxOrder);
    if (order >= 0 && check_osd_args(order, params->osd_max_hard_errors)) return -1;
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    if (ensure_multipass_buffers(c)) return -1;
    if (order >= 0 && ensure_osd_buffers(c)) return -1;
    Rescue osd;
    if (order >= 0) osd = [=](const Chunk &k, const PassSet &f, int col) { return osd_step(k, f, col, order, params->osd_max_hard_errors); };
    return decode_messages_masked(c, iq, nframes, passes, 2, msgs, n_msgs, n_by_stage, flags, osd);
}

}  // extern "C"
