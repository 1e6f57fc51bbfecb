// api_osd.hip -- host side of ordered-statistics decoding: the lazily allocated buffers, the stage entry
// ft8gpu_osd_candidates and the pass loop of ft8gpu_decode_messages_deep (DESIGN.md "Ordered-statistics decoding").
#include "ft8gpu_ctx.h"

namespace {

constexpr int kOsdMaxOrder = 2, kOsdMaxHard = kLdpcM;

}  // namespace

// the constant tables, the info records and the host form's staging of status_out, on the first OSD call
// (ft8gpu_create's footprint is unchanged); the record buffers follow the cap when ft8gpu_set_params grows it
int ensure_osd_buffers(ft8gpu_ctx *c) {
    if (!c->osd_tables) {
        HIP_TRY(osd_tables_init(c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->osd_tables = true;
    }
    const size_t mf = (size_t)c->max_frames;
    if (!c->d_nosd) HIP_TRY(hipMalloc(&c->d_nosd, mf * sizeof(int32_t)));
    if (c->osd_cap < c->cap_candidates) {
        HIP_TRY(hipStreamSynchronize(c->stream));                   // the old set may still be in use
        if (c->d_osd_info) (void)hipFree(c->d_osd_info);
        if (c->d_osd_out) (void)hipFree(c->d_osd_out);
        c->d_osd_info = nullptr;
        c->d_osd_out = nullptr;
        c->osd_cap = 0;
        HIP_TRY(hipMalloc(&c->d_osd_info, mf * c->cap_candidates * sizeof(ft8gpu_osd_info)));
        HIP_TRY(hipMalloc(&c->d_osd_out, mf * c->cap_candidates * sizeof(ft8gpu_decode_status)));
        c->osd_cap = c->cap_candidates;
    }
    return 0;
}

int check_osd_args(int order, int max_hard_errors) {
    if (order < 0 || order > kOsdMaxOrder) return ft8_fail("order %d out of range [0, %d]", order, kOsdMaxOrder);
    if (max_hard_errors < 0 || max_hard_errors > kOsdMaxHard)
        return ft8_fail("max_hard_errors %d out of range [0, %d]", max_hard_errors, kOsdMaxHard);
    return 0;
}

namespace {

struct Deep {
    ft8gpu_ctx *c;
    int n, passes, order, max_hard;
    ft8gpu_message *msgs;
    int32_t *n_msgs, *nbs;

    // nbs[f][col..] = n_msgs[f]: the count after a stage, carried into the stages that may not run
    int counts_to(int col) const {
        if (nbs) HIP_TRY(launch_pass_counts(n_msgs, nbs, n, 2 * passes, col, c->stream));
        return 0;
    }
    // OSD on a pass's failures, in place, then the append step and the nhard tags of what it gained
    int osd(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts, ft8gpu_decode_status *status,
            const int32_t *map, int nslots) const {
        if (order < 0) return 0;
        const int mc = c->params.max_candidates;
        HIP_TRY(hipMemcpyAsync(c->d_nosd, n_msgs, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(launch_osd(mag, cands, counts, status, status, c->d_osd_info, nslots, mc, order, max_hard, c->stream));
        HIP_TRY(launch_append(mag, c->d_base, cands, counts, status, c->d_msgtab, map, nslots, mc, c->params.min_score, msgs, n_msgs, c->stream));
        HIP_TRY(launch_osd_tag(c->d_osd_info, map, c->d_nosd, n_msgs, nslots, mc, msgs, c->stream));
        return 0;
    }
    // one chunk already through pass 1 (run_pipeline_messages): the pass loop of api_multipass.hip with OSD behind every pass
    int run() const {
        const ft8gpu_params &p = c->params;
        const int mc = p.max_candidates;
        if (counts_to(0)) return -1;
        if (osd(c->d_mag, c->d_cands, c->d_counts, c->d_status, nullptr, n)) return -1;
        if (counts_to(1)) return -1;
        if (passes < 2) return 0;
        HIP_TRY(hipMemsetAsync(c->d_nprev, 0, (size_t)n * sizeof(int32_t), c->stream));
        for (int pass = 2; pass <= passes; ++pass) {
            HIP_TRY(launch_mask(c->d_mag, c->d_base, msgs, c->d_nprev, n_msgs, c->d_msgtab, n, 1, c->d_mag2, c->d_map, c->d_nactive, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_nprev, n_msgs, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->h_nactive, c->d_nactive, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            const int na = *c->h_nactive;
            if (na <= 0) break;
            HIP_TRY(launch_sync(c->d_mag2, c->d_lists, c->d_list_counts, nullptr, na, p.min_score, c->stream));
            HIP_TRY(launch_heap(c->d_lists, c->d_list_counts, c->d_cands2, c->d_counts2, na, mc, c->debug_flags, c->stream));
            HIP_TRY(launch_decode(c->d_mag2, c->d_cands2, c->d_counts2, c->d_status2, na, mc, p.ldpc_iters, false, force_ieee(c), c->stream));
            HIP_TRY(launch_append(c->d_mag2, c->d_base, c->d_cands2, c->d_counts2, c->d_status2, c->d_msgtab, c->d_map, na, mc, p.min_score,
                                  msgs, n_msgs, c->stream));
            if (counts_to(2 * (pass - 1))) return -1;
            if (osd(c->d_mag2, c->d_cands2, c->d_counts2, c->d_status2, c->d_map, na)) return -1;
            if (counts_to(2 * (pass - 1) + 1)) return -1;
        }
        return 0;
    }
};

}  // namespace

void free_osd_buffers(ft8gpu_ctx *c) {
    void *bufs[] = { c->d_osd_info, c->d_osd_out, c->d_nosd, c->d_nbs };
    for (void *b : bufs) if (b) (void)hipFree(b);
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
    // records at and behind a frame's count keep the caller's bytes (both outputs are uploaded in the host form)
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kIn },
                           { counts, c->d_counts, sizeof(int32_t), kIn },
                           { status_in, c->d_status, mc * sizeof(ft8gpu_decode_status), kIn },
                           { status_out, c->d_osd_out, mc * sizeof(ft8gpu_decode_status), kInOut },
                           { info, c->d_osd_info, mc * sizeof(ft8gpu_osd_info), kInOut } };
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
    flags &= FT8GPU_DEVICE_PTRS;
    if (!flags) {
        const size_t mf = (size_t)c->max_frames;
        if (!c->d_iq) HIP_TRY(hipMalloc(&c->d_iq, mf * 2 * kNSamples * sizeof(float)));
        if (!c->d_msgs) HIP_TRY(hipMalloc(&c->d_msgs, mf * kMaxMessages * sizeof(ft8gpu_message)));
        if (n_by_stage && !c->d_nbs) HIP_TRY(hipMalloc(&c->d_nbs, mf * FT8GPU_MAX_PASSES * 2 * sizeof(int32_t)));
    }
    // slots past a frame's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { iq, c->d_iq, 2 * (size_t)kNSamples * sizeof(float), kIn },
                           { msgs, c->d_msgs, kMaxMessages * sizeof(ft8gpu_message), kInOut },
                           { n_msgs, c->d_nres, sizeof(int32_t), kOut },
                           { n_by_stage, c->d_nbs, (size_t)passes * 2 * sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        if (run_pipeline_messages(c, (const float *)p[0], n, (ft8gpu_message *)p[1], (int32_t *)p[2])) return -1;
        const Deep d{ c, n, passes, order, params->osd_max_hard_errors, (ft8gpu_message *)p[1], (int32_t *)p[2], (int32_t *)p[3] };
        return d.run();
    });
}

}  // extern "C"
