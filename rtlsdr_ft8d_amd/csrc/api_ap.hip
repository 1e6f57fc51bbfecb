// api_ap.hip -- host side of a-priori decoding: the lazily allocated buffers, the stage entry ft8gpu_ap_candidates and the
// pass loop of ft8gpu_decode_messages_ap (DESIGN.md "A-priori decoding").
#include "ft8gpu_ctx.h"

namespace {

constexpr int kApMaxHard = kLdpcN, kOsdMaxOrder = 2;

// the constant tables, the info records and the host form's staging of status_out, on the first AP call
// (ft8gpu_create's footprint is unchanged); the record buffers follow the cap when ft8gpu_set_params grows it
int ensure_ap_buffers(ft8gpu_ctx *c) {
    if (!c->ap_tables) {
        HIP_TRY(ap_tables_init(c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->ap_tables = true;
    }
    const size_t mf = (size_t)c->max_frames;
    if (!c->d_nap) HIP_TRY(hipMalloc(&c->d_nap, mf * sizeof(int32_t)));
    if (c->ap_cap < c->cap_candidates) {
        HIP_TRY(hipStreamSynchronize(c->stream));                   // the old set may still be in use
        if (c->d_ap_info) (void)hipFree(c->d_ap_info);
        if (c->d_ap_out) (void)hipFree(c->d_ap_out);
        c->d_ap_info = nullptr;
        c->d_ap_out = nullptr;
        c->ap_cap = 0;
        HIP_TRY(hipMalloc(&c->d_ap_info, mf * c->cap_candidates * sizeof(ft8gpu_ap_info)));
        HIP_TRY(hipMalloc(&c->d_ap_out, mf * c->cap_candidates * sizeof(ft8gpu_decode_status)));
        c->ap_cap = c->cap_candidates;
    }
    return 0;
}

int popcount8(unsigned v) { int n = 0; for (; v; v &= v - 1) ++n; return n; }

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

struct ApDeep {
    ft8gpu_ctx *c;
    int n;
    const ft8gpu_ap_params *q;
    ft8gpu_message *msgs;
    int32_t *n_msgs, *nbs;

    // nbs[f][col..] = n_msgs[f]: the count after a stage, carried into the stages that may not run
    int counts_to(int col) const {
        if (nbs) HIP_TRY(launch_pass_counts(n_msgs, nbs, n, 3 * q->passes, col, c->stream));
        return 0;
    }
    // AP, then OSD, on a pass's failures, in place; each followed by the append step and the tags of what it gained
    int stages(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts, ft8gpu_decode_status *status,
               const int32_t *map, int nslots, int col) const {
        const ft8gpu_params &p = c->params;
        const int mc = p.max_candidates;
        if (counts_to(col)) return -1;
        if (q->nhyp > 0) {
            HIP_TRY(hipMemcpyAsync(c->d_nap, n_msgs, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(launch_ap(mag, cands, counts, status, status, c->d_ap_info, nslots, mc, p.ldpc_iters, force_ieee(c), q->hyps,
                              q->nhyp, q->ap_max_hard_errors, c->stream));
            HIP_TRY(launch_append(mag, c->d_base, cands, counts, status, c->d_msgtab, map, nslots, mc, p.min_score, msgs, n_msgs, c->stream));
            HIP_TRY(launch_ap_tag(c->d_ap_info, map, c->d_nap, n_msgs, nslots, mc, msgs, c->stream));
            if (counts_to(col + 1)) return -1;
        }
        if (q->osd_order >= 0) {
            HIP_TRY(hipMemcpyAsync(c->d_nosd, n_msgs, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(launch_osd(mag, cands, counts, status, status, c->d_osd_info, nslots, mc, q->osd_order, q->osd_max_hard_errors, c->stream));
            HIP_TRY(launch_append(mag, c->d_base, cands, counts, status, c->d_msgtab, map, nslots, mc, p.min_score, msgs, n_msgs, c->stream));
            HIP_TRY(launch_osd_tag(c->d_osd_info, map, c->d_nosd, n_msgs, nslots, mc, msgs, c->stream));
        }
        return counts_to(col + 2);
    }
    // one chunk already through pass 1 (run_pipeline_messages): the pass loop of api_osd.hip with AP in front of OSD
    int run() const {
        const ft8gpu_params &p = c->params;
        const int mc = p.max_candidates, passes = q->passes;
        if (stages(c->d_mag, c->d_cands, c->d_counts, c->d_status, nullptr, n, 0)) return -1;
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
            if (stages(c->d_mag2, c->d_cands2, c->d_counts2, c->d_status2, c->d_map, na, 3 * (pass - 1))) return -1;
        }
        return 0;
    }
};

}  // namespace

void free_ap_buffers(ft8gpu_ctx *c) {
    void *bufs[] = { c->d_ap_info, c->d_ap_out, c->d_nap, c->d_nbs3 };
    for (void *b : bufs) if (b) (void)hipFree(b);
}

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
    // records at and behind a frame's count keep the caller's bytes (both outputs are uploaded in the host form)
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kIn },
                           { counts, c->d_counts, sizeof(int32_t), kIn },
                           { status_in, c->d_status, mc * sizeof(ft8gpu_decode_status), kIn },
                           { status_out, c->d_ap_out, mc * sizeof(ft8gpu_decode_status), kInOut },
                           { info, c->d_ap_info, mc * sizeof(ft8gpu_ap_info), kInOut } };
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
    flags &= FT8GPU_DEVICE_PTRS;
    if (!flags) {
        const size_t mf = (size_t)c->max_frames;
        if (!c->d_iq) HIP_TRY(hipMalloc(&c->d_iq, mf * 2 * kNSamples * sizeof(float)));
        if (!c->d_msgs) HIP_TRY(hipMalloc(&c->d_msgs, mf * kMaxMessages * sizeof(ft8gpu_message)));
        if (n_by_stage && !c->d_nbs3) HIP_TRY(hipMalloc(&c->d_nbs3, mf * FT8GPU_MAX_PASSES * 3 * sizeof(int32_t)));
    }
    // slots past a frame's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { iq, c->d_iq, 2 * (size_t)kNSamples * sizeof(float), kIn },
                           { msgs, c->d_msgs, kMaxMessages * sizeof(ft8gpu_message), kInOut },
                           { n_msgs, c->d_nres, sizeof(int32_t), kOut },
                           { n_by_stage, c->d_nbs3, (size_t)passes * 3 * sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        if (run_pipeline_messages(c, (const float *)p[0], n, (ft8gpu_message *)p[1], (int32_t *)p[2])) return -1;
        const ApDeep d{ c, n, params, (ft8gpu_message *)p[1], (int32_t *)p[2], (int32_t *)p[3] };
        return d.run();
    });
}

}  // extern "C"
