// api_multipass.hip -- host side of multi-pass decoding: the lazily allocated buffers, the pass loop of
// ft8gpu_decode_messages_passes, and the stage entries ft8gpu_mask_messages / ft8gpu_append_messages (DESIGN.md
// "Multi-pass decoding").
#include "ft8gpu_ctx.h"

// the compact waterfall, the map, the counts before a pass and a candidate / status set of the context's cap, on the first
// multi-pass call (ft8gpu_create's footprint is unchanged); the candidate set follows the cap when ft8gpu_set_params grows it
int ensure_multipass_buffers(ft8gpu_ctx *c) {
    if (ensure_messages_buffers(c)) return -1;
    const size_t mf = (size_t)c->max_frames;
    if (!c->d_mag2) HIP_TRY(hipMalloc(&c->d_mag2, mf * kMagArray));
    if (!c->d_map) HIP_TRY(hipMalloc(&c->d_map, mf * sizeof(int32_t)));
    if (!c->d_nprev) HIP_TRY(hipMalloc(&c->d_nprev, mf * sizeof(int32_t)));
    if (!c->d_nactive) HIP_TRY(hipMalloc(&c->d_nactive, sizeof(int32_t)));
    if (!c->h_nactive) HIP_TRY(hipHostMalloc(&c->h_nactive, sizeof(int32_t)));
    if (!c->d_counts2) HIP_TRY(hipMalloc(&c->d_counts2, mf * sizeof(int32_t)));
    if (c->cap2 < c->cap_candidates) {
        HIP_TRY(hipStreamSynchronize(c->stream));                   // the old set may still be in use
        if (c->d_cands2) (void)hipFree(c->d_cands2);
        if (c->d_status2) (void)hipFree(c->d_status2);
        c->d_cands2 = nullptr;
        c->d_status2 = nullptr;
        c->cap2 = 0;
        HIP_TRY(hipMalloc(&c->d_cands2, mf * c->cap_candidates * sizeof(ft8gpu_candidate)));
        HIP_TRY(hipMalloc(&c->d_status2, mf * c->cap_candidates * sizeof(ft8gpu_decode_status)));
        c->cap2 = c->cap_candidates;
    }
    return 0;
}

namespace {

// passes 2.. on one chunk of n frames already through pass 1 (run_pipeline_messages): c->d_mag holds W1, c->d_base its
// baseline, msgs / n_msgs the records so far.  nbp (nullable): [n][passes].
int run_later_passes(ft8gpu_ctx *c, int n, int passes, ft8gpu_message *msgs, int32_t *n_msgs, int32_t *nbp) {
    const ft8gpu_params &p = c->params;
    const int mc = p.max_candidates;
    if (nbp) HIP_TRY(launch_pass_counts(n_msgs, nbp, n, passes, 0, c->stream));
    if (passes < 2) return 0;
    HIP_TRY(hipMemsetAsync(c->d_nprev, 0, (size_t)n * sizeof(int32_t), c->stream));   // counts before pass 1
    for (int pass = 2; pass <= passes; ++pass) {
        // the frames that gained records in the last pass, compacted, their waterfall masked with every record so far
        HIP_TRY(launch_mask(c->d_mag, c->d_base, msgs, c->d_nprev, n_msgs, c->d_msgtab, n, 1, c->d_mag2, c->d_map, c->d_nactive, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_nprev, n_msgs, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_nactive, c->d_nactive, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                   // the one host read of the pass
        const int na = *c->h_nactive;
        if (na <= 0) break;                                         // nothing changes any more; nbp already holds the counts
        HIP_TRY(launch_sync(c->d_mag2, c->d_lists, c->d_list_counts, nullptr, na, p.min_score, c->stream));
        HIP_TRY(launch_heap(c->d_lists, c->d_list_counts, c->d_cands2, c->d_counts2, na, mc, c->debug_flags, c->stream));
        HIP_TRY(launch_decode(c->d_mag2, c->d_cands2, c->d_counts2, c->d_status2, na, mc, p.ldpc_iters, false, force_ieee(c), c->stream));
        HIP_TRY(launch_append(c->d_mag2, c->d_base, c->d_cands2, c->d_counts2, c->d_status2, c->d_msgtab, c->d_map, na, mc, p.min_score,
                              msgs, n_msgs, c->stream));
        if (nbp) HIP_TRY(launch_pass_counts(n_msgs, nbp, n, passes, pass - 1, c->stream));
    }
    return 0;
}

}  // namespace

void free_multipass_buffers(ft8gpu_ctx *c) {
    void *bufs[] = { c->d_mag2, c->d_map, c->d_nprev, c->d_nactive, c->d_cands2, c->d_counts2, c->d_status2, c->d_nbp };
    for (void *b : bufs) if (b) (void)hipFree(b);
    if (c->h_nactive) (void)hipHostFree(c->h_nactive);
}

extern "C" {

int ft8gpu_decode_messages_passes(ft8gpu_ctx *c, const float *iq, int nframes, int passes, ft8gpu_message *msgs,
                                  int32_t *n_msgs, int32_t *n_by_pass, int flags) {
    CHECK_COMMON(c, nframes);
    if (passes < 1 || passes > FT8GPU_MAX_PASSES) return ft8_fail("passes %d out of range [1, %d]", passes, FT8GPU_MAX_PASSES);
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    if (ensure_multipass_buffers(c)) return -1;
    flags &= FT8GPU_DEVICE_PTRS;
    if (!flags) {
        const size_t mf = (size_t)c->max_frames;
        if (!c->d_iq) HIP_TRY(hipMalloc(&c->d_iq, mf * 2 * kNSamples * sizeof(float)));
        if (!c->d_msgs) HIP_TRY(hipMalloc(&c->d_msgs, mf * kMaxMessages * sizeof(ft8gpu_message)));
        if (n_by_pass && !c->d_nbp) HIP_TRY(hipMalloc(&c->d_nbp, mf * FT8GPU_MAX_PASSES * sizeof(int32_t)));
    }
    // slots past a frame's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { iq, c->d_iq, 2 * (size_t)kNSamples * sizeof(float), kIn },
                           { msgs, c->d_msgs, kMaxMessages * sizeof(ft8gpu_message), kInOut },
                           { n_msgs, c->d_nres, sizeof(int32_t), kOut },
                           { n_by_pass, c->d_nbp, (size_t)passes * sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        if (run_pipeline_messages(c, (const float *)p[0], n, (ft8gpu_message *)p[1], (int32_t *)p[2])) return -1;
        return run_later_passes(c, n, passes, (ft8gpu_message *)p[1], (int32_t *)p[2], (int32_t *)p[3]);
    });
}

int ft8gpu_mask_messages(ft8gpu_ctx *c, const uint8_t *mag, const uint8_t *base, const ft8gpu_message *msgs,
                         const int32_t *first, const int32_t *n_msgs, int nframes, uint8_t *mag_out, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !base || !msgs || !first || !n_msgs || !mag_out) return ft8_fail("NULL array argument");
    if (ensure_multipass_buffers(c)) return -1;
    flags &= FT8GPU_DEVICE_PTRS;
    if (!flags && !c->d_msgs) HIP_TRY(hipMalloc(&c->d_msgs, (size_t)c->max_frames * kMaxMessages * sizeof(ft8gpu_message)));
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { base, c->d_base, 2 * kNumBin, kIn },
                           { msgs, c->d_msgs, kMaxMessages * sizeof(ft8gpu_message), kIn }, { first, c->d_nprev, sizeof(int32_t), kIn },
                           { n_msgs, c->d_nres, sizeof(int32_t), kIn }, { mag_out, c->d_mag2, kMagArray, kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_mask((const uint8_t *)p[0], (const uint8_t *)p[1], (const ft8gpu_message *)p[2], (const int32_t *)p[3],
                            (const int32_t *)p[4], c->d_msgtab, n, 0, (uint8_t *)p[5], nullptr, nullptr, c->stream));
        return 0;
    });
}

int ft8gpu_append_messages(ft8gpu_ctx *c, const uint8_t *mag, const uint8_t *base, const ft8gpu_candidate *cands,
                           const int32_t *counts, const ft8gpu_decode_status *status, int nframes, ft8gpu_message *msgs,
                           int32_t *n_msgs, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !base || !cands || !counts || !status || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    if (ensure_multipass_buffers(c)) return -1;
    flags &= FT8GPU_DEVICE_PTRS;
    if (!flags && !c->d_msgs) HIP_TRY(hipMalloc(&c->d_msgs, (size_t)c->max_frames * kMaxMessages * sizeof(ft8gpu_message)));
    const int mc = c->params.max_candidates;
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { base, c->d_base, 2 * kNumBin, kIn },
                           { cands, c->d_cands2, mc * sizeof(ft8gpu_candidate), kIn }, { counts, c->d_counts2, sizeof(int32_t), kIn },
                           { status, c->d_status2, mc * sizeof(ft8gpu_decode_status), kIn },
                           { msgs, c->d_msgs, kMaxMessages * sizeof(ft8gpu_message), kInOut }, { n_msgs, c->d_nres, sizeof(int32_t), kInOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_append((const uint8_t *)p[0], (const uint8_t *)p[1], (const ft8gpu_candidate *)p[2], (const int32_t *)p[3],
                              (const ft8gpu_decode_status *)p[4], c->d_msgtab, nullptr, n, mc, c->params.min_score, (ft8gpu_message *)p[5],
                              (int32_t *)p[6], c->stream));
        return 0;
    });
}

}  // extern "C"
