// api_multipass.hip -- host side of multi-pass decoding: the lazily allocated buffers, the masking whole path that
// ft8gpu_decode_messages_passes, _deep (api_osd.hip) and _ap (api_ap.hip) share, and the stage entries ft8gpu_mask_messages /
// ft8gpu_append_messages (DESIGN.md "Multi-pass decoding").
#include "ft8gpu_ctx.h"

// the compact waterfall, the map, the counts before a pass and a candidate / status set of the context's cap, on the first
// multi-pass call (ft8gpu_create's footprint is unchanged)
int ensure_multipass_buffers(ft8gpu_ctx *c) {
    if (ensure_messages_buffers(c)) return -1;
    const size_t mf = (size_t)c->max_frames;
    CtxMem &m = c->mem;
    if (m.once(&c->d_mag2, mf * kMagArray, "a later pass's waterfall") || m.once(&c->d_map, mf * sizeof(int32_t), "the slot map") ||
        m.once(&c->d_nprev, mf * sizeof(int32_t), "the counts before a pass") || m.once(&c->d_nactive, sizeof(int32_t), "the active count") ||
        m.once_pinned(&c->h_nactive, sizeof(int32_t), "the active count") || m.once(&c->d_counts2, mf * sizeof(int32_t), "a later pass's counts"))
        return -1;
    return follow_cap(c, &c->d_cands2, &c->d_status2, &c->cap2, "a later pass's candidates");
}

namespace {

// One chunk through run_pipeline_messages: c->d_mag holds W1, c->d_base its baseline, k.msgs / k.n_msgs the records so far.
// Column cols * (pass - 1) of k.nbs gets the count after the pass's belief propagation, `rescue` the columns behind it.
int run_masking_passes(const Chunk &k, const Rescue &rescue) {
    ft8gpu_ctx *c = k.c;
    const ft8gpu_params &p = c->params;
    const int n = k.n, mc = p.max_candidates;
    if (k.counts_to(0)) return -1;
    if (rescue && rescue(k, PassSet{ c->d_mag, c->d_cands, c->d_counts, c->d_status, nullptr, n }, 1)) return -1;
    if (k.passes < 2) return 0;
    HIP_TRY(hipMemsetAsync(c->d_nprev, 0, (size_t)n * sizeof(int32_t), c->stream));   // counts before pass 1
    for (int pass = 2; pass <= k.passes; ++pass) {
        // the frames that gained records in the last pass, compacted, their waterfall masked with every record so far
        HIP_TRY(launch_mask(c->d_mag, c->d_base, k.msgs, c->d_nprev, k.n_msgs, c->d_msgtab, n, 1, c->d_mag2, c->d_map, c->d_nactive, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_nprev, k.n_msgs, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_nactive, c->d_nactive, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                   // the one host read of the pass
        const int na = *c->h_nactive;
        if (na <= 0) break;                                         // nothing changes any more; k.nbs already holds the counts
        HIP_TRY(launch_sync(c->d_mag2, c->d_lists, c->d_list_counts, nullptr, na, p.min_score, c->stream));
        HIP_TRY(launch_heap(c->d_lists, c->d_list_counts, c->d_cands2, c->d_counts2, na, mc, c->debug_flags, c->stream));
        HIP_TRY(launch_decode(c->d_mag2, c->d_cands2, c->d_counts2, c->d_status2, na, mc, p.ldpc_iters, false, force_ieee(c), c->stream));
        HIP_TRY(launch_append(c->d_mag2, c->d_base, c->d_cands2, c->d_counts2, c->d_status2, c->d_msgtab, c->d_map, na, mc, p.min_score,
                              k.msgs, k.n_msgs, c->stream));
        const int col = k.cols * (pass - 1);
        if (k.counts_to(col)) return -1;
        if (rescue && rescue(k, PassSet{ c->d_mag2, c->d_cands2, c->d_counts2, c->d_status2, c->d_map, na }, col + 1)) return -1;
    }
    return 0;
}

}  // namespace

int decode_messages_masked(ft8gpu_ctx *c, const float *iq, int nframes, int passes, int cols, ft8gpu_message *msgs, int32_t *n_msgs,
                           int32_t *n_by_stage, int flags, const Rescue &rescue) {
    flags &= FT8GPU_DEVICE_PTRS;
    if (!flags && (ensure_host_staging(c) || (n_by_stage && ensure_counts_staging(c)))) return -1;
    // slots past a frame's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { iq, c->d_iq, 2 * (size_t)kNSamples * sizeof(float), kIn },
                           { msgs, c->d_msgs, kMaxMessages * sizeof(ft8gpu_message), kInOut },
                           { n_msgs, c->d_nres, sizeof(int32_t), kOut },
                           { n_by_stage, c->d_nbs, (size_t)passes * cols * sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        if (run_pipeline_messages(c, (const float *)p[0], n, (ft8gpu_message *)p[1], (int32_t *)p[2])) return -1;
        return run_masking_passes(Chunk{ c, n, passes, cols, (ft8gpu_message *)p[1], (int32_t *)p[2], (int32_t *)p[3] }, rescue);
    });
}

extern "C" {

int ft8gpu_decode_messages_passes(ft8gpu_ctx *c, const float *iq, int nframes, int passes, ft8gpu_message *msgs,
                                  int32_t *n_msgs, int32_t *n_by_pass, int flags) {
    CHECK_COMMON(c, nframes);
    if (passes < 1 || passes > FT8GPU_MAX_PASSES) return ft8_fail("passes %d out of range [1, %d]", passes, FT8GPU_MAX_PASSES);
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    if (ensure_multipass_buffers(c)) return -1;
    return decode_messages_masked(c, iq, nframes, passes, 1, msgs, n_msgs, n_by_pass, flags, nullptr);
}

int ft8gpu_mask_messages(ft8gpu_ctx *c, const uint8_t *mag, const uint8_t *base, const ft8gpu_message *msgs,
                         const int32_t *first, const int32_t *n_msgs, int nframes, uint8_t *mag_out, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !base || !msgs || !first || !n_msgs || !mag_out) return ft8_fail("NULL array argument");
    if (ensure_multipass_buffers(c)) return -1;
    flags &= FT8GPU_DEVICE_PTRS;
    if (!flags && ensure_msgs_staging(c)) return -1;
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
    if (!flags && ensure_msgs_staging(c)) return -1;
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
