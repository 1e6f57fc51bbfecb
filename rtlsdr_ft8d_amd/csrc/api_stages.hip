// api_stages.hip -- the same data stage by stage (used by the parity tests and by the ft8_lib-level symbols of
// ft8_compat.c): waterfall, sync search, candidate decode, spot collection.
#include "ft8gpu_ctx.h"

extern "C" {

int ft8gpu_waterfall(ft8gpu_ctx *c, const float *iq, int nframes, uint8_t *mag, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!iq || !mag) return ft8_fail("NULL array argument");
    const size_t frame_floats = 2 * (size_t)kNSamples;
    if (!(flags & FT8GPU_DEVICE_PTRS) && ensure_host_staging(c, false)) return -1;
    const StageArg a[] = { { iq, c->d_iq, frame_floats * sizeof(float), kIn }, { mag, c->d_mag, kMagArray, kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_waterfall((const float *)p[0], (uint8_t *)p[1], c->d_tab, n, c->num_cus, c->debug_flags, c->stream));
        return 0;
    });
}

int ft8gpu_find_sync(ft8gpu_ctx *c, const uint8_t *mag, int nframes, ft8gpu_candidate *cands, int32_t *counts, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts) return ft8_fail("NULL array argument");
    const int mc = c->params.max_candidates;
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kOut },
                           { counts, c->d_counts, sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_sync((const uint8_t *)p[0], c->d_lists, c->d_list_counts, nullptr, n, c->params.min_score, c->stream));
        HIP_TRY(launch_heap(c->d_lists, c->d_list_counts, (ft8gpu_candidate *)p[1], (int32_t *)p[2], n, mc, c->debug_flags, c->stream));
        return 0;
    });
}

int ft8gpu_score_map(ft8gpu_ctx *c, const uint8_t *mag, int nframes, int16_t *scores, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !scores) return ft8_fail("NULL array argument");
    if (!(flags & FT8GPU_DEVICE_PTRS) &&
        c->mem.once(&c->d_scores, (size_t)c->max_frames * kScoresPerFrame * sizeof(int16_t), "staging of the score map")) return -1;
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { scores, c->d_scores, kScoresPerFrame * sizeof(int16_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_sync((const uint8_t *)p[0], c->d_lists, c->d_list_counts, (int16_t *)p[1], n, c->params.min_score, c->stream));
        return 0;
    });
}

int ft8gpu_decode_candidates(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                             int nframes, ft8gpu_decode_status *status, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status) return ft8_fail("NULL array argument");
    const int mc = c->params.max_candidates;
    // the stage entry reports the exact ldpc_errors; FT8GPU_DBG_PIPELINE_FORM runs the form of the
    // kernel the batch pipeline uses instead (test hook: every field but ldpc_errors must agree)
    const bool count_errors = !(c->debug_flags & FT8GPU_DBG_PIPELINE_FORM);
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kIn },
                           { counts, c->d_counts, sizeof(int32_t), kIn },
                           { status, c->d_status, mc * sizeof(ft8gpu_decode_status), kOutZeroed } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_decode((const uint8_t *)p[0], (const ft8gpu_candidate *)p[1], (const int32_t *)p[2], (ft8gpu_decode_status *)p[3],
                              n, mc, c->params.ldpc_iters, count_errors, force_ieee(c), c->stream));
        return 0;
    });
}

int ft8gpu_collect_spots(ft8gpu_ctx *c, const ft8gpu_candidate *cands, const int32_t *counts,
                         const ft8gpu_decode_status *status, int nframes, struct decoder_results *decodes,
                         int32_t *n_results, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!cands || !counts || !status || !decodes || !n_results) return ft8_fail("NULL array argument");
    const int mc = c->params.max_candidates;
    // slots the kernel does not write keep the caller's bytes
    const StageArg a[] = { { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kIn }, { counts, c->d_counts, sizeof(int32_t), kIn },
                           { status, c->d_status, mc * sizeof(ft8gpu_decode_status), kIn },
                           { decodes, c->d_decodes, kMaxMessages * sizeof(struct decoder_results), kInOut },
                           { n_results, c->d_nres, sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_spots((const ft8gpu_candidate *)p[0], (const int32_t *)p[1], (const ft8gpu_decode_status *)p[2], n, mc,
                             c->params.min_score, (struct decoder_results *)p[3], (int32_t *)p[4], c->stream));
        return 0;
    });
}

}  // extern "C"
