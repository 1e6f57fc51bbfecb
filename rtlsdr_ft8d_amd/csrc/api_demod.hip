// api_demod.hip -- host side of the demodulation from the I/Q samples: the stage entry ft8gpu_demod_candidates and the whole
// path ft8gpu_decode_messages_demod (DESIGN.md "Demodulation from the I/Q samples"; the kernels are demod.hip).
//
// Both entries cut the frames with for_each_chunk.  Everything beyond the messages path lives in the context's scratch
// blocks (ensure_scratch), which no other entry uses while this one holds the context's mutex: the info records (block 3), the
// host form's staging of status_out (2), the whole path's counts before the append step (0).  w4 is the subtraction's table.
#include "demod.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr size_t kFrameBytes = 2 * (size_t)kNSamples * sizeof(float);
constexpr size_t kMsgBytes = kMaxMessages * sizeof(ft8gpu_message);

int check_demod_args(const ft8gpu_ctx *c, const ft8gpu_demod_params *p) {
    if (!p) return ft8_fail("params is NULL");
    if (p->sets < 1 || p->sets > 7) return ft8_fail("sets %d out of range [1, 7]", p->sets);
    if (p->max_hard_errors < 0 || p->max_hard_errors > kLdpcN)
        return ft8_fail("max_hard_errors %d out of range [0, %d]", p->max_hard_errors, kLdpcN);
    if (p->max_per_frame < 0 || p->max_per_frame > c->params.max_candidates)
        return ft8_fail("max_per_frame %d out of range [0, %d]", p->max_per_frame, c->params.max_candidates);
    return 0;
}

// the kernels' constant tables, on the context's first call
int ensure_demod_tables(ft8gpu_ctx *c) {
    if (ensure_subtract_tables(c)) return -1;
    return tables_once(c, &c->demod_tables, demod_tables_init);
}

}  // namespace

extern "C" {

int ft8gpu_demod_candidates(ft8gpu_ctx *c, const float *iq, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_demod_params *params,
                            ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_demod_args(c, params)) return -1;
    if (nframes == 0) return 0;
    if (!iq || !cands || !counts || !status_in || !status_out || !info) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)iq & 15) != 0) return ft8_fail("iq must be 16-byte aligned");
    if (ensure_messages_buffers(c) || ensure_demod_tables(c)) return -1;
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (!dev && ensure_host_staging(c)) return -1;
    if (ensure_scratch(c, 0, 0, dev ? 0 : piece * mc * sizeof(ft8gpu_decode_status), dev ? 0 : piece * mc * sizeof(ft8gpu_demod_info)))
        return -1;
    const ft8gpu_demod_params p = *params;
    StageArg a[kCandRows];
    cand_stage_rows(a, c, { iq, c->d_iq, kFrameBytes, kIn }, cands, counts, status_in, status_out, c->d_scratch[2], info, c->d_scratch[3],
                    sizeof(ft8gpu_demod_info));
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *q) {
        HIP_TRY(launch_demod((const float *)q[0], (const ft8gpu_candidate *)q[1], (const int32_t *)q[2],
                             (const ft8gpu_decode_status *)q[3], (ft8gpu_decode_status *)q[4], (ft8gpu_demod_info *)q[5], n, mc,
                             c->d_subtab, p.sets, p.max_hard_errors, p.max_per_frame, c->params.ldpc_iters, force_ieee(c), c->stream));
        return 0;
    });
}

int ft8gpu_decode_messages_demod(ft8gpu_ctx *c, const float *iq, int nframes, const ft8gpu_demod_params *params,
                                 ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_demod_args(c, params)) return -1;
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)iq | (uintptr_t)msgs) & 15) != 0) return ft8_fail("iq and msgs must be 16-byte aligned");
    if (ensure_messages_buffers(c) || ensure_demod_tables(c)) return -1;
    if (!dev && (ensure_host_staging(c) || (n_by_stage && ensure_counts_staging(c)))) return -1;
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (ensure_scratch(c, piece * sizeof(int32_t), 0, 0, piece * mc * sizeof(ft8gpu_demod_info))) return -1;
    const ft8gpu_demod_params p = *params;
    // slots past a frame's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { iq, c->d_iq, kFrameBytes, kIn }, { msgs, c->d_msgs, kMsgBytes, kInOut },
                           { n_msgs, c->d_nres, sizeof(int32_t), kOut }, { n_by_stage, c->d_nbs, 2 * sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *q) {
        const float *x = (const float *)q[0];
        ft8gpu_message *dm = (ft8gpu_message *)q[1];
        int32_t *pn = (int32_t *)q[2], *pb = (int32_t *)q[3], *before = (int32_t *)c->d_scratch[0];
        ft8gpu_demod_info *inf = (ft8gpu_demod_info *)c->d_scratch[3];
        if (run_pipeline_messages(c, x, n, dm, pn)) return -1;
        if (pb) HIP_TRY(launch_pass_counts(pn, pb, n, 2, 0, c->stream));
        HIP_TRY(hipMemcpyAsync(before, pn, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(launch_demod(x, c->d_cands, c->d_counts, c->d_status, c->d_status, inf, n, mc, c->d_subtab, p.sets, p.max_hard_errors,
                             p.max_per_frame, c->params.ldpc_iters, force_ieee(c), c->stream));
        HIP_TRY(launch_append(c->d_mag, c->d_base, c->d_cands, c->d_counts, c->d_status, c->d_msgtab, nullptr, n, mc, c->params.min_score,
                              dm, pn, c->stream));
        HIP_TRY(launch_demod_tag(before, pn, n, inf, mc, dm, c->stream));
        if (pb) HIP_TRY(launch_pass_counts(pn, pb, n, 2, 1, c->stream));
        return 0;
    });
}

}  // extern "C"
