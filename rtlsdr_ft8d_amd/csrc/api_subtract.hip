// api_subtract.hip -- host side of the subtraction in the I/Q samples: the stage entry ft8gpu_subtract_messages and the pass loop
// of ft8gpu_decode_messages_subtracted (DESIGN.md "Subtraction in the I/Q samples"; the kernels are subtract.hip, the tables plain
// C in ft8_subtract.c).
//
// Both entries cut the frames with for_each_chunk.  Everything here is allocated on the first subtraction call, so
// ft8gpu_create's footprint is unchanged.  The estimate kernel leaves 10 240 bytes per record for the apply kernel; a chunk is
// therefore worked off in pieces of kSubFrames frames (estimate, apply, estimate, apply, ...), which bounds that buffer at 131 MB.
// The shaped entries take the reference's shape (include/ft8gpu.h "GFSK reference"); the two older entries are their shape 0.
// The GFSK tables come from the synthesiser's host helpers on the first call with that shape.
#include "subtract.h"
#include "refine.h"
#include "ft8gpu_ctx.h"

extern "C" void ft8_subtract_inv_table(float *inv);

namespace {

constexpr size_t kFrameFloats = 2 * (size_t)kNSamples;
constexpr size_t kFrameBytes = kFrameFloats * sizeof(float);
constexpr size_t kMsgBytes = kMaxMessages * sizeof(ft8gpu_message);
constexpr size_t kRefBytes = kMaxMessages * sizeof(ft8gpu_refined);
constexpr size_t kInfoBytes = kMaxMessages * sizeof(ft8gpu_subtract_info);
constexpr int kSubFrames = 256;

// host: the staging buffers of the host form (the device form needs the tables and the scratch only); work: the frame buffer
// the pass loop subtracts in
int ensure_subtract_buffers(ft8gpu_ctx *c, int shape, bool host, bool work, bool info) {
    if (ensure_messages_buffers(c)) return -1;
    const size_t mf = (size_t)c->max_frames;
    if (ensure_subtract_tables(c)) return -1;
    CtxMem &m = c->mem;
    if (shape == FT8GPU_SUBTRACT_GFSK && m.table(&c->d_subgfsktab, "the GFSK reference's tables", [](SubGfskTables *h) {
            return ft8gpu_gfsk_pulse(FT8GPU_GFSK_SPS_IQ, h->q) || ft8gpu_gfsk_ramp(FT8GPU_GFSK_SPS_IQ, h->ramp) ? ft8_fail("the GFSK tables") : 0;
        }))
        return -1;
    c->sub_frames = c->max_frames < kSubFrames ? c->max_frames : kSubFrames;
    if (m.once(&c->d_sub_scratch, (size_t)c->sub_frames * kMaxMessages * kSubStride * sizeof(uint32_t), "the subtraction's scratch")) return -1;
    if ((host || work) && (m.once(&c->d_sub_x, mf * kFrameBytes, "the frames being subtracted from") ||
                           m.once(&c->d_sub_ref, mf * kRefBytes, "the refined records")))
        return -1;
    if (work && m.once(&c->d_sub_nref, mf * sizeof(int32_t), "the counts a pass subtracts")) return -1;
    if (host && ensure_host_staging(c)) return -1;
    if (host && info && m.once(&c->d_sub_info, mf * kInfoBytes, "staging of the subtraction's info records")) return -1;
    return 0;
}

// out[f] = x[f] minus the records [first[f], n_msgs[f]) for the n frames of a chunk (device pointers; out may be x)
int subtract_chunk(ft8gpu_ctx *c, const float *x, const ft8gpu_message *msgs, const ft8gpu_refined *refined, const int32_t *first,
                   const int32_t *n_msgs, int n, float *out, ft8gpu_subtract_info *info, int shape) {
    for (int g0 = 0; g0 < n; g0 += c->sub_frames) {
        const int m = n - g0 < c->sub_frames ? n - g0 : c->sub_frames;
        const size_t r0 = (size_t)g0 * kMaxMessages;
        HIP_TRY(launch_subtract_estimate(x + g0 * kFrameFloats, msgs + r0, refined + r0, first + g0, n_msgs + g0, m, shape, c->d_subtab,
                                         c->d_subgfsktab, c->d_msgtab, c->d_sub_scratch, info ? info + r0 : nullptr, c->stream));
        HIP_TRY(launch_subtract_apply(x + g0 * kFrameFloats, out + g0 * kFrameFloats, first + g0, n_msgs + g0, m, shape, c->d_subtab,
                                      c->d_subgfsktab, c->d_sub_scratch, c->stream));
    }
    return 0;
}

// passes 2.. on one chunk of n frames already through pass 1 (run_pipeline_messages on iq): c->d_base holds the pass-1 baseline,
// msgs / n_msgs the records so far.  nbp (nullable): [n][passes].  work: [n] frames that end up holding every frame's last x_p;
// *used says whether anything was written to it.  shape: the reference the records are subtracted with.
int run_subtracted_passes(ft8gpu_ctx *c, const float *iq, int n, int passes, int shape, ft8gpu_message *msgs, int32_t *n_msgs,
                          int32_t *nbp, float *work, bool *used) {
    const ft8gpu_params &p = c->params;
    const int mc = p.max_candidates;
    *used = false;
    if (nbp) HIP_TRY(launch_pass_counts(n_msgs, nbp, n, passes, 0, c->stream));
    if (passes < 2) return 0;
    HIP_TRY(hipMemsetAsync(c->d_nprev, 0, (size_t)n * sizeof(int32_t), c->stream));   // counts before pass 1
    const float *x = iq;
    for (int pass = 2; pass <= passes; ++pass) {
        // the frames that gained records in the last pass and have room for more; d_sub_nref: their counts, 0 for the others
        HIP_TRY(launch_subtract_active(c->d_nprev, n_msgs, n, c->d_sub_nref, c->d_nactive, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_nactive, c->d_nactive, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                   // the one host read of the pass
        if (*c->h_nactive <= 0) break;                              // nothing changes any more; nbp already holds the counts
        // x_(p+1) = x_p minus the records first written in pass p, located on x_p
        HIP_TRY(launch_refine(x, msgs, c->d_sub_nref, n, c->d_tab, c->d_msgtab, c->d_sub_ref, c->stream));
        if (subtract_chunk(c, x, msgs, c->d_sub_ref, c->d_nprev, c->d_sub_nref, n, work, nullptr, shape)) return -1;
        x = work;
        *used = true;
        HIP_TRY(hipMemcpyAsync(c->d_nprev, n_msgs, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(launch_waterfall(work, c->d_mag2, c->d_tab, n, c->num_cus, c->debug_flags, c->stream));
        HIP_TRY(launch_sync(c->d_mag2, c->d_lists, c->d_list_counts, nullptr, n, p.min_score, c->stream));
        HIP_TRY(launch_heap(c->d_lists, c->d_list_counts, c->d_cands2, c->d_counts2, n, mc, c->debug_flags, c->stream));
        HIP_TRY(launch_subtract_gate(c->d_sub_nref, n, c->d_counts2, c->stream));      // the other frames are not decoded again
        HIP_TRY(launch_decode(c->d_mag2, c->d_cands2, c->d_counts2, c->d_status2, n, mc, p.ldpc_iters, false, force_ieee(c), c->stream));
        HIP_TRY(launch_append(c->d_mag2, c->d_base, c->d_cands2, c->d_counts2, c->d_status2, c->d_msgtab, nullptr, n, mc, p.min_score,
                              msgs, n_msgs, c->stream));
        if (nbp) HIP_TRY(launch_pass_counts(n_msgs, nbp, n, passes, pass - 1, c->stream));
    }
    return 0;
}

int bad_shape(int shape) {
    if (shape == FT8GPU_SUBTRACT_CPFSK || shape == FT8GPU_SUBTRACT_GFSK) return 0;
    return ft8_fail("shape %d is neither FT8GPU_SUBTRACT_CPFSK (0) nor FT8GPU_SUBTRACT_GFSK (1)", shape);
}

}  // namespace

// the constant tables (w4, inv), on the first call that needs them; api_demod.hip reads w4 too
int ensure_subtract_tables(ft8gpu_ctx *c) {
    return c->mem.table(&c->d_subtab, "the subtraction tables", [](SubTables *h) {
        ft8gpu_subtract_twiddles(&h->w4[0].x);
        ft8_subtract_inv_table(h->inv);
        return 0;
    });
}

extern "C" {

int ft8gpu_subtract_messages_shaped(ft8gpu_ctx *c, const float *iq, const ft8gpu_message *msgs, const ft8gpu_refined *refined,
                                    const int32_t *first, const int32_t *n_msgs, int nframes, float *iq_out,
                                    ft8gpu_subtract_info *info, int shape, int flags) {
    CHECK_COMMON(c, nframes);
    if (bad_shape(shape)) return -1;
    if (nframes == 0) return 0;
    if (!iq || !msgs || !refined || !first || !n_msgs || !iq_out) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)iq | (uintptr_t)iq_out) & 15) != 0) return ft8_fail("iq and iq_out must be 16-byte aligned");
    if (ensure_multipass_buffers(c)) return -1;                     // d_nprev stages `first`
    if (ensure_subtract_buffers(c, shape, !dev, false, info != nullptr)) return -1;
    // info records outside [first, n_msgs) keep the caller's bytes, so info travels both ways
    const StageArg a[] = { { iq, c->d_iq, kFrameBytes, kIn }, { msgs, c->d_msgs, kMsgBytes, kIn }, { refined, c->d_sub_ref, kRefBytes, kIn },
                           { first, c->d_nprev, sizeof(int32_t), kIn }, { n_msgs, c->d_nres, sizeof(int32_t), kIn },
                           { iq_out, c->d_sub_x, kFrameBytes, kOut }, { info, c->d_sub_info, kInfoBytes, kInOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        return subtract_chunk(c, (const float *)p[0], (const ft8gpu_message *)p[1], (const ft8gpu_refined *)p[2], (const int32_t *)p[3],
                              (const int32_t *)p[4], n, (float *)p[5], (ft8gpu_subtract_info *)p[6], shape);
    });
}

int ft8gpu_subtract_messages(ft8gpu_ctx *c, const float *iq, const ft8gpu_message *msgs, const ft8gpu_refined *refined,
                             const int32_t *first, const int32_t *n_msgs, int nframes, float *iq_out,
                             ft8gpu_subtract_info *info, int flags) {
    return ft8gpu_subtract_messages_shaped(c, iq, msgs, refined, first, n_msgs, nframes, iq_out, info, FT8GPU_SUBTRACT_CPFSK, flags);
}

int ft8gpu_decode_messages_subtracted_shaped(ft8gpu_ctx *c, const float *iq, int nframes, int passes, ft8gpu_message *msgs,
                                             int32_t *n_msgs, int32_t *n_by_pass, float *residual, int shape, int flags) {
    CHECK_COMMON(c, nframes);
    if (bad_shape(shape)) return -1;
    if (passes < 1 || passes > FT8GPU_MAX_PASSES) return ft8_fail("passes %d out of range [1, %d]", passes, FT8GPU_MAX_PASSES);
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (residual == iq) return ft8_fail("residual must not be iq: the caller's frames are never written");
    if (dev && (((uintptr_t)iq | (uintptr_t)residual) & 15) != 0) return ft8_fail("iq and residual must be 16-byte aligned");
    if (ensure_multipass_buffers(c)) return -1;
    if (ensure_subtract_buffers(c, shape, !dev, true, false)) return -1;
    if (!dev && n_by_pass && ensure_counts_staging(c)) return -1;
    // slots past a frame's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { iq, c->d_iq, kFrameBytes, kIn }, { msgs, c->d_msgs, kMsgBytes, kInOut }, { n_msgs, c->d_nres, sizeof(int32_t), kOut },
                           { n_by_pass, c->d_nbs, (size_t)passes * sizeof(int32_t), kOut }, { residual, c->d_sub_x, kFrameBytes, kOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        const float *x = (const float *)p[0];
        float *work = p[4] ? (float *)p[4] : c->d_sub_x;            // the caller's residual is the frame buffer of the passes
        bool used = false;
        if (run_pipeline_messages(c, x, n, (ft8gpu_message *)p[1], (int32_t *)p[2])) return -1;
        if (run_subtracted_passes(c, x, n, passes, shape, (ft8gpu_message *)p[1], (int32_t *)p[2], (int32_t *)p[3], work, &used)) return -1;
        if (p[4] && !used) HIP_TRY(hipMemcpyAsync(work, x, (size_t)n * kFrameBytes, hipMemcpyDeviceToDevice, c->stream));
        return 0;
    });
}

int ft8gpu_decode_messages_subtracted(ft8gpu_ctx *c, const float *iq, int nframes, int passes, ft8gpu_message *msgs,
                                      int32_t *n_msgs, int32_t *n_by_pass, float *residual, int flags) {
    return ft8gpu_decode_messages_subtracted_shaped(c, iq, nframes, passes, msgs, n_msgs, n_by_pass, residual, FT8GPU_SUBTRACT_CPFSK, flags);
}

}  // extern "C"
