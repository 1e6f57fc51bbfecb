// api_refine.hip -- host side of the refined time and frequency: the stage entry ft8gpu_refine_messages and the whole path
// ft8gpu_decode_messages_refined (DESIGN.md "Refined time and frequency"; the kernel is refine.hip, the estimate and the table
// are plain C in ft8_refine.c).
//
// Both entries cut the frames with for_each_chunk.  The host form stages the frames in the context's d_iq, the records in d_msgs,
// the counts in d_nres and the refined records in the context's scratch block 3 (ensure_scratch), which no other entry uses while
// this one holds the context's mutex.  Records at and behind a frame's count keep the caller's bytes, so msgs and refined travel both ways.
#include "refine.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr size_t kFrameBytes = 2 * (size_t)kNSamples * sizeof(float);
constexpr size_t kMsgBytes = kMaxMessages * sizeof(ft8gpu_message);
constexpr size_t kRefBytes = kMaxMessages * sizeof(ft8gpu_refined);

// the staging buffers of the host form (the device form needs the tables only)
int ensure_refine_buffers(ft8gpu_ctx *c, int nframes, bool dev) {
    if (ensure_messages_buffers(c)) return -1;
    if (dev) return 0;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    return ensure_host_staging(c) || ensure_scratch(c, 0, 0, 0, piece * kRefBytes) ? -1 : 0;
}

}  // namespace

extern "C" {

int ft8gpu_refine_messages(ft8gpu_ctx *c, const float *iq, const ft8gpu_message *msgs, const int32_t *n_msgs, int nframes,
                           ft8gpu_refined *refined, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs || !refined) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)iq & 15) != 0) return ft8_fail("iq must be 16-byte aligned");
    if (ensure_refine_buffers(c, nframes, dev)) return -1;
    const StageArg a[] = { { iq, c->d_iq, kFrameBytes, kIn }, { msgs, c->d_msgs, kMsgBytes, kIn },
                           { n_msgs, c->d_nres, sizeof(int32_t), kIn }, { refined, c->d_scratch[3], kRefBytes, kInOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        HIP_TRY(launch_refine((const float *)p[0], (const ft8gpu_message *)p[1], (const int32_t *)p[2], n, c->d_tab, c->d_msgtab,
                              (ft8gpu_refined *)p[3], c->stream));
        return 0;
    });
}

int ft8gpu_decode_messages_refined(ft8gpu_ctx *c, const float *iq, int nframes, ft8gpu_message *msgs, int32_t *n_msgs,
                                   ft8gpu_refined *refined, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs || !refined) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)iq & 15) != 0) return ft8_fail("iq must be 16-byte aligned");
    if (ensure_refine_buffers(c, nframes, dev)) return -1;
    const StageArg a[] = { { iq, c->d_iq, kFrameBytes, kIn }, { msgs, c->d_msgs, kMsgBytes, kInOut },
                           { n_msgs, c->d_nres, sizeof(int32_t), kOut }, { refined, c->d_scratch[3], kRefBytes, kInOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        if (run_pipeline_messages(c, (const float *)p[0], n, (ft8gpu_message *)p[1], (int32_t *)p[2])) return -1;
        HIP_TRY(launch_refine((const float *)p[0], (const ft8gpu_message *)p[1], (const int32_t *)p[2], n, c->d_tab, c->d_msgtab,
                              (ft8gpu_refined *)p[3], c->stream));
        return 0;
    });
}

}  // extern "C"
