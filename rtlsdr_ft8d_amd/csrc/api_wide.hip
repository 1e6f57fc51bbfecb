// api_wide.hip -- host side of the wideband RX front end: the stage entry ft8gpu_wide_frames and the whole path ft8gpu_decode_wide
// (DESIGN.md "Wideband RX"; the kernels are wide.hip, the tables plain C in ft8_wide.c).
//
// Both entries cut the captures with for_each_chunk.  A chunk's captures go through the planes kernel in runs of at most
// kPlaneRun planes (capture, channel), so the 19 200 sps planes take 148 MB at most; a run's frames g = capture * nchannels +
// channel are then worked off in pieces of at most max_frames through one frame buffer.  Everything here is allocated on the
// first wide call that needs it, so ft8gpu_create's footprint is unchanged.
#include "wide.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr size_t kFrameFloats = 2 * (size_t)kNSamples;
constexpr size_t kFrameBytes = kFrameFloats * sizeof(float);
constexpr size_t kChanMsgBytes = kMaxMessages * sizeof(ft8gpu_message);
constexpr int kPlaneRun = 64;                               // planes in flight between the two stages

int ensure_wide_tables(ft8gpu_ctx *c) {
    return c->mem.table(&c->d_widetab, "the wideband RX tables", [](WideTables *h) {
        ft8gpu_wide_mixer1(h->w1);
        ft8gpu_wide_mixer2(&h->w2[0].x);
        ft8gpu_wide_taps(h->h);
        return 0;
    });
}

// a buffer of the wide path at `need` bytes or more; the stream is drained first if the old block has to go
template <class T> int wide_grow(ft8gpu_ctx *c, T **field, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return c->mem.grow(field, cap, need, what);
}

int wide_iq(ft8gpu_ctx *c) { return c->mem.once(&c->d_wide_iq, (size_t)c->max_frames * kFrameBytes, "the wideband RX frames"); }

// the refusals of both entries, before anything is enqueued
int check_wide_args(size_t npairs, const int32_t *freq_bin, int nchannels, WideChannels *ch) {
    if (nchannels < 1 || nchannels > FT8GPU_WIDE_MAX_CHANNELS)
        return ft8_fail("nchannels %d out of range [1, %d]", nchannels, FT8GPU_WIDE_MAX_CHANNELS);
    if (!freq_bin) return ft8_fail("NULL array argument");
    if (npairs == 0 || npairs % 8 != 0 || npairs > FT8GPU_WIDE_MAX_PAIRS)
        return ft8_fail("npairs %zu is not a positive multiple of 8 up to %d", npairs, FT8GPU_WIDE_MAX_PAIRS);
    *ch = WideChannels{};
    ch->n = nchannels;
    for (int b = 0; b < nchannels; ++b) {
        if (freq_bin[b] < -FT8GPU_WIDE_MAX_BIN || freq_bin[b] > FT8GPU_WIDE_MAX_BIN)
            return ft8_fail("freq_bin[%d] = %d out of range [%d, %d]", b, (int)freq_bin[b], -FT8GPU_WIDE_MAX_BIN, FT8GPU_WIDE_MAX_BIN);
        const int f = freq_bin[b] + 128;
        const int cc = (f + 32 + 64 * 4096) / 64 - 4096;     // floor((F + 32) / 64)
        const int q = f - 64 * cc;                           // in [-32, 31]
        ch->c[b] = (int16_t)(((cc % FT8GPU_WIDE_MIX1) + FT8GPU_WIDE_MIX1) % FT8GPU_WIDE_MIX1);
        ch->q[b] = (int16_t)((q + FT8GPU_WIDE_MIX2) % FT8GPU_WIDE_MIX2);
        ch->bin[b] = freq_bin[b];
    }
    return 0;
}

// The frames of a chunk of n captures: planes run by run, then each run's frames in pieces of at most `piece` frames through
// sink(g, m, planes of frame g), g counted from the chunk's first frame.
template <class Sink>
int wide_chunk(ft8gpu_ctx *c, const uint8_t *raw, int n, size_t npairs, const WideChannels &ch, int piece, Sink sink) {
    const int run = kPlaneRun / ch.n > 0 ? kPlaneRun / ch.n : 1;                 // captures per run
    float2 *planes = (float2 *)c->d_wide_planes;
    for (int c0 = 0; c0 < n; c0 += run) {
        const int nc = n - c0 < run ? n - c0 : run;
        HIP_TRY(launch_wide_planes(raw + (size_t)c0 * 2 * npairs, nc, npairs, ch, c->d_widetab, planes, c->stream));
        const int total = nc * ch.n;
        for (int g0 = 0; g0 < total; g0 += piece) {
            const int m = total - g0 < piece ? total - g0 : piece;
            if (sink(c0 * ch.n + g0, m, planes + (size_t)g0 * kWidePlaneLen)) return -1;
        }
    }
    return 0;
}

int wide_planes(ft8gpu_ctx *c, int ncaptures, int nchannels) {
    const int chunk = ncaptures < c->max_frames ? ncaptures : c->max_frames;
    const int run = kPlaneRun / nchannels > 0 ? kPlaneRun / nchannels : 1;
    const size_t planes = (size_t)(chunk < run ? chunk : run) * nchannels;
    return wide_grow(c, &c->d_wide_planes, &c->wide_planes_cap, planes * kWidePlaneBytes, "the wideband RX planes");
}

}  // namespace

extern "C" {

int ft8gpu_wide_frames(ft8gpu_ctx *c, const uint8_t *raw, int ncaptures, size_t npairs, const int32_t *freq_bin, int nchannels,
                       float *iq, int normalise, int flags) {
    CHECK_COMMON(c, ncaptures);
    WideChannels ch;
    if (check_wide_args(npairs, freq_bin, nchannels, &ch)) return -1;
    if (ncaptures == 0) return 0;
    if (!raw || !iq) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)raw & 15) != 0) return ft8_fail("raw must be 16-byte aligned");
    if (dev && ((uintptr_t)iq & 15) != 0) return ft8_fail("iq must be 16-byte aligned");
    if (ensure_wide_tables(c) || wide_planes(c, ncaptures, nchannels)) return -1;
    const int chunk = ncaptures < c->max_frames ? ncaptures : c->max_frames;
    if (!dev && (wide_iq(c) || wide_grow(c, &c->d_wide_raw, &c->wide_raw_cap, (size_t)chunk * 2 * npairs, "staging of the captures")))
        return -1;
    const StageArg a[] = { { raw, c->d_wide_raw, 2 * npairs, kIn } };
    size_t done = 0;                                        // frames of the chunks before this one
    return for_each_chunk(c, ncaptures, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        float *user = iq + done * kFrameFloats;
        done += (size_t)n * nchannels;
        const int piece = dev ? n * nchannels : c->max_frames;
        return wide_chunk(c, (const uint8_t *)p[0], n, npairs, ch, piece, [&](int g, int m, const float2 *planes) {
            if (dev) {
                HIP_TRY(launch_wide_fir(planes, npairs, m, c->d_widetab, user + g * kFrameFloats, normalise, c->stream));
                return 0;
            }
            HIP_TRY(launch_wide_fir(planes, npairs, m, c->d_widetab, c->d_wide_iq, normalise, c->stream));
            HIP_TRY(hipMemcpyAsync(user + g * kFrameFloats, c->d_wide_iq, m * kFrameBytes, hipMemcpyDeviceToHost, c->stream));
            return 0;
        });
    });
}

int ft8gpu_decode_wide(ft8gpu_ctx *c, const uint8_t *raw, int ncaptures, size_t npairs, const int32_t *freq_bin, int nchannels,
                       ft8gpu_message *msgs, int32_t *n_msgs, int flags) {
    CHECK_COMMON(c, ncaptures);
    WideChannels ch;
    if (check_wide_args(npairs, freq_bin, nchannels, &ch)) return -1;
    if (ncaptures == 0) return 0;
    if (!raw || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)raw & 15) != 0) return ft8_fail("raw must be 16-byte aligned");
    if (ensure_messages_buffers(c)) return -1;
    if (ensure_wide_tables(c) || wide_planes(c, ncaptures, nchannels) || wide_iq(c)) return -1;
    const size_t chunk = (size_t)(ncaptures < c->max_frames ? ncaptures : c->max_frames);
    if (wide_grow(c, &c->d_wide_cmsgs, &c->wide_cmsgs_cap, chunk * nchannels * kChanMsgBytes, "the channels' records") ||
        wide_grow(c, &c->d_wide_cn, &c->wide_cn_cap, chunk * nchannels * sizeof(int32_t), "the channels' counts"))
        return -1;
    if (!dev && (wide_grow(c, &c->d_wide_raw, &c->wide_raw_cap, chunk * 2 * npairs, "staging of the captures") ||
                 wide_grow(c, &c->d_wide_msgs, &c->wide_msgs_cap, chunk * nchannels * kChanMsgBytes, "staging of the merged records")))
        return -1;
    // slots past a capture's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { raw, c->d_wide_raw, 2 * npairs, kIn },
                           { msgs, c->d_wide_msgs, (size_t)nchannels * kChanMsgBytes, kInOut }, { n_msgs, c->d_nres, sizeof(int32_t), kOut } };
    return for_each_chunk(c, ncaptures, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        if (wide_chunk(c, (const uint8_t *)p[0], n, npairs, ch, c->max_frames, [&](int g, int m, const float2 *planes) {
                HIP_TRY(launch_wide_fir(planes, npairs, m, c->d_widetab, c->d_wide_iq, 1, c->stream));
                return run_pipeline_messages(c, c->d_wide_iq, m, c->d_wide_cmsgs + (size_t)g * kMaxMessages, c->d_wide_cn + g);
            }))
            return -1;
        HIP_TRY(launch_wide_merge(c->d_wide_cmsgs, c->d_wide_cn, n, ch, (ft8gpu_message *)p[1], (int32_t *)p[2], c->stream));
        return 0;
    });
}

}  // extern "C"
