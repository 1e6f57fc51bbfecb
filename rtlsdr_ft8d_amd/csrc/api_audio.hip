// api_audio.hip -- host side of the audio front end: the stage entry ft8gpu_audio_frames and the whole path ft8gpu_decode_audio
// (DESIGN.md "Audio front end"; the kernels are audio.hip, the tables plain C in ft8_subtract.c).
//
// Both entries cut the clips with for_each_chunk.  A clip gives bands.n frames, and the pipeline takes max_frames frames at a
// time, so a chunk's frames g = clip * bands.n + band are worked off in runs of at most max_frames through one frame buffer.
// Everything here is allocated on the first audio call, so ft8gpu_create's footprint is unchanged.
#include "audio.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr size_t kFrameFloats = 2 * (size_t)kNSamples;
constexpr size_t kFrameBytes = kFrameFloats * sizeof(float);

int ensure_audio_tables(ft8gpu_ctx *c) {
    return c->mem.table(&c->d_audiotab, "the audio tables", [](AudioTables *h) {
        ft8gpu_audio_taps(h->h);
        ft8gpu_audio_mixer(&h->wm[0].x);
        return 0;
    });
}

// the buffers of the audio front end, each on the first call that needs it
int audio_pcm(ft8gpu_ctx *c) { return c->mem.once(&c->d_audio_pcm, (size_t)c->max_frames * FT8GPU_AUDIO_NSAMPLES * sizeof(float), "staging of the clips"); }
int audio_iq(ft8gpu_ctx *c) { return c->mem.once(&c->d_audio_iq, (size_t)c->max_frames * kFrameBytes, "the audio front end's frames"); }

// the refusals of both entries, before anything is enqueued
int check_audio_args(int format, int nsamples, const int32_t *base_bin, int nbands, AudioBands *bands) {
    if (format != FT8GPU_AUDIO_S16 && format != FT8GPU_AUDIO_F32) return ft8_fail("unknown audio format %d", format);
    if (nsamples < 1 || nsamples > FT8GPU_AUDIO_NSAMPLES)
        return ft8_fail("nsamples %d out of range [1, %d]", nsamples, FT8GPU_AUDIO_NSAMPLES);
    if (nbands < 1 || nbands > FT8GPU_AUDIO_MAX_BANDS) return ft8_fail("nbands %d out of range [1, %d]", nbands, FT8GPU_AUDIO_MAX_BANDS);
    if (!base_bin) return ft8_fail("NULL array argument");
    bands->n = nbands;
    for (int b = 0; b < FT8GPU_AUDIO_MAX_BANDS; ++b) bands->base[b] = 0;
    for (int b = 0; b < nbands; ++b) {
        if (base_bin[b] < 0 || base_bin[b] > FT8GPU_AUDIO_MAX_BASE)
            return ft8_fail("base_bin[%d] = %d out of range [0, %d]", b, (int)base_bin[b], FT8GPU_AUDIO_MAX_BASE);
        bands->base[b] = base_bin[b];
    }
    return 0;
}

size_t sample_bytes(int format) { return format == FT8GPU_AUDIO_S16 ? sizeof(int16_t) : sizeof(float); }

}  // namespace

extern "C" {

int ft8gpu_audio_frames(ft8gpu_ctx *c, const void *pcm, int format, int nclips, int nsamples, const int32_t *base_bin, int nbands,
                        float *iq_out, int flags) {
    CHECK_COMMON(c, nclips);
    AudioBands bands;
    if (check_audio_args(format, nsamples, base_bin, nbands, &bands)) return -1;
    if (nclips == 0) return 0;
    if (!pcm || !iq_out) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)iq_out & 15) != 0) return ft8_fail("iq_out must be 16-byte aligned");
    if (ensure_audio_tables(c)) return -1;
    if (!dev && (audio_pcm(c) || audio_iq(c))) return -1;
    const StageArg a[] = { { pcm, c->d_audio_pcm, (size_t)nsamples * sample_bytes(format), kIn } };
    size_t done = 0;                                        // frames of the chunks before this one
    return for_each_chunk(c, nclips, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        const int total = n * nbands;
        float *user = iq_out + done * kFrameFloats;
        done += (size_t)total;
        if (dev) {
            HIP_TRY(launch_audio_frames(p[0], format, nsamples, bands, 0, total, c->d_audiotab, user, c->stream));
            return 0;
        }
        for (int g0 = 0; g0 < total; g0 += c->max_frames) {
            const int m = total - g0 < c->max_frames ? total - g0 : c->max_frames;
            HIP_TRY(launch_audio_frames(p[0], format, nsamples, bands, g0, g0 + m, c->d_audiotab, c->d_audio_iq, c->stream));
            HIP_TRY(hipMemcpyAsync(user + g0 * kFrameFloats, c->d_audio_iq, m * kFrameBytes, hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    });
}

int ft8gpu_decode_audio(ft8gpu_ctx *c, const void *pcm, int format, int nclips, int nsamples, const int32_t *base_bin, int nbands,
                        ft8gpu_message *msgs, int32_t *n_msgs, int flags) {
    CHECK_COMMON(c, nclips);
    AudioBands bands;
    if (check_audio_args(format, nsamples, base_bin, nbands, &bands)) return -1;
    if (nclips == 0) return 0;
    if (!pcm || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (ensure_messages_buffers(c)) return -1;
    if (ensure_audio_tables(c)) return -1;
    const size_t mf = (size_t)c->max_frames;
    constexpr size_t kBandMsgBytes = kMaxMessages * sizeof(ft8gpu_message);
    if (audio_iq(c) || c->mem.once(&c->d_audio_bmsgs, mf * FT8GPU_AUDIO_MAX_BANDS * kBandMsgBytes, "the bands' records") ||
        c->mem.once(&c->d_audio_bn, mf * FT8GPU_AUDIO_MAX_BANDS * sizeof(int32_t), "the bands' counts"))
        return -1;
    if (!dev && (audio_pcm(c) || c->mem.once(&c->d_audio_msgs, mf * FT8GPU_AUDIO_MAX_BANDS * kBandMsgBytes, "staging of the merged records")))
        return -1;
    // slots past a clip's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { pcm, c->d_audio_pcm, (size_t)nsamples * sample_bytes(format), kIn },
                           { msgs, c->d_audio_msgs, (size_t)nbands * kBandMsgBytes, kInOut }, { n_msgs, c->d_nres, sizeof(int32_t), kOut } };
    return for_each_chunk(c, nclips, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        const int total = n * nbands;
        for (int g0 = 0; g0 < total; g0 += c->max_frames) {
            const int m = total - g0 < c->max_frames ? total - g0 : c->max_frames;
            HIP_TRY(launch_audio_frames(p[0], format, nsamples, bands, g0, g0 + m, c->d_audiotab, c->d_audio_iq, c->stream));
            if (run_pipeline_messages(c, c->d_audio_iq, m, c->d_audio_bmsgs + (size_t)g0 * kMaxMessages, c->d_audio_bn + g0)) return -1;
        }
        HIP_TRY(launch_audio_merge(c->d_audio_bmsgs, c->d_audio_bn, n, bands, (ft8gpu_message *)p[1], (int32_t *)p[2], c->stream));
        return 0;
    });
}

}  // extern "C"
