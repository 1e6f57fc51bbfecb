// api_pcm.hip -- host side of the PCM front end: the stage entry ft8gpu_pcm_frames and the whole path ft8gpu_decode_pcm
// (DESIGN.md "PCM front end"; the kernels are pcm.hip, the tables and the .wav reader plain C in ft8_pcm.c).
//
// Both entries cut the captures with for_each_chunk, as api_wide.hip does.  A chunk's captures go through the planes kernel in
// runs of at most kPlaneRun planes (capture, channel), so the 9600 sps planes take 74 MB at most; a run's frames g = capture *
// nchannels + channel are then worked off in pieces of at most max_frames through one frame buffer.  Everything here is allocated
// on the first PCM call that needs it, so ft8gpu_create's footprint is unchanged.
#include "pcm.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr size_t kFrameFloats = 2 * (size_t)kNSamples;
constexpr size_t kFrameBytes = kFrameFloats * sizeof(float);
constexpr size_t kChanMsgBytes = kMaxMessages * sizeof(ft8gpu_message);
constexpr int kPlaneRun = 64;                               // planes in flight between the two stages

int ensure_pcm_tables(ft8gpu_ctx *c) {
    return c->mem.table(&c->d_pcmtab, "the PCM front end's tables", [](PcmTables *h) {
        for (int i = 0; i < kPcmRates; ++i) {
            ft8gpu_pcm_mixer1(15 << i, &h->w1[i][0].x);
            if (ft8gpu_pcm_taps_a(15 << i, h->hA[i]) < 0) return ft8_fail("the PCM front end's taps of D = %d", 15 << i);
        }
        ft8gpu_pcm_mixer2(&h->w2[0].x);
        ft8gpu_pcm_taps_b(h->hB);
        return 0;
    });
}

// a buffer of the PCM path at `need` bytes or more; the stream is drained first if the old block has to go
template <class T> int pcm_grow(ft8gpu_ctx *c, T **field, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return c->mem.grow(field, cap, need, what);
}

int pcm_iq(ft8gpu_ctx *c) { return c->mem.once(&c->d_pcm_iq, (size_t)c->max_frames * kFrameBytes, "the PCM front end's frames"); }

struct PcmCall {
    int format, D;
    size_t sample_bytes;                                    // of one element
    size_t capture_bytes;
    PcmChannels ch;
};

// the refusals of both entries, before anything is enqueued
int check_pcm_args(int format, int rate, int nsamples, const int32_t *freq_bin, int nchannels, PcmCall *call) {
    if (format < 0 || format > (FT8GPU_PCM_F32 | FT8GPU_PCM_COMPLEX)) return ft8_fail("unknown PCM format %d", format);
    const int D = ft8gpu_pcm_decimation(rate);
    if (D == 0) return ft8_fail("rate %d is not one of 48000, 96000, 192000, 384000, 768000", rate);
    if (nchannels < 1 || nchannels > FT8GPU_PCM_MAX_CHANNELS)
        return ft8_fail("nchannels %d out of range [1, %d]", nchannels, FT8GPU_PCM_MAX_CHANNELS);
    if (!freq_bin) return ft8_fail("NULL array argument");
    if (nsamples < 1 || nsamples > FT8GPU_PCM_MAX_SAMPLES_PER_D * D)
        return ft8_fail("nsamples %d out of range [1, %d]", nsamples, FT8GPU_PCM_MAX_SAMPLES_PER_D * D);
    const bool cplx = format & FT8GPU_PCM_COMPLEX;
    const int lo = cplx ? -256 * D : 0, hi = 256 * D - 256, period = 16 * D;
    *call = PcmCall{};
    call->format = format;
    call->D = D;
    call->sample_bytes = (format & FT8GPU_PCM_F32) ? sizeof(float) : sizeof(int16_t);
    call->capture_bytes = (size_t)nsamples * (cplx ? 2 : 1) * call->sample_bytes;
    PcmChannels *ch = &call->ch;
    ch->n = nchannels;
    for (int b = 0; b < nchannels; ++b) {
        if (freq_bin[b] < lo || freq_bin[b] > hi)
            return ft8_fail("freq_bin[%d] = %d out of range [%d, %d]", b, (int)freq_bin[b], lo, hi);
        const int f = freq_bin[b] + 128;
        const int cc = (f + 16 + 32 * 4096) / 32 - 4096;     // floor((F + 16) / 32)
        const int q = f - 32 * cc;                           // in [-16, 15]
        ch->c[b] = (int16_t)(((cc % period) + period) % period);
        ch->q[b] = (int16_t)((q + FT8GPU_PCM_MIX2) % FT8GPU_PCM_MIX2);
        ch->bin[b] = freq_bin[b];
    }
    return 0;
}

// The frames of a chunk of n captures: planes run by run, then each run's frames in pieces of at most `piece` frames through
// sink(g, m, planes of frame g), g counted from the chunk's first frame.
template <class Sink>
int pcm_chunk(ft8gpu_ctx *c, const void *pcm, int n, int nsamples, const PcmCall &call, int piece, Sink sink) {
    const PcmChannels &ch = call.ch;
    const int run = kPlaneRun / ch.n > 0 ? kPlaneRun / ch.n : 1;                 // captures per run
    float2 *planes = (float2 *)c->d_pcm_planes;
    for (int c0 = 0; c0 < n; c0 += run) {
        const int nc = n - c0 < run ? n - c0 : run;
        HIP_TRY(launch_pcm_planes((const char *)pcm + (size_t)c0 * call.capture_bytes, call.format, call.D, nc, nsamples, ch,
                                  c->d_pcmtab, planes, c->stream));
        const int total = nc * ch.n;
        for (int g0 = 0; g0 < total; g0 += piece) {
            const int m = total - g0 < piece ? total - g0 : piece;
            if (sink(c0 * ch.n + g0, m, planes + (size_t)g0 * kPcmPlaneLen)) return -1;
        }
    }
    return 0;
}

int pcm_planes(ft8gpu_ctx *c, int ncaptures, int nchannels) {
    const int chunk = ncaptures < c->max_frames ? ncaptures : c->max_frames;
    const int run = kPlaneRun / nchannels > 0 ? kPlaneRun / nchannels : 1;
    const size_t planes = (size_t)(chunk < run ? chunk : run) * nchannels;
    return pcm_grow(c, &c->d_pcm_planes, &c->pcm_planes_cap, planes * kPcmPlaneBytes, "the PCM front end's planes");
}

}  // namespace

extern "C" {

int ft8gpu_pcm_frames(ft8gpu_ctx *c, const void *pcm, int format, int rate, int ncaptures, int nsamples, const int32_t *freq_bin,
                      int nchannels, float *iq, int normalise, int flags) {
    CHECK_COMMON(c, ncaptures);
    PcmCall call;
    if (check_pcm_args(format, rate, nsamples, freq_bin, nchannels, &call)) return -1;
    if (ncaptures == 0) return 0;
    if (!pcm || !iq) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)pcm & (call.sample_bytes - 1)) != 0) return ft8_fail("pcm must be aligned to its sample type");
    if (dev && ((uintptr_t)iq & 15) != 0) return ft8_fail("iq must be 16-byte aligned");
    if (ensure_pcm_tables(c) || pcm_planes(c, ncaptures, nchannels)) return -1;
    const int chunk = ncaptures < c->max_frames ? ncaptures : c->max_frames;
    if (!dev && (pcm_iq(c) || pcm_grow(c, &c->d_pcm_raw, &c->pcm_raw_cap, (size_t)chunk * call.capture_bytes, "staging of the captures")))
        return -1;
    const StageArg a[] = { { pcm, c->d_pcm_raw, call.capture_bytes, kIn } };
    size_t done = 0;                                        // frames of the chunks before this one
    return for_each_chunk(c, ncaptures, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        float *user = iq + done * kFrameFloats;
        done += (size_t)n * nchannels;
        const int piece = dev ? n * nchannels : c->max_frames;
        return pcm_chunk(c, p[0], n, nsamples, call, piece, [&](int g, int m, const float2 *planes) {
            if (dev) {
                HIP_TRY(launch_pcm_fir(planes, call.D, nsamples, m, c->d_pcmtab, user + g * kFrameFloats, normalise, c->stream));
                return 0;
            }
            HIP_TRY(launch_pcm_fir(planes, call.D, nsamples, m, c->d_pcmtab, c->d_pcm_iq, normalise, c->stream));
            HIP_TRY(hipMemcpyAsync(user + g * kFrameFloats, c->d_pcm_iq, m * kFrameBytes, hipMemcpyDeviceToHost, c->stream));
            return 0;
        });
    });
}

int ft8gpu_decode_pcm(ft8gpu_ctx *c, const void *pcm, int format, int rate, int ncaptures, int nsamples, const int32_t *freq_bin,
                      int nchannels, ft8gpu_message *msgs, int32_t *n_msgs, int flags) {
    CHECK_COMMON(c, ncaptures);
    PcmCall call;
    if (check_pcm_args(format, rate, nsamples, freq_bin, nchannels, &call)) return -1;
    if (ncaptures == 0) return 0;
    if (!pcm || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)pcm & (call.sample_bytes - 1)) != 0) return ft8_fail("pcm must be aligned to its sample type");
    if (ensure_messages_buffers(c)) return -1;
    if (ensure_pcm_tables(c) || pcm_planes(c, ncaptures, nchannels) || pcm_iq(c)) return -1;
    const size_t chunk = (size_t)(ncaptures < c->max_frames ? ncaptures : c->max_frames);
    if (pcm_grow(c, &c->d_pcm_cmsgs, &c->pcm_cmsgs_cap, chunk * nchannels * kChanMsgBytes, "the channels' records") ||
        pcm_grow(c, &c->d_pcm_cn, &c->pcm_cn_cap, chunk * nchannels * sizeof(int32_t), "the channels' counts"))
        return -1;
    if (!dev && (pcm_grow(c, &c->d_pcm_raw, &c->pcm_raw_cap, chunk * call.capture_bytes, "staging of the captures") ||
                 pcm_grow(c, &c->d_pcm_msgs, &c->pcm_msgs_cap, chunk * nchannels * kChanMsgBytes, "staging of the merged records")))
        return -1;
    // slots past a capture's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { pcm, c->d_pcm_raw, call.capture_bytes, kIn },
                           { msgs, c->d_pcm_msgs, (size_t)nchannels * kChanMsgBytes, kInOut }, { n_msgs, c->d_nres, sizeof(int32_t), kOut } };
    return for_each_chunk(c, ncaptures, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        if (pcm_chunk(c, p[0], n, nsamples, call, c->max_frames, [&](int g, int m, const float2 *planes) {
                HIP_TRY(launch_pcm_fir(planes, call.D, nsamples, m, c->d_pcmtab, c->d_pcm_iq, 1, c->stream));
                return run_pipeline_messages(c, c->d_pcm_iq, m, c->d_pcm_cmsgs + (size_t)g * kMaxMessages, c->d_pcm_cn + g);
            }))
            return -1;
        HIP_TRY(launch_pcm_merge(c->d_pcm_cmsgs, c->d_pcm_cn, n, call.ch, (ft8gpu_message *)p[1], (int32_t *)p[2], c->stream));
        return 0;
    });
}

}  // extern "C"
