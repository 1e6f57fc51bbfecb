// api_gfsk.hip -- host side of the GFSK synthesiser: ft8gpu_synth_gfsk_frames and ft8gpu_synth_gfsk_audio (DESIGN.md "GFSK
// synthesis"; the kernels are gfsk.hip, the tables plain C in ft8_gfsk.c).
//
// Both entries check their arguments first (a refusal needs no GPU), derive the signals' headers (step, start, extended tones)
// on the host, and cut the clips with for_each_chunk.  With peak == 0 the kernel writes the caller's format directly; otherwise
// it writes floats (into the output itself where that holds floats) and leaves the tiles' maxima, and a second launch scales.
// Everything here is allocated on the first GFSK call, so ft8gpu_create's footprint is unchanged.
// With channels ("Fading channel") of which at least one is faded, the host also derives the taps, delays and path amplitudes,
// and every chunk gets a launch that fills its paths' grid values in front of the faded kernel; a call without a faded signal is
// the unfaded one.
#include "gfsk.h"
#include "ft8gpu_ctx.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace {

constexpr size_t kClipFloats = FT8GPU_AUDIO_NSAMPLES;       // the longest output of a clip in floats (an I/Q frame takes 96000)

int ensure_gfsk_tables(ft8gpu_ctx *c) {
    return c->mem.table(&c->d_gfsktab, "the GFSK tables", [](GfskTables *h) {
        ft8gpu_gfsk_pulse(FT8GPU_GFSK_SPS_IQ, h->q_iq);
        ft8gpu_gfsk_pulse(FT8GPU_GFSK_SPS_AUDIO, h->q_audio);
        ft8gpu_gfsk_twiddles(&h->gc[0].x, &h->gf[0].x);
        ft8gpu_gfsk_ramp(FT8GPU_GFSK_SPS_IQ, h->ramp_iq);
        ft8gpu_gfsk_ramp(FT8GPU_GFSK_SPS_AUDIO, h->ramp_audio);
        return 0;
    });
}

// the refusals of both entries; on success hdr holds the nclips * nsig headers
int check_gfsk_args(int mode, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nclips, int nsig, int nsamples,
                    float noise_sigma, uint64_t seed, uint64_t first, float peak, int format, std::vector<GfskHeader> *hdr,
                    std::vector<GfskChannel> *chs) {
    const int rate = mode == FT8GPU_GFSK_IQ ? 3200 : FT8GPU_AUDIO_RATE;
    if (format != FT8GPU_AUDIO_S16 && format != FT8GPU_AUDIO_F32) return ft8_fail("unknown audio format %d", format);
    if (nsamples < 1 || nsamples > FT8GPU_AUDIO_NSAMPLES)
        return ft8_fail("nsamples %d out of range [1, %d]", nsamples, FT8GPU_AUDIO_NSAMPLES);
    if (nsig < 0 || nsig > FT8GPU_GFSK_MAX_SIGNALS) return ft8_fail("nsig %d out of range [0, %d]", nsig, FT8GPU_GFSK_MAX_SIGNALS);
    if (!isfinite(noise_sigma) || noise_sigma < 0.0f) return ft8_fail("noise_sigma %g is negative or not finite", (double)noise_sigma);
    if (!isfinite(peak) || peak < 0.0f) return ft8_fail("peak %g is negative or not finite", (double)peak);
    if (nclips < 1 || nsig == 0) return 0;
    if (!signals) return ft8_fail("NULL array argument");
    const size_t total = (size_t)nclips * nsig;
    hdr->resize(total);
    for (size_t g = 0; g < total; ++g) {
        const ft8gpu_synth_signal &sg = signals[g];
        const int clip = (int)(g / nsig), s = (int)(g % nsig);
        if (!isfinite(sg.f0_hz) || !isfinite(sg.t0_s) || !isfinite(sg.amplitude))
            return ft8_fail("signal %d of clip %d: f0_hz, t0_s or amplitude is not finite", s, clip);
        if (mode == FT8GPU_GFSK_AUDIO && (sg.f0_hz < 0.0f || sg.f0_hz >= (float)rate))
            return ft8_fail("signal %d of clip %d: f0_hz %g out of range [0, %d)", s, clip, (double)sg.f0_hz, rate);
        if (fabsf(sg.f0_hz) >= (float)rate)
            return ft8_fail("signal %d of clip %d: f0_hz %g out of range (-%d, %d)", s, clip, (double)sg.f0_hz, rate, rate);
        if (fabsf(sg.t0_s) > 60.0f) return ft8_fail("signal %d of clip %d: t0_s %g out of range [-60, 60]", s, clip, (double)sg.t0_s);
        GfskHeader &h = (*hdr)[g];
        h.step = (uint32_t)(unsigned long long)llrint((double)sg.f0_hz * 4294967296.0 / (double)rate);
        h.start = (int32_t)lrintf(sg.t0_s * (float)rate);
        h.amplitude = sg.amplitude;
        for (int j = 0; j < FT8GPU_NN; ++j) {
            if (sg.tones[j] > 7) return ft8_fail("signal %d of clip %d: tone %d is %d, above 7", s, clip, j, (int)sg.tones[j]);
            h.e[j + 1] = sg.tones[j];
        }
        h.e[0] = sg.tones[0];
        h.e[80] = sg.tones[FT8GPU_NN - 1];
        h.e[81] = h.e[82] = h.e[83] = 0;
    }
    if (!channels) return 0;
    bool faded = false;
    for (size_t g = 0; g < total; ++g) {
        const ft8gpu_channel &ch = channels[g];
        const int clip = (int)(g / nsig), s = (int)(g % nsig);
        switch (ft8gpu_channel_check(&ch)) {
        case 1: return ft8_fail("channel of signal %d of clip %d: spread_hz %g out of range [0, 20] or not finite", s, clip, (double)ch.spread_hz);
        case 2: return ft8_fail("channel of signal %d of clip %d: delay_ms %g out of range [0, 10] or not finite", s, clip, (double)ch.delay_ms);
        case 3: return ft8_fail("channel of signal %d of clip %d: path2_gain %g out of range [0, 4] or not finite", s, clip, (double)ch.path2_gain);
        case 4: return ft8_fail("channel of signal %d of clip %d: unknown mode %u", s, clip, (unsigned)ch.mode);
        }
        faded = faded || ch.mode == FT8GPU_CHANNEL_FADED;
    }
    if (!faded) return 0;                                   // all unfaded: the unfaded entry
    chs->resize(total);
    for (size_t g = 0; g < total; ++g) {
        const ft8gpu_channel &ch = channels[g];
        GfskChannel &k = (*chs)[g];
        memset(&k, 0, sizeof k);
        if (ch.mode != FT8GPU_CHANNEL_FADED) continue;
        const float g2 = ch.path2_gain, r = sqrtf(1.0f + g2 * g2);
        k.w[0] = 1.0f / r;
        k.w[1] = g2 / r;
        k.d = (int32_t)lrintf(ch.delay_ms * (float)rate / 1000.0f);
        k.paths = g2 == 0.0f ? 1u : 2u;
        for (uint32_t p = 0; p < k.paths; ++p)
            ft8gpu_channel_taps(seed, first + (uint64_t)(g / nsig), (uint32_t)(g % nsig), p, ch.spread_hz, k.gstep[p], k.theta[p]);
    }
    return 0;
}

int synth_gfsk(ft8gpu_ctx *c, int mode, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nclips, int nsig,
               int nsamples, float noise_sigma, uint64_t seed, uint64_t first, float peak, int format, void *out, int flags) {
    std::vector<GfskHeader> hdr;
    std::vector<GfskChannel> chs;                           // empty: no signal of the call is faded
    if (nclips >= 0 && check_gfsk_args(mode, signals, channels, nclips, nsig, nsamples, noise_sigma, seed, first, peak, format, &hdr, &chs))
        return -1;
    CHECK_COMMON(c, nclips);
    if (nclips == 0) return 0;
    if (!out) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    const bool iq = mode == FT8GPU_GFSK_IQ;
    const size_t len = iq ? 2 * (size_t)kNSamples : (size_t)nsamples;               // values per clip
    const size_t out_bytes = len * (format == FT8GPU_AUDIO_S16 ? sizeof(int16_t) : sizeof(float));
    const int ntiles = gfsk_tiles(mode, nsamples);
    const size_t mf = (size_t)c->max_frames;
    if (ensure_gfsk_tables(c)) return -1;
    if (!dev && c->mem.once(&c->d_gfsk_out, mf * kClipFloats * sizeof(float), "staging of the GFSK output")) return -1;
    if (peak > 0.0f && c->mem.once(&c->d_gfsk_max, mf * kGfskMaxTiles * sizeof(float), "the GFSK tiles' maxima")) return -1;
    if (peak > 0.0f && format == FT8GPU_AUDIO_S16 && c->mem.once(&c->d_gfsk_x, mf * kClipFloats * sizeof(float), "the GFSK floats")) return -1;
    HIP_TRY(hipStreamSynchronize(c->stream));               // an earlier call's launches may still read the headers
    if (!hdr.empty()) {
        if (c->mem.grow(&c->d_gfsk_hdr, &c->gfsk_hdr_cap, hdr.size() * sizeof(GfskHeader), "the GFSK signal headers")) return -1;
        HIP_TRY(hipMemcpyAsync(c->d_gfsk_hdr, hdr.data(), hdr.size() * sizeof(GfskHeader), hipMemcpyHostToDevice, c->stream));
        if (!chs.empty()) {
            const size_t per_clip = (size_t)nsig * 2 * kGfskGrid * sizeof(float2);
            if (c->mem.grow(&c->d_gfsk_ch, &c->gfsk_ch_cap, chs.size() * sizeof(GfskChannel), "the GFSK channel headers")) return -1;
            if (c->mem.grow(&c->d_gfsk_grid, &c->gfsk_grid_cap, std::min((size_t)nclips, mf) * per_clip, "the GFSK channels' grid values")) return -1;
            HIP_TRY(hipMemcpyAsync(c->d_gfsk_ch, chs.data(), chs.size() * sizeof(GfskChannel), hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));           // hdr and chs are gone when this call returns
    }
    const StageArg a[] = { { out, c->d_gfsk_out, out_bytes, kOut } };
    size_t done = 0;                                        // clips of the chunks before this one
    return for_each_chunk(c, nclips, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        const GfskHeader *h = c->d_gfsk_hdr + done * (size_t)nsig;
        const uint64_t g0 = first + (uint64_t)done;
        const GfskChannel *k = chs.empty() ? nullptr : c->d_gfsk_ch + done * (size_t)nsig;
        done += (size_t)n;
        if (k) HIP_TRY(launch_gfsk_grid(k, n, nsig, c->d_gfsktab, c->d_gfsk_grid, c->stream));
        // one launch of either kernel: fmt and the maxima as the caller or the second pass wants them
        auto launch = [&](int fmt, void *dst, float *tile_max) {
            return k ? launch_gfsk_faded(mode, fmt, h, k, c->d_gfsk_grid, n, nsig, nsamples, c->d_gfsktab, noise_sigma, seed, g0, dst, tile_max, c->stream)
                     : launch_gfsk(mode, fmt, h, n, nsig, nsamples, c->d_gfsktab, noise_sigma, seed, g0, dst, tile_max, c->stream);
        };
        if (!(peak > 0.0f)) {
            HIP_TRY(launch(format, p[0], nullptr));
            return 0;
        }
        float *x = format == FT8GPU_AUDIO_S16 ? c->d_gfsk_x : (float *)p[0];
        HIP_TRY(launch(FT8GPU_AUDIO_F32, x, c->d_gfsk_max));
        HIP_TRY(launch_gfsk_normalise(format, x, c->d_gfsk_max, n, (int)len, ntiles, peak, p[0], c->stream));
        return 0;
    });
}

}  // namespace

extern "C" {

int ft8gpu_synth_gfsk_frames(ft8gpu_ctx *c, const ft8gpu_synth_signal *signals, int nframes, int nsig, float noise_sigma, uint64_t seed,
                             uint64_t first_frame, float peak, float *iq_out, int flags) {
    return synth_gfsk(c, FT8GPU_GFSK_IQ, signals, nullptr, nframes, nsig, kNSamples, noise_sigma, seed, first_frame, peak, FT8GPU_AUDIO_F32,
                      iq_out, flags);
}

int ft8gpu_synth_gfsk_audio(ft8gpu_ctx *c, const ft8gpu_synth_signal *signals, int nclips, int nsig, int nsamples, float noise_sigma,
                            uint64_t seed, uint64_t first_clip, float peak, int format, void *pcm_out, int flags) {
    return synth_gfsk(c, FT8GPU_GFSK_AUDIO, signals, nullptr, nclips, nsig, nsamples, noise_sigma, seed, first_clip, peak, format, pcm_out, flags);
}

int ft8gpu_synth_gfsk_frames_faded(ft8gpu_ctx *c, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nframes, int nsig,
                                   float noise_sigma, uint64_t seed, uint64_t first_frame, float peak, float *iq_out, int flags) {
    return synth_gfsk(c, FT8GPU_GFSK_IQ, signals, channels, nframes, nsig, kNSamples, noise_sigma, seed, first_frame, peak, FT8GPU_AUDIO_F32,
                      iq_out, flags);
}

int ft8gpu_synth_gfsk_audio_faded(ft8gpu_ctx *c, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nclips, int nsig,
                                  int nsamples, float noise_sigma, uint64_t seed, uint64_t first_clip, float peak, int format, void *pcm_out,
                                  int flags) {
    return synth_gfsk(c, FT8GPU_GFSK_AUDIO, signals, channels, nclips, nsig, nsamples, noise_sigma, seed, first_clip, peak, format, pcm_out, flags);
}

}  // extern "C"
