// pcm.h -- launchers of pcm.hip, shared with its host side api_pcm.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

constexpr int kPcmRates = 5;                                // D = 15 << i, i = 0 .. 4
constexpr int kPcmMaxMix1 = 16 * FT8GPU_PCM_MAX_D;
constexpr int kPcmMaxTapsA = 8 * (FT8GPU_PCM_MAX_D / 3) + 1;

// constant tables of the PCM front end (include/ft8gpu.h "PCM front end"), built on the host (ft8_pcm.c), for every rate
struct PcmTables {
    float2 w1[kPcmRates][kPcmMaxMix1];                      // (cos, -sin)(2 pi i / (16 D)), 16 D entries of row log2(D / 15)
    float hA[kPcmRates][kPcmMaxTapsA + 7];                  // 8 M + 1 taps of that row
    float2 w2[FT8GPU_PCM_MIX2];                             // (cos, -sin)(2 pi i / 1536)
    float hB[FT8GPU_PCM_TAPS_B];                            // 47 taps, hB[47] = 0
};

// the channels of a call, passed by value: the two mixer steps reduced to their tables' periods, and freq_bin for the merge
struct PcmChannels {
    int32_t n;
    int16_t c[FT8GPU_PCM_MAX_CHANNELS];                     // c mod 16 D, in [0, 16 D)
    int16_t q[FT8GPU_PCM_MAX_CHANNELS];                     // q mod 1536, in [0, 1536)
    int32_t bin[FT8GPU_PCM_MAX_CHANNELS];
};

// One 9600 sps plane per (capture, channel): z[m] as (re, im) at index m, m = 0 .. min(143999, (nsamples - 1 + 4 M) / M); the
// second stage reads nothing outside that range, so the rest of a plane is never written.
constexpr size_t kPcmPlaneLen = 144000;
constexpr size_t kPcmPlaneBytes = kPcmPlaneLen * sizeof(float2);

// stage A and the second mixer: pcm [ncaptures][nsamples] samples of `format` (aligned to the sample type) -> planes
// [ncaptures][ch.n][kPcmPlaneLen].  The samples of a capture are fetched once for all its channels.
hipError_t launch_pcm_planes(const void *pcm, int format, int D, int ncaptures, int nsamples, const PcmChannels &ch,
                             const PcmTables *tab, float2 *planes, hipStream_t s);
// stage B: nframes planes (frame g = capture * ch.n + channel, in that order) -> out [nframes][2][48000] (16-byte aligned),
// peak-normalised to 0.5 if normalise != 0
hipError_t launch_pcm_fir(const float2 *planes, int D, int nsamples, int nframes, const PcmTables *tab, float *out, int normalise,
                          hipStream_t s);
// the merge of the whole path, as launch_wide_merge
hipError_t launch_pcm_merge(const ft8gpu_message *chan_msgs, const int32_t *chan_n, int ncaptures, const PcmChannels &ch,
                            ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s);
