// wide.h -- launchers of wide.hip, shared with its host side api_wide.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// constant tables of the wideband RX front end (include/ft8gpu.h "wideband RX"), built on the host (ft8_wide.c)
struct WideTables {
    int16_t w1[2 * FT8GPU_WIDE_MIX1];                       // (lrint(32767 cos), -lrint(32767 sin))(2 pi i / 6000)
    float2 w2[FT8GPU_WIDE_MIX2];                            // (cos, -sin)(2 pi i / 3072)
    float h[FT8GPU_WIDE_TAPS];                              // the second stage's taps, h[95] = 0
};

// the channels of a call, passed by value: the two mixer steps reduced to their tables' periods, and freq_bin for the merge
struct WideChannels {
    int32_t n;
    int16_t c[FT8GPU_WIDE_MAX_CHANNELS];                    // c mod 6000, in [0, 6000)
    int16_t q[FT8GPU_WIDE_MAX_CHANNELS];                    // q mod 3072, in [0, 3072)
    int32_t bin[FT8GPU_WIDE_MAX_CHANNELS];
};

// One 19 200 sps plane per (capture, channel): z[m] as (re, im) at index m + kWidePlanePad, m = -1 .. (npairs + 247) / 125; the
// second stage reads nothing outside that range, so the rest of a plane is never written.
constexpr int kWidePlanePad = 48;
constexpr size_t kWidePlaneLen = 288128;                    // >= kWidePlanePad + (36 000 000 + 247) / 125 + 1
constexpr size_t kWidePlaneBytes = kWidePlaneLen * sizeof(float2);

// stage A and the second mixer: raw [ncaptures][2 npairs] (16-byte aligned, npairs a multiple of 8) -> planes
// [ncaptures][ch.n][kWidePlaneLen].  The bytes of a capture are fetched once for all its channels.
hipError_t launch_wide_planes(const uint8_t *raw, int ncaptures, size_t npairs, const WideChannels &ch, const WideTables *tab,
                              float2 *planes, hipStream_t s);
// stage B: nframes planes (frame g = capture * ch.n + channel, in that order) -> out [nframes][2][48000] (16-byte aligned),
// peak-normalised to 0.5 if normalise != 0
hipError_t launch_wide_fir(const float2 *planes, size_t npairs, int nframes, const WideTables *tab, float *out, int normalise,
                           hipStream_t s);
// the merge of the whole path: chan_msgs [ncaptures][ch.n][50], chan_n [ncaptures][ch.n] (clamped to [0, 50]) -> msgs
// [ncaptures][50 * ch.n] (slots at and behind the count are not written), n_msgs [ncaptures]
hipError_t launch_wide_merge(const ft8gpu_message *chan_msgs, const int32_t *chan_n, int ncaptures, const WideChannels &ch,
                             ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s);
