// audio.h -- launchers of audio.hip, shared with its host side api_audio.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// constant tables of the audio front end (include/ft8gpu.h "12 kHz audio"), built on the host
struct AudioTables {
    float h[FT8GPU_AUDIO_TAPS];                             // the Kaiser low-pass, h[159] = 0
    float2 wm[FT8GPU_AUDIO_MIX];                            // (cos, -sin)(2 pi i / 1920)
};

// the bands of a call, passed by value
struct AudioBands {
    int32_t n;
    int32_t base[FT8GPU_AUDIO_MAX_BANDS];
};

// The frames [g0, g1) of a chunk of clips, frame g = clip * bands.n + band: pcm [clips][nsamples] of `format` (any alignment; the
// 16-byte loads are taken where a clip's first sample is 16-byte aligned), out [g1 - g0][2][48000] (16-byte aligned) = frame g0
// onwards.  A workgroup fetches its input tile once for all the bands of its clip that lie in [g0, g1).
hipError_t launch_audio_frames(const void *pcm, int format, int nsamples, const AudioBands &bands, int g0, int g1,
                               const AudioTables *tab, float *out, hipStream_t s);
// the merge of the whole path: band_msgs [nclips][bands.n][50], band_n [nclips][bands.n] (clamped to [0, 50]) -> msgs
// [nclips][50 * bands.n] (slots at and behind the count are not written), n_msgs [nclips]
hipError_t launch_audio_merge(const ft8gpu_message *band_msgs, const int32_t *band_n, int nclips, const AudioBands &bands,
                              ft8gpu_message *msgs, int32_t *n_msgs, hipStream_t s);
