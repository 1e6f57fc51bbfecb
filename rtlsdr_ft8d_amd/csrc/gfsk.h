// gfsk.h -- launchers of gfsk.hip, shared with its host side api_gfsk.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

#include <stddef.h>

// constant tables of the GFSK synthesiser (include/ft8gpu.h "GFSK synthesis"), built on the host (ft8_gfsk.c)
struct GfskTables {
    float2 gc[FT8GPU_GFSK_TWIDDLES];                        // (cos, sin)(2 pi i / 4096); first, 16-byte aligned: copied to LDS
    float2 gf[FT8GPU_GFSK_TWIDDLES];                        // (cos, sin)(2 pi i / 2^24)    as float4
    uint32_t q_iq[3 * FT8GPU_GFSK_SPS_IQ + 1];              // Q_512
    uint32_t q_audio[3 * FT8GPU_GFSK_SPS_AUDIO + 1];        // Q_1920
    float ramp_iq[FT8GPU_GFSK_SPS_IQ / 8];
    float ramp_audio[FT8GPU_GFSK_SPS_AUDIO / 8];
};

// one signal as the kernel takes it: what the host derives from an ft8gpu_synth_signal (24 words)
struct GfskHeader {
    uint32_t step;                                          // f0 in units of 2^-32 turn per sample
    int32_t start;                                          // output sample of the signal's local sample 0
    float amplitude;
    uint8_t e[84];                                          // the extended tones e[0 .. 80]
};
// one signal's channel as the kernels take it: what the host derives from an ft8gpu_channel (include/ft8gpu.h "Fading channel")
struct GfskChannel {
    uint32_t gstep[2][FT8GPU_CHANNEL_TAPS];                 // per path: the taps' phase steps per grid step
    uint32_t theta[2][FT8GPU_CHANNEL_TAPS];                 //           and start phases
    float w[2];                                             // the paths' amplitudes
    int32_t d;                                              // delay of path 1 in samples
    uint32_t paths;                                         // 0: the unfaded rule; 1 or 2: faded, that many paths
};
static_assert(offsetof(GfskTables, gc) % 16 == 0 && offsetof(GfskTables, gf) % 16 == 0, "gc and gf are loaded 16 bytes at a time");
static_assert(sizeof(GfskHeader) == 96, "GfskHeader is copied to LDS as 24 words");
static_assert(sizeof(GfskChannel) == 272 && offsetof(GfskChannel, w) == 256 && offsetof(GfskChannel, d) == 264, "GfskChannel layout");
constexpr int kGfskGrid = FT8GPU_CHANNEL_GRID;              // grid points of one path
static_assert(kGfskGrid == FT8GPU_NN * FT8GPU_GFSK_SPS_IQ / FT8GPU_CHANNEL_STEP_IQ + 1 &&
              kGfskGrid == FT8GPU_NN * FT8GPU_GFSK_SPS_AUDIO / FT8GPU_CHANNEL_STEP_AUDIO + 1, "both modes have the same grid in time");

constexpr int kGfskTile = FT8GPU_GFSK_TILE;                 // output samples per workgroup
constexpr int kGfskMaxTiles = (FT8GPU_AUDIO_NSAMPLES + kGfskTile - 1) / kGfskTile;   // 22 (the I/Q mode has 6)
inline int gfsk_clip_samples(int mode, int nsamples) { return mode == FT8GPU_GFSK_IQ ? kNSamples : nsamples; }
inline int gfsk_tiles(int mode, int nsamples) { return (gfsk_clip_samples(mode, nsamples) + kGfskTile - 1) / kGfskTile; }

// The clips [0, nclips) of a chunk, clip c being global clip first + c for the noise: hdr [nclips][nsig] (device memory) -> out
// [nclips][2][48000] floats (I/Q mode; format is FT8GPU_AUDIO_F32) or [nclips][nsamples] of `format` (audio mode), before any
// normalisation.  tile_max [nclips][gfsk_tiles()] (nullptr: not wanted) gets the largest |x| of every tile.
hipError_t launch_gfsk(int mode, int format, const GfskHeader *hdr, int nclips, int nsig, int nsamples, const GfskTables *tab,
                       float noise_sigma, uint64_t seed, uint64_t first, void *out, float *tile_max, hipStream_t s);
// The grid values of a chunk's faded paths: ch [nclips][nsig] (device memory) -> grid [nclips][nsig][2][kGfskGrid] (cos, sin)
// pairs; the entries of a path that ch does not use are left as they are.
hipError_t launch_gfsk_grid(const GfskChannel *ch, int nclips, int nsig, const GfskTables *tab, float2 *grid, hipStream_t s);
// launch_gfsk with channels: ch and grid as above, grid filled by launch_gfsk_grid on the same stream
hipError_t launch_gfsk_faded(int mode, int format, const GfskHeader *hdr, const GfskChannel *ch, const float2 *grid, int nclips, int nsig,
                             int nsamples, const GfskTables *tab, float noise_sigma, uint64_t seed, uint64_t first, void *out,
                             float *tile_max, hipStream_t s);
// The second pass: x [nclips][len] floats, scaled by peak / max(the clip's largest tile_max entry, 1e-24f), go to out
// [nclips][len] of `format` (out == x is allowed for floats).  ntiles: tile_max entries per clip.
hipError_t launch_gfsk_normalise(int format, const float *x, const float *tile_max, int nclips, int len, int ntiles, float peak,
                                 void *out, hipStream_t s);
