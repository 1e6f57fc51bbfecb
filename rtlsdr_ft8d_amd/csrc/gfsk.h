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
static_assert(offsetof(GfskTables, gc) % 16 == 0 && offsetof(GfskTables, gf) % 16 == 0, "gc and gf are loaded 16 bytes at a time");
static_assert(sizeof(GfskHeader) == 96, "GfskHeader is copied to LDS as 24 words");

constexpr int kGfskTile = FT8GPU_GFSK_TILE;                 // output samples per workgroup
constexpr int kGfskMaxTiles = (FT8GPU_AUDIO_NSAMPLES + kGfskTile - 1) / kGfskTile;   // 22 (the I/Q mode has 6)
inline int gfsk_clip_samples(int mode, int nsamples) { return mode == FT8GPU_GFSK_IQ ? kNSamples : nsamples; }
inline int gfsk_tiles(int mode, int nsamples) { return (gfsk_clip_samples(mode, nsamples) + kGfskTile - 1) / kGfskTile; }

// The clips [0, nclips) of a chunk, clip c being global clip first + c for the noise: hdr [nclips][nsig] (device memory) -> out
// [nclips][2][48000] floats (I/Q mode; format is FT8GPU_AUDIO_F32) or [nclips][nsamples] of `format` (audio mode), before any
// normalisation.  tile_max [nclips][gfsk_tiles()] (nullptr: not wanted) gets the largest |x| of every tile.
hipError_t launch_gfsk(int mode, int format, const GfskHeader *hdr, int nclips, int nsig, int nsamples, const GfskTables *tab,
                       float noise_sigma, uint64_t seed, uint64_t first, void *out, float *tile_max, hipStream_t s);
// The second pass: x [nclips][len] floats, scaled by peak / max(the clip's largest tile_max entry, 1e-24f), go to out
// [nclips][len] of `format` (out == x is allowed for floats).  ntiles: tile_max entries per clip.
hipError_t launch_gfsk_normalise(int format, const float *x, const float *tile_max, int nclips, int len, int ntiles, float peak,
                                 void *out, hipStream_t s);
