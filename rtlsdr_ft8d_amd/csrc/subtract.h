// subtract.h -- launchers of subtract.hip, shared with its host side api_subtract.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// constant tables of the subtraction (include/ft8gpu.h "subtraction in the I/Q samples"), built on the host
struct SubTables {
    float2 w4[FT8GPU_SUBTRACT_TABLE];                       // (cos, -sin)(2 pi i / 4096)
    float inv[32];                                          // inv[n] = (float)(1.0 / (32 n)), n = 1 .. 17
};

// tables of the GFSK reference (include/ft8gpu.h "GFSK reference"), built on the host by the synthesiser's helpers
struct SubGfskTables {
    uint32_t q[3 * FT8GPU_GFSK_SPS_IQ + 4];                 // Q_512[0 .. 1536] of ft8gpu_gfsk_pulse, padded to whole 16-byte words
    float ramp[FT8GPU_GFSK_SPS_IQ / 8];                     // r[0 .. 63] of ft8gpu_gfsk_ramp
};

// What the estimate kernel leaves for the apply kernel, per record, in dwords: the amplitudes A(q) as 1264 float2, then S*,
// k4*, valid, a zero, and the 79 tones as bytes.
constexpr int kSubSegs = 16 * FT8GPU_NN;                    // 1264 segments of 32 samples
constexpr int kSubHdr = 2 * kSubSegs;                       // dword offset of the header
constexpr int kSubTones = kSubHdr + 4;                      // dword offset of the tone bytes
constexpr int kSubStride = 2560;                            // dwords per record (10 240 bytes)
static_assert(kSubTones + (FT8GPU_NN + 3) / 4 <= kSubStride, "record scratch");

// iq [nframes][2][48000] (16-byte aligned), msgs / refined / info [nframes][50] (info nullable), first / n_msgs [nframes]
// (clamped to [0, 50]); scratch: [nframes][50][kSubStride] dwords.  Records outside [first, n_msgs) are not touched.
// shape: FT8GPU_SUBTRACT_CPFSK (gtab is not read) or FT8GPU_SUBTRACT_GFSK, in both launchers; anything else is hipErrorInvalidValue.
hipError_t launch_subtract_estimate(const float *iq, const ft8gpu_message *msgs, const ft8gpu_refined *refined, const int32_t *first,
                                    const int32_t *n_msgs, int nframes, int shape, const SubTables *tab, const SubGfskTables *gtab,
                                    const MsgTables *mtab, uint32_t *scratch, ft8gpu_subtract_info *info, hipStream_t s);
// out[f] = iq[f] minus the records [first[f], n_msgs[f]) in that order, from what the estimate kernel left in scratch; out may
// be iq.  A frame without such records is copied unchanged.
hipError_t launch_subtract_apply(const float *iq, float *out, const int32_t *first, const int32_t *n_msgs, int nframes, int shape,
                                 const SubTables *tab, const SubGfskTables *gtab, const uint32_t *scratch, hipStream_t s);
// the pass loop's bookkeeping: a frame is active when prev[f] < n_msgs[f] < 50.  n_ref[f] = n_msgs[f] for an active frame and 0
// for every other; *n_active = their number.
hipError_t launch_subtract_active(const int32_t *prev, const int32_t *n_msgs, int nframes, int32_t *n_ref, int32_t *n_active,
                                  hipStream_t s);
// counts[f] = 0 for every frame with n_ref[f] == 0: a frame that is not decoded again offers no candidates
hipError_t launch_subtract_gate(const int32_t *n_ref, int nframes, int32_t *counts, hipStream_t s);
