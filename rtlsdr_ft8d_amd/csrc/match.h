// match.h -- launchers of match.hip, shared with its host side api_match.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// the codewords of a frame's table, as the pre-kernel leaves them for the match kernel: six dwords per entry (positions
// 0..173, position p at bit p & 31 of dword p >> 5), entry-minor so that the lanes of a round load neighbouring dwords, and
// the live entries of each round of 64 as a lane mask
constexpr int kExpectEntries = FT8GPU_EXPECT_ENTRIES;
constexpr int kExpectRounds = kExpectEntries / 64;
constexpr size_t kExpectCwBytes = (size_t)kExpectEntries * 6 * sizeof(uint32_t);     // per frame
constexpr size_t kExpectLiveBytes = (size_t)kExpectRounds * sizeof(uint64_t);        // per frame
constexpr size_t kExpectWorkBytes = kExpectCwBytes + kExpectLiveBytes;

// match.hip: the expected messages of a receiver against the candidates BP gives up on (include/ft8gpu.h "expected
// messages").  launch_expect_encode fills work (kExpectWorkBytes per frame: all codeword blocks, then all live masks) from
// states [nframes]; launch_match reads it.  tab: the messages path's tables (the generator rows).
hipError_t launch_expect_encode(const ft8gpu_expect_state *states, int nframes, uint32_t max_age, const MsgTables *tab,
                                void *work, hipStream_t s);
hipError_t launch_match(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                        const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_match_info *info,
                        int nframes, int max_candidates, const void *work, int max_hard_errors, hipStream_t s);
// the update rule over msgs [nrecv][ns][50], n_msgs [nrecv][ns], state [nrecv] (16-byte aligned)
hipError_t launch_expect_update(const ft8gpu_message *msgs, const int32_t *n_msgs, int nrecv, int ns,
                                ft8gpu_expect_state *state, int derive, hipStream_t s);
// pad[2] = 1 for the records [n_before[f * stride], n_msgs[f]) of nframes frames
hipError_t launch_match_tag(const int32_t *n_before, int stride, const int32_t *n_msgs, int nframes, ft8gpu_message *msgs,
                            hipStream_t s);
