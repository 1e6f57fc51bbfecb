// hint.h -- launchers of hint.hip, shared with its host side api_hint.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// hint.hip: the call hints of a receiver against the candidates BP gives up on (include/ft8gpu.h "call hints").
// hint_tables_init uploads the LDPC tables of the kernel's translation unit; launch_hint reads states [nframes] (16-byte
// aligned) and encodes them into work (kHintWorkBytes per frame) ahead of the candidate kernel.  work == nullptr selects, in
// the A/B build only, the other form (FT8GPU_AB_HINT_IN_WAVE: the entries are converted in the wave).
constexpr size_t kHintWorkBytes = (size_t)FT8GPU_HINT_ENTRIES * 8;
hipError_t hint_tables_init(hipStream_t s);
hipError_t launch_hint(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                       const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_hint_info *info,
                       int nframes, int max_candidates, int ldpc_iters, int force_ieee_div, const ft8gpu_hint_state *states,
                       const ft8gpu_hint_params &q, void *work, hipStream_t s);
// the update rule over msgs [nrecv][ns][50], n_msgs [nrecv][ns], state [nrecv] (16-byte aligned)
hipError_t launch_hint_update(const ft8gpu_message *msgs, const int32_t *n_msgs, int nrecv, int ns, ft8gpu_hint_state *state,
                              hipStream_t s);
// pad[2] = 3 for the records [n_before[f * stride], n_msgs[f]) of nframes frames
hipError_t launch_hint_tag(const int32_t *n_before, int stride, const int32_t *n_msgs, int nframes, ft8gpu_message *msgs,
                           hipStream_t s);
