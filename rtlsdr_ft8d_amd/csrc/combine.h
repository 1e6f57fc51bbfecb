// combine.h -- launchers of combine.hip, shared with its host side api_combine.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

constexpr int kSoftmemEntries = FT8GPU_SOFTMEM_ENTRIES;

// combine.hip: the soft-bit memory of a receiver against the candidates BP gives up on (include/ft8gpu.h "soft-bit memory").
// combine_tables_init uploads the file's instance of the LDPC tables (cand_dev.h: LdpcTables; a __device__ variable belongs
// to one translation unit, so ap.hip has another).
hipError_t combine_tables_init(hipStream_t s);
hipError_t launch_combine(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                          const ft8gpu_decode_status *status_in, ft8gpu_decode_status *status_out, ft8gpu_combine_info *info,
                          int nframes, int max_candidates, const ft8gpu_softmem_state *states, uint32_t max_age, int min_agree,
                          int ldpc_iters, int force_ieee_div, hipStream_t s);
// the update rule of one slot: reads old [nframes], writes into out [nframes], which holds a copy of old at entry (old != out:
// every sum is formed from the state at entry); both 16-byte aligned
hipError_t launch_softmem_update(const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                                 const ft8gpu_decode_status *status, const ft8gpu_combine_info *info, int nframes,
                                 int max_candidates, const ft8gpu_softmem_state *old, ft8gpu_softmem_state *out,
                                 int store_per_slot, hipStream_t s);
// pad[2] = 2 for the records [n_before[f * stride], n_msgs[f]) of nframes frames
hipError_t launch_combine_tag(const int32_t *n_before, int stride, const int32_t *n_msgs, int nframes, ft8gpu_message *msgs,
                              hipStream_t s);
