// apsoft.h -- launchers of apsoft.hip, shared with its host side api_demod.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// apsoft.hip: a-priori decoding on a soft-bit array (include/ft8gpu.h "a-priori decoding on the soft bits demodulated from the
// I/Q samples").  apsoft_tables_init uploads the file's instance of the LDPC tables (cand_dev.h: LdpcTables).
hipError_t apsoft_tables_init(hipStream_t s);
// soft [nframes][max_candidates][3][FT8GPU_SOFT_STRIDE] (16-byte aligned), status_in / status_out / info
// [nframes][max_candidates], counts [nframes]; hyps is host memory (it travels as a kernel argument).  status_out may be
// status_in.
hipError_t launch_ap_soft(const float *soft, const int32_t *counts, const ft8gpu_decode_status *status_in,
                          ft8gpu_decode_status *status_out, ft8gpu_apsoft_info *info, int nframes, int max_candidates, int ldpc_iters,
                          int force_ieee_div, int sets, const ft8gpu_ap_hypothesis *hyps, int nhyp, int max_hard_errors, hipStream_t s);
// pad[1] = 1 + info[cand_index].hyp and pad[3] = info[cand_index].set for the records [n_before[f], n_msgs[f]) of nframes frames
hipError_t launch_ap_soft_tag(const int32_t *n_before, const int32_t *n_msgs, int nframes, const ft8gpu_apsoft_info *info,
                              int max_candidates, ft8gpu_message *msgs, hipStream_t s);
