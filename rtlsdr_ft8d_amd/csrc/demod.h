// demod.h -- launchers of demod.hip, shared with its host side api_demod.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"
#include "subtract.h"

// demod.hip: undecoded candidates demodulated again from the I/Q samples (include/ft8gpu.h "demodulation from the I/Q samples").
// demod_tables_init uploads the file's instance of the LDPC tables (cand_dev.h: LdpcTables).
hipError_t demod_tables_init(hipStream_t s);
// iq [nframes][2][48000], cands / status_in / status_out / info [nframes][max_candidates], counts [nframes]; tab: the subtraction's
// tables (w4).  status_out may be status_in.  Two launches: the marks of the attempted candidates, then the stage.
// soft: nullptr, or [nframes][max_candidates][3][FT8GPU_SOFT_STRIDE] (16-byte aligned) for the kernel that also writes the
// normalised soft bits of the sets it tried (ft8gpu_demod_soft).
hipError_t launch_demod(const float *iq, const ft8gpu_candidate *cands, const int32_t *counts, const ft8gpu_decode_status *status_in,
                        ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, float *soft, int nframes, int max_candidates,
                        const SubTables *tab, int sets, int max_hard_errors, int max_per_frame, int ldpc_iters, int force_ieee_div,
                        hipStream_t s);
// pad[3] = info[cand_index].set for the records [n_before[f], n_msgs[f]) of nframes frames
hipError_t launch_demod_tag(const int32_t *n_before, const int32_t *n_msgs, int nframes, const ft8gpu_demod_info *info,
                            int max_candidates, ft8gpu_message *msgs, hipStream_t s);
