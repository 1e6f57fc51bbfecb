// refine.h -- launcher of refine.hip, shared with its host side api_refine.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// refine.hip: every message record located in the frame's samples (include/ft8gpu.h "refined time and frequency").
// iq [nframes][2][48000] (16-byte aligned), msgs / refined [nframes][50], n_msgs [nframes]; tab: the context's window and
// twiddle tables, mtab: the messages path's tables (the generator rows)
hipError_t launch_refine(const float *iq, const ft8gpu_message *msgs, const int32_t *n_msgs, int nframes, const Ft8Tables *tab,
                         const MsgTables *mtab, ft8gpu_refined *refined, hipStream_t s);
