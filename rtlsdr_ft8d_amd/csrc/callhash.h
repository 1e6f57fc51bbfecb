// callhash.h -- launcher of callhash.hip, shared with its host side api_callhash.hip (not installed).
#pragma once
#include "ft8gpu_internal.h"

// callhash.hip: the call hash table of nrecv receivers over ns consecutive slots each (include/ft8gpu.h "hashed call signs").
// msgs / resolved [nrecv][ns][50], n_msgs [nrecv][ns], state [nrecv]; every pointer 16-byte aligned; ns <= 2^24.
hipError_t launch_callhash(const ft8gpu_message *msgs, const int32_t *n_msgs, int nrecv, int ns, ft8gpu_callhash_state *state,
                           uint32_t max_age, ft8gpu_resolved *resolved, hipStream_t s);
