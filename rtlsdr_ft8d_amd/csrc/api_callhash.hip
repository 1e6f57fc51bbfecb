// api_callhash.hip -- host side of the call hash table: the stage entry ft8gpu_resolve_calls and the whole path
// ft8gpu_decode_messages_resolved (DESIGN.md "Call hash table"; the kernel is callhash.hip, the host helpers of the table are
// plain C in ft8_pack.c).
//
// A receiver is sequential in its slots and independent of every other receiver, so work is cut along exactly those two
// lines (Pieces, ft8gpu_ctx.h), each run of slots starting from the state the previous one left.  Either cut leaves the bytes of
// one launch.  The host form stages a piece through for_each_chunk with a receiver as its unit; records and counts use the
// staging buffers of the messages path, the states (80 KB each) and the resolved records the context's scratch blocks 1 and 2
// (ensure_scratch).
#include "callhash.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr int kMaxSlots = 1 << 24;       // the kernel's election tags count the slots of a launch in 24 bits

}  // namespace

extern "C" {

int ft8gpu_resolve_calls(ft8gpu_ctx *c, const ft8gpu_message *msgs, const int32_t *n_msgs, int nstreams, int nslots,
                         ft8gpu_callhash_state *state, uint32_t max_age, ft8gpu_resolved *resolved, int flags) {
    if (!c) return ft8_fail("ctx is NULL");
    if (nstreams < 0 || nslots < 0) return ft8_fail("nstreams %d / nslots %d: negative", nstreams, nslots);
    if (nslots > kMaxSlots) return ft8_fail("nslots %d exceeds %d", nslots, kMaxSlots);
    Entry entry_(c);
    HIP_TRY(entry_.err);
    if (nstreams == 0 || nslots == 0) return 0;
    if (!msgs || !n_msgs || !state || !resolved) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)msgs | (uintptr_t)state | (uintptr_t)resolved) & 15) != 0)
        return ft8_fail("msgs, state and resolved must be 16-byte aligned");
    if (dev && ((uintptr_t)n_msgs & 3) != 0) return ft8_fail("n_msgs must be 4-byte aligned");
    const Pieces cut(nstreams, nslots, dev ? kNoBound : c->max_frames);      // the device form needs no staging: nothing bounds a piece
    if (!dev && (ensure_scratch(c, 0, (size_t)cut.rg_max * sizeof(ft8gpu_callhash_state),
                                   (size_t)cut.rg_max * cut.ns_max * kMaxMessages * sizeof(ft8gpu_resolved), 0) || ensure_msgs_staging(c)))
        return -1;
    return cut.each([&](int r0, int rg, int, int ns, size_t f0) {
        // slots at and above a frame's count keep the caller's bytes (resolved is uploaded in the host form)
        const StageArg a[] = { { msgs + f0 * kMaxMessages, c->d_msgs, (size_t)ns * kMaxMessages * sizeof(ft8gpu_message), kIn },
                               { n_msgs + f0, c->d_nres, (size_t)ns * sizeof(int32_t), kIn },
                               { state + r0, c->d_scratch[1], sizeof(ft8gpu_callhash_state), kInOut },
                               { resolved + f0 * kMaxMessages, c->d_scratch[2], (size_t)ns * kMaxMessages * sizeof(ft8gpu_resolved), kInOut } };
        return for_each_chunk(c, rg, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
            HIP_TRY(launch_callhash((const ft8gpu_message *)p[0], (const int32_t *)p[1], n, ns, (ft8gpu_callhash_state *)p[2],
                                    max_age, (ft8gpu_resolved *)p[3], c->stream));
            return 0;
        });
    });
}

int ft8gpu_decode_messages_resolved(ft8gpu_ctx *c, const float *iq, int nstreams, int nslots, const ft8gpu_ap_params *ap_params,
                                    ft8gpu_callhash_state *state, uint32_t max_age, ft8gpu_message *msgs, int32_t *n_msgs,
                                    ft8gpu_resolved *resolved, int flags) {
    if (!c) return ft8_fail("ctx is NULL");
    if (nstreams < 0 || nslots < 0) return ft8_fail("nstreams %d / nslots %d: negative", nstreams, nslots);
    if ((long long)nstreams * nslots > 0x7FFFFFFF) return ft8_fail("nstreams * nslots = %lld frames: too many", (long long)nstreams * nslots);
    if (nslots > kMaxSlots) return ft8_fail("nslots %d exceeds %d", nslots, kMaxSlots);
    if (nstreams == 0 || nslots == 0) return 0;
    if (!state || !resolved) return ft8_fail("NULL array argument");
    // both are entries of the ABI that take the context's mutex themselves; the resolve stage is ordered behind the decode on
    // the context's stream
    const int nframes = nstreams * nslots;
    const int rc = ap_params ? ft8gpu_decode_messages_ap(c, iq, nframes, ap_params, msgs, n_msgs, nullptr, flags)
                             : ft8gpu_decode_messages(c, iq, nframes, msgs, n_msgs, flags);
    if (rc) return rc;
    return ft8gpu_resolve_calls(c, msgs, n_msgs, nstreams, nslots, state, max_age, resolved, flags);
}

}  // extern "C"
