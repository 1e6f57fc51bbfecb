// api_combine.hip -- host side of the soft-bit memory: the stage entries ft8gpu_combine_candidates and ft8gpu_softmem_update
// and the whole path ft8gpu_decode_messages_combined (DESIGN.md "Soft-bit memory"; the kernels are combine.hip, the reset
// of a state is plain C in ft8_pack.c).
//
// Buffers.  As for the expected messages, everything this file needs beyond the messages path lives in the context's
// scratch blocks (ensure_scratch): the update kernel's read-only copy of the entry states (block 0), the host form's staging of
// the states (1) and of status_out (2), the info records (3).  A state is 92 176 bytes, so a call over n receivers
// needs n of them once or twice; they grow on the first call that needs them.
//
// Update.  The rule forms every sum from the state as it was at entry to the slot, while the ring may overwrite a partner in
// the same slot.  The kernel therefore never reads what it writes: the states are copied (device to device), the kernel reads
// the copy and writes the entries it stores, cursor and slot into the states themselves.
//
// The whole path is the slot-major one of api_match.hip (decode_messages_slot_major) with combine, append, update as the
// slot-by-slot part.
#include "combine.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr size_t kStateBytes = sizeof(ft8gpu_softmem_state);

int check_combine_args(int min_agree, int store_per_slot) {
    if (min_agree < 0 || min_agree > kLdpcN) return ft8_fail("min_agree %d out of range [0, %d]", min_agree, kLdpcN);
    if (store_per_slot < 0 || store_per_slot > kSoftmemEntries)
        return ft8_fail("store_per_slot %d out of range [0, %d]", store_per_slot, kSoftmemEntries);
    return 0;
}

// the kernels' constant tables, on the context's first call
int ensure_combine_tables(ft8gpu_ctx *c) {
    return tables_once(c, &c->combine_tables, combine_tables_init);
}

// one slot of n receivers: states (device memory) in-out, through the read-only copy in the context's buffer
int update_slot(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                const ft8gpu_decode_status *status, const ft8gpu_combine_info *info, int n, ft8gpu_softmem_state *states,
                int store_per_slot) {
    HIP_TRY(hipMemcpyAsync(c->d_scratch[0], states, (size_t)n * kStateBytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(launch_softmem_update(mag, cands, counts, status, info, n, c->params.max_candidates,
                                  (const ft8gpu_softmem_state *)c->d_scratch[0], states, store_per_slot, c->stream));
    return 0;
}

}  // namespace

extern "C" {

int ft8gpu_combine_candidates(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                              const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_softmem_state *states,
                              uint32_t max_age, int min_agree, ft8gpu_decode_status *status_out, ft8gpu_combine_info *info,
                              int flags) {
    CHECK_COMMON(c, nframes);
    if (check_combine_args(min_agree, 0)) return -1;
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status_in || !states || !status_out || !info) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)states & 15) != 0) return ft8_fail("states must be 16-byte aligned");
    if (ensure_messages_buffers(c) || ensure_combine_tables(c)) return -1;
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (ensure_scratch(c, 0, dev ? 0 : piece * kStateBytes, dev ? 0 : piece * mc * sizeof(ft8gpu_decode_status),
                          dev ? 0 : piece * mc * sizeof(ft8gpu_combine_info)))
        return -1;
    StageArg a[kCandRows + 1];
    cand_stage_rows(a, c, { mag, c->d_mag, kMagArray, kIn }, cands, counts, status_in, status_out, c->d_scratch[2], info, c->d_scratch[3],
                    sizeof(ft8gpu_combine_info));
    a[kCandRows] = { states, c->d_scratch[1], kStateBytes, kIn };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        HIP_TRY(launch_combine((const uint8_t *)p[0], (const ft8gpu_candidate *)p[1], (const int32_t *)p[2],
                               (const ft8gpu_decode_status *)p[3], (ft8gpu_decode_status *)p[4], (ft8gpu_combine_info *)p[5], n, mc,
                               (const ft8gpu_softmem_state *)p[kCandRows], max_age, min_agree, c->params.ldpc_iters, force_ieee(c),
                               c->stream));
        return 0;
    });
}

int ft8gpu_softmem_update(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                          const ft8gpu_decode_status *status, const ft8gpu_combine_info *info, int nframes,
                          ft8gpu_softmem_state *states, int store_per_slot, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_combine_args(0, store_per_slot)) return -1;
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status || !info || !states) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)states & 15) != 0) return ft8_fail("states must be 16-byte aligned");
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (ensure_scratch(c, piece * kStateBytes, dev ? 0 : piece * kStateBytes, 0, dev ? 0 : piece * mc * sizeof(ft8gpu_combine_info)))
        return -1;
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kIn },
                           { counts, c->d_counts, sizeof(int32_t), kIn },
                           { status, c->d_status, mc * sizeof(ft8gpu_decode_status), kIn },
                           { info, c->d_scratch[3], mc * sizeof(ft8gpu_combine_info), kIn },
                           { states, c->d_scratch[1], kStateBytes, kInOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        return update_slot(c, (const uint8_t *)p[0], (const ft8gpu_candidate *)p[1], (const int32_t *)p[2],
                           (const ft8gpu_decode_status *)p[3], (const ft8gpu_combine_info *)p[4], n, (ft8gpu_softmem_state *)p[5],
                           store_per_slot);
    });
}

int ft8gpu_decode_messages_combined(ft8gpu_ctx *c, const float *iq, int nstreams, int nslots, ft8gpu_softmem_state *state,
                                    const ft8gpu_combine_params *params, ft8gpu_message *msgs, int32_t *n_msgs,
                                    int32_t *n_by_stage, int flags) {
    if (!c) return ft8_fail("ctx is NULL");
    if (nstreams < 0 || nslots < 0) return ft8_fail("nstreams %d / nslots %d: negative", nstreams, nslots);
    if ((long long)nstreams * nslots > 0x7FFFFFFF) return ft8_fail("nstreams * nslots = %lld frames: too many", (long long)nstreams * nslots);
    if (!params) return ft8_fail("params is NULL");
    if (check_combine_args(params->min_agree, params->store_per_slot)) return -1;
    Entry entry_(c);
    HIP_TRY(entry_.err);
    if (nstreams == 0 || nslots == 0) return 0;
    if (!iq || !state || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)msgs | (uintptr_t)state | (uintptr_t)iq) & 15) != 0) return ft8_fail("iq, msgs and state must be 16-byte aligned");
    if (ensure_messages_buffers(c) || ensure_combine_tables(c)) return -1;
    const int mc = c->params.max_candidates, rg_max = Pieces(nstreams, nslots, c->max_frames).rg_max;
    if (ensure_scratch(c, (size_t)rg_max * kStateBytes, dev ? 0 : (size_t)rg_max * kStateBytes, 0,
                          (size_t)rg_max * mc * sizeof(ft8gpu_combine_info)))
        return -1;
    const int gate = params->min_agree, store = params->store_per_slot;
    const uint32_t max_age = params->max_age;
    hipStream_t s = c->stream;
    return decode_messages_slot_major(c, iq, nstreams, nslots, state, kStateBytes, msgs, n_msgs, n_by_stage, flags,
                                      [=](size_t o, int rg, void *st, ft8gpu_message *dm, int32_t *pn, int32_t *pb) {
        ft8gpu_softmem_state *states = (ft8gpu_softmem_state *)st;
        ft8gpu_decode_status *status = c->d_status + o * mc;
        ft8gpu_combine_info *inf = (ft8gpu_combine_info *)c->d_scratch[3];
        HIP_TRY(launch_combine(c->d_mag + o * kMagArray, c->d_cands + o * mc, c->d_counts + o, status, status, inf, rg, mc, states,
                               max_age, gate, c->params.ldpc_iters, force_ieee(c), s));
        HIP_TRY(launch_append(c->d_mag + o * kMagArray, c->d_base + o * 2 * kNumBin, c->d_cands + o * mc, c->d_counts + o, status,
                              c->d_msgtab, nullptr, rg, mc, c->params.min_score, dm, pn, s));
        HIP_TRY(launch_combine_tag(pb, 2, pn, rg, dm, s));
        return update_slot(c, c->d_mag + o * kMagArray, c->d_cands + o * mc, c->d_counts + o, status, inf, rg, states, store);
    });
}

}  // extern "C"
