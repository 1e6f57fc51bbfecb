// api_hint.hip -- host side of the call hints: the stage entries ft8gpu_hint_candidates and ft8gpu_hint_update and the whole
// path ft8gpu_decode_messages_hinted, the third user of the slot-major walk (api_match.hip; DESIGN.md "Call hints"; the
// kernels are hint.hip, the host helpers of the table are plain C in ft8_hint.c).
//
// Buffers.  The info records and the host form's staging of the states and of status_out live in the context's scratch blocks
// (ensure_scratch: 0 the encoded tables, 4 KB per frame; 1 states, 2 status_out, 3 info).
#include "hint.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr int kHintMaxHard = kLdpcN;

// the encoded tables want scratch block 0 (hint.h); the A/B build's other form converts in the wave and wants none
size_t hint_work_bytes(const ft8gpu_ctx *c) {
#ifdef FT8GPU_AB_FORMS
    if (c->debug_flags & FT8GPU_AB_HINT_IN_WAVE) return 0;
#endif
    (void)c;
    return kHintWorkBytes;
}

int check_hint_args(const ft8gpu_hint_params *q) {
    if (!q) return ft8_fail("params is NULL");
    if (q->tries < 1 || q->tries > FT8GPU_AP_MAX_HYPOTHESES) return ft8_fail("tries %d out of range [1, %d]", q->tries, FT8GPU_AP_MAX_HYPOTHESES);
    if (q->max_bad_per_64 < 0 || q->max_bad_per_64 > 64) return ft8_fail("max_bad_per_64 %d out of range [0, 64]", q->max_bad_per_64);
    if (q->max_hard_errors < 0 || q->max_hard_errors > kHintMaxHard)
        return ft8_fail("max_hard_errors %d out of range [0, %d]", q->max_hard_errors, kHintMaxHard);
    return 0;
}

}  // namespace

extern "C" {

int ft8gpu_hint_candidates(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                           const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_hint_state *states,
                           const ft8gpu_hint_params *params, ft8gpu_decode_status *status_out, ft8gpu_hint_info *info, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_hint_args(params)) return -1;
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status_in || !states || !status_out || !info) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)states & 15) != 0) return ft8_fail("states must be 16-byte aligned");
    if (tables_once(c, &c->hint_tables, hint_tables_init)) return -1;
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    const size_t wb = hint_work_bytes(c);
    if (ensure_scratch(c, piece * wb, dev ? 0 : piece * sizeof(ft8gpu_hint_state), dev ? 0 : piece * mc * sizeof(ft8gpu_decode_status),
                          dev ? 0 : piece * mc * sizeof(ft8gpu_hint_info)))
        return -1;
    const ft8gpu_hint_params q = *params;
    StageArg a[kCandRows + 1];
    cand_stage_rows(a, c, { mag, c->d_mag, kMagArray, kIn }, cands, counts, status_in, status_out, c->d_scratch[2], info, c->d_scratch[3],
                    sizeof(ft8gpu_hint_info));
    a[kCandRows] = { states, c->d_scratch[1], sizeof(ft8gpu_hint_state), kIn };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        HIP_TRY(launch_hint((const uint8_t *)p[0], (const ft8gpu_candidate *)p[1], (const int32_t *)p[2],
                            (const ft8gpu_decode_status *)p[3], (ft8gpu_decode_status *)p[4], (ft8gpu_hint_info *)p[5], n, mc,
                            c->params.ldpc_iters, force_ieee(c), (const ft8gpu_hint_state *)p[kCandRows], q, wb ? c->d_scratch[0] : nullptr,
                            c->stream));
        return 0;
    });
}

int ft8gpu_hint_update(ft8gpu_ctx *c, const ft8gpu_message *msgs, const int32_t *n_msgs, int nstreams, int nslots,
                       ft8gpu_hint_state *state, int flags) {
    if (!c) return ft8_fail("ctx is NULL");
    if (nstreams < 0 || nslots < 0) return ft8_fail("nstreams %d / nslots %d: negative", nstreams, nslots);
    Entry entry_(c);
    HIP_TRY(entry_.err);
    if (nstreams == 0 || nslots == 0) return 0;
    if (!msgs || !n_msgs || !state) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)msgs | (uintptr_t)state) & 15) != 0) return ft8_fail("msgs and state must be 16-byte aligned");
    if (dev && ((uintptr_t)n_msgs & 3) != 0) return ft8_fail("n_msgs must be 4-byte aligned");
    const Pieces cut(nstreams, nslots, dev ? kNoBound : c->max_frames);      // nothing bounds a piece in the device form
    if (!dev && (ensure_scratch(c, 0, (size_t)cut.rg_max * sizeof(ft8gpu_hint_state), 0, 0) || ensure_msgs_staging(c))) return -1;
    return cut.each([&](int r0, int rg, int, int ns, size_t f0) {
        const StageArg a[] = { { msgs + f0 * kMaxMessages, c->d_msgs, (size_t)ns * kMaxMessages * sizeof(ft8gpu_message), kIn },
                               { n_msgs + f0, c->d_nres, (size_t)ns * sizeof(int32_t), kIn },
                               { state + r0, c->d_scratch[1], sizeof(ft8gpu_hint_state), kInOut } };
        return for_each_chunk(c, rg, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
            HIP_TRY(launch_hint_update((const ft8gpu_message *)p[0], (const int32_t *)p[1], n, ns, (ft8gpu_hint_state *)p[2], c->stream));
            return 0;
        });
    });
}

int ft8gpu_decode_messages_hinted(ft8gpu_ctx *c, const float *iq, int nstreams, int nslots, ft8gpu_hint_state *state,
                                  const ft8gpu_hint_params *params, ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage,
                                  int flags) {
    if (!c) return ft8_fail("ctx is NULL");
    if (nstreams < 0 || nslots < 0) return ft8_fail("nstreams %d / nslots %d: negative", nstreams, nslots);
    if ((long long)nstreams * nslots > 0x7FFFFFFF) return ft8_fail("nstreams * nslots = %lld frames: too many", (long long)nstreams * nslots);
    if (check_hint_args(params)) return -1;
    Entry entry_(c);
    HIP_TRY(entry_.err);
    if (nstreams == 0 || nslots == 0) return 0;
    if (!iq || !state || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)msgs | (uintptr_t)state | (uintptr_t)iq) & 15) != 0) return ft8_fail("iq, msgs and state must be 16-byte aligned");
    if (ensure_messages_buffers(c)) return -1;
    if (tables_once(c, &c->hint_tables, hint_tables_init)) return -1;
    const int mc = c->params.max_candidates, rg_max = Pieces(nstreams, nslots, c->max_frames).rg_max;
    const size_t wb = hint_work_bytes(c);
    if (ensure_scratch(c, (size_t)rg_max * wb, dev ? 0 : (size_t)rg_max * sizeof(ft8gpu_hint_state), 0, (size_t)rg_max * mc * sizeof(ft8gpu_hint_info)))
        return -1;
    const ft8gpu_hint_params q = *params;
    hipStream_t s = c->stream;
    return decode_messages_slot_major(c, iq, nstreams, nslots, state, sizeof(ft8gpu_hint_state), msgs, n_msgs, n_by_stage, flags,
                                      [=](size_t o, int rg, void *st, ft8gpu_message *dm, int32_t *pn, int32_t *pb) {
        ft8gpu_hint_state *states = (ft8gpu_hint_state *)st;
        ft8gpu_decode_status *status = c->d_status + o * mc;
        HIP_TRY(launch_hint(c->d_mag + o * kMagArray, c->d_cands + o * mc, c->d_counts + o, status, status,
                            (ft8gpu_hint_info *)c->d_scratch[3], rg, mc, c->params.ldpc_iters, force_ieee(c), states, q,
                            wb ? c->d_scratch[0] : nullptr, s));
        HIP_TRY(launch_append(c->d_mag + o * kMagArray, c->d_base + o * 2 * kNumBin, c->d_cands + o * mc, c->d_counts + o, status,
                              c->d_msgtab, nullptr, rg, mc, c->params.min_score, dm, pn, s));
        HIP_TRY(launch_hint_tag(pb, 2, pn, rg, dm, s));
        HIP_TRY(launch_hint_update(dm, pn, rg, 1, states, s));
        return 0;
    });
}

}  // extern "C"
