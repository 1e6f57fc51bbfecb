// api_demod.hip -- host side of the demodulation from the I/Q samples and of AP on its soft bits: the stage entries
// ft8gpu_demod_candidates, ft8gpu_demod_soft and ft8gpu_ap_soft_candidates, and the whole paths ft8gpu_decode_messages_demod
// and ft8gpu_decode_messages_demod_ap (DESIGN.md "Demodulation from the I/Q samples", "A-priori decoding on the demodulated
// soft bits"; the kernels are demod.hip and apsoft.hip).
//
// Every entry cuts the frames with for_each_chunk.  Everything beyond the messages path lives in the context's scratch
// blocks (ensure_scratch), which no other entry uses while this one holds the context's mutex: the info records of the
// demodulation (block 3) and of AP (1), the host form's staging of status_out (2), the whole paths' counts before an append
// step (0).  The soft-bit array of a chunk is the context's d_soft (ensure_soft): the whole path's intermediate and the host
// form's staging of `soft`.  w4 is the subtraction's table.
#include "apsoft.h"
#include "demod.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr size_t kFrameBytes = 2 * (size_t)kNSamples * sizeof(float);
constexpr size_t kMsgBytes = kMaxMessages * sizeof(ft8gpu_message);
constexpr size_t kSoftBytes = 3 * (size_t)FT8GPU_SOFT_STRIDE * sizeof(float);     // per candidate
static_assert(kSoftBytes == 2112 && kSoftBytes % 16 == 0, "soft rows");

int check_demod_args(const ft8gpu_ctx *c, const ft8gpu_demod_params *p) {
    if (!p) return ft8_fail("params is NULL");
    if (p->sets < 1 || p->sets > 7) return ft8_fail("sets %d out of range [1, 7]", p->sets);
    if (p->max_hard_errors < 0 || p->max_hard_errors > kLdpcN)
        return ft8_fail("max_hard_errors %d out of range [0, %d]", p->max_hard_errors, kLdpcN);
    if (p->max_per_frame < 0 || p->max_per_frame > c->params.max_candidates)
        return ft8_fail("max_per_frame %d out of range [0, %d]", p->max_per_frame, c->params.max_candidates);
    return 0;
}

// the kernels' constant tables, on the context's first call
int ensure_demod_tables(ft8gpu_ctx *c) {
    if (ensure_subtract_tables(c)) return -1;
    return tables_once(c, &c->demod_tables, demod_tables_init);
}

// the soft-bit array of `frames` frames at the context's max_candidates, through the context's owner.  The old block goes
// first (CtxMem::grow: two of them need not fit), so a failed allocation leaves d_soft null and soft_cap 0, the error text
// set, and everything else of the context as it was; the next call allocates again.
int ensure_soft(ft8gpu_ctx *c, size_t frames) {
    const size_t need = frames * (size_t)c->params.max_candidates * kSoftBytes;
    if (need <= c->soft_cap) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));                       // the old block may still be in use
    return c->mem.grow(&c->d_soft, &c->soft_cap, need, "the soft bits of a chunk");
}

// ft8gpu_demod_candidates, and with want_soft ft8gpu_demod_soft
int demod_stage(ft8gpu_ctx *c, const float *iq, const ft8gpu_candidate *cands, const int32_t *counts,
                const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_demod_params *params,
                ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, float *soft, bool want_soft, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_demod_args(c, params)) return -1;
    if (nframes == 0) return 0;
    if (!iq || !cands || !counts || !status_in || !status_out || !info || (want_soft && !soft)) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)iq & 15) != 0) return ft8_fail("iq must be 16-byte aligned");
    if (dev && want_soft && ((uintptr_t)soft & 15) != 0) return ft8_fail("soft must be 16-byte aligned");
    if (ensure_messages_buffers(c) || ensure_demod_tables(c)) return -1;
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (!dev && ensure_host_staging(c)) return -1;
    if (ensure_scratch(c, 0, 0, dev ? 0 : piece * mc * sizeof(ft8gpu_decode_status), dev ? 0 : piece * mc * sizeof(ft8gpu_demod_info)))
        return -1;
    if (want_soft && !dev && ensure_soft(c, piece)) return -1;
    const ft8gpu_demod_params p = *params;
    // rows at and behind a frame's count keep the caller's bytes: soft is uploaded in the host form, as the records are
    StageArg a[kCandRows + 1];
    cand_stage_rows(a, c, { iq, c->d_iq, kFrameBytes, kIn }, cands, counts, status_in, status_out, c->d_scratch[2], info, c->d_scratch[3],
                    sizeof(ft8gpu_demod_info));
    a[kCandRows] = { want_soft ? soft : nullptr, c->d_soft, mc * kSoftBytes, kInOut };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *q) {
        HIP_TRY(launch_demod((const float *)q[0], (const ft8gpu_candidate *)q[1], (const int32_t *)q[2],
                             (const ft8gpu_decode_status *)q[3], (ft8gpu_decode_status *)q[4], (ft8gpu_demod_info *)q[5],
                             (float *)q[kCandRows], n, mc, c->d_subtab, p.sets, p.max_hard_errors, p.max_per_frame,
                             c->params.ldpc_iters, force_ieee(c), c->stream));
        return 0;
    });
}

// ft8gpu_decode_messages_demod (ap == nullptr: two columns), and ft8gpu_decode_messages_demod_ap (three; AP runs with nhyp > 0)
int demod_whole_path(ft8gpu_ctx *c, const float *iq, int nframes, const ft8gpu_demod_params *params, const ft8gpu_demod_ap_params *ap,
                     ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags) {
    CHECK_COMMON(c, nframes);
    if (check_demod_args(c, params)) return -1;
    const int nhyp = ap ? ap->nhyp : 0, cols = ap ? 3 : 2;
    if (nhyp < 0 || nhyp > FT8GPU_AP_MAX_HYPOTHESES) return ft8_fail("nhyp %d out of range [0, %d]", nhyp, FT8GPU_AP_MAX_HYPOTHESES);
    if (nhyp > 0 && check_ap_args(ap->hyps, nhyp, ap->ap_max_hard_errors)) return -1;
    if (nframes == 0) return 0;
    if (!iq || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)iq | (uintptr_t)msgs) & 15) != 0) return ft8_fail("iq and msgs must be 16-byte aligned");
    if (ensure_messages_buffers(c) || ensure_demod_tables(c)) return -1;
    if (!dev && (ensure_host_staging(c) || (n_by_stage && ensure_counts_staging(c)))) return -1;
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (ensure_scratch(c, piece * sizeof(int32_t), nhyp > 0 ? piece * mc * sizeof(ft8gpu_apsoft_info) : 0, 0,
                       piece * mc * sizeof(ft8gpu_demod_info)))
        return -1;
    if (nhyp > 0 && (tables_once(c, &c->apsoft_tables, apsoft_tables_init) || ensure_soft(c, piece))) return -1;
    const ft8gpu_demod_params p = *params;
    // slots past a frame's count keep the caller's bytes (msgs is uploaded in the host form)
    const StageArg a[] = { { iq, c->d_iq, kFrameBytes, kIn }, { msgs, c->d_msgs, kMsgBytes, kInOut },
                           { n_msgs, c->d_nres, sizeof(int32_t), kOut }, { n_by_stage, c->d_nbs, cols * sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *q) {
        const float *x = (const float *)q[0];
        ft8gpu_message *dm = (ft8gpu_message *)q[1];
        int32_t *pn = (int32_t *)q[2], *pb = (int32_t *)q[3], *before = (int32_t *)c->d_scratch[0];
        ft8gpu_demod_info *inf = (ft8gpu_demod_info *)c->d_scratch[3];
        if (run_pipeline_messages(c, x, n, dm, pn)) return -1;
        if (pb) HIP_TRY(launch_pass_counts(pn, pb, n, cols, 0, c->stream));
        HIP_TRY(hipMemcpyAsync(before, pn, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(launch_demod(x, c->d_cands, c->d_counts, c->d_status, c->d_status, inf, nhyp > 0 ? c->d_soft : nullptr, n, mc,
                             c->d_subtab, p.sets, p.max_hard_errors, p.max_per_frame, c->params.ldpc_iters, force_ieee(c), c->stream));
        HIP_TRY(launch_append(c->d_mag, c->d_base, c->d_cands, c->d_counts, c->d_status, c->d_msgtab, nullptr, n, mc, c->params.min_score,
                              dm, pn, c->stream));
        HIP_TRY(launch_demod_tag(before, pn, n, inf, mc, dm, c->stream));
        if (pb) HIP_TRY(launch_pass_counts(pn, pb, n, cols, 1, c->stream));
        if (nhyp < 1) return 0;
        // AP on the soft bits of what is still undecoded, in place; `before` is free again behind the tag launch
        ft8gpu_apsoft_info *ainf = (ft8gpu_apsoft_info *)c->d_scratch[1];
        HIP_TRY(hipMemcpyAsync(before, pn, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(launch_ap_soft(c->d_soft, c->d_counts, c->d_status, c->d_status, ainf, n, mc, c->params.ldpc_iters, force_ieee(c), p.sets,
                               ap->hyps, nhyp, ap->ap_max_hard_errors, c->stream));
        HIP_TRY(launch_append(c->d_mag, c->d_base, c->d_cands, c->d_counts, c->d_status, c->d_msgtab, nullptr, n, mc, c->params.min_score,
                              dm, pn, c->stream));
        HIP_TRY(launch_ap_soft_tag(before, pn, n, ainf, mc, dm, c->stream));
        if (pb) HIP_TRY(launch_pass_counts(pn, pb, n, cols, 2, c->stream));
        return 0;
    });
}

}  // namespace

extern "C" {

int ft8gpu_demod_candidates(ft8gpu_ctx *c, const float *iq, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_demod_params *params,
                            ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, int flags) {
    return demod_stage(c, iq, cands, counts, status_in, nframes, params, status_out, info, nullptr, false, flags);
}

int ft8gpu_demod_soft(ft8gpu_ctx *c, const float *iq, const ft8gpu_candidate *cands, const int32_t *counts,
                      const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_demod_params *params,
                      ft8gpu_decode_status *status_out, ft8gpu_demod_info *info, float *soft, int flags) {
    return demod_stage(c, iq, cands, counts, status_in, nframes, params, status_out, info, soft, true, flags);
}

int ft8gpu_ap_soft_candidates(ft8gpu_ctx *c, const float *soft, const int32_t *counts, const ft8gpu_decode_status *status_in,
                              int nframes, int sets, const ft8gpu_ap_hypothesis *hyps, int nhyp, int max_hard_errors,
                              ft8gpu_decode_status *status_out, ft8gpu_apsoft_info *info, int flags) {
    CHECK_COMMON(c, nframes);
    if (sets < 1 || sets > 7) return ft8_fail("sets %d out of range [1, 7]", sets);
    if (check_ap_args(hyps, nhyp, max_hard_errors)) return -1;
    if (nframes == 0) return 0;
    if (!soft || !counts || !status_in || !status_out || !info) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)soft & 15) != 0) return ft8_fail("soft must be 16-byte aligned");
    if (tables_once(c, &c->apsoft_tables, apsoft_tables_init)) return -1;
    const size_t mc = (size_t)c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (!dev && (ensure_scratch(c, 0, piece * mc * sizeof(ft8gpu_apsoft_info), piece * mc * sizeof(ft8gpu_decode_status), 0) ||
                 ensure_soft(c, piece)))
        return -1;
    // both outputs are uploaded in the host form: records at and behind a frame's count keep the caller's bytes
    const StageArg a[] = { { soft, c->d_soft, mc * kSoftBytes, kIn },
                           { counts, c->d_counts, sizeof(int32_t), kIn },
                           { status_in, c->d_status, mc * sizeof(ft8gpu_decode_status), kIn },
                           { status_out, c->d_scratch[2], mc * sizeof(ft8gpu_decode_status), kInOut },
                           { info, c->d_scratch[1], mc * sizeof(ft8gpu_apsoft_info), kInOut } };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *q) {
        HIP_TRY(launch_ap_soft((const float *)q[0], (const int32_t *)q[1], (const ft8gpu_decode_status *)q[2],
                               (ft8gpu_decode_status *)q[3], (ft8gpu_apsoft_info *)q[4], n, (int)mc, c->params.ldpc_iters, force_ieee(c),
                               sets, hyps, nhyp, max_hard_errors, c->stream));
        return 0;
    });
}

int ft8gpu_decode_messages_demod(ft8gpu_ctx *c, const float *iq, int nframes, const ft8gpu_demod_params *params,
                                 ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags) {
    return demod_whole_path(c, iq, nframes, params, nullptr, msgs, n_msgs, n_by_stage, flags);
}

int ft8gpu_decode_messages_demod_ap(ft8gpu_ctx *c, const float *iq, int nframes, const ft8gpu_demod_ap_params *params,
                                    ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags) {
    if (c && !params) return ft8_fail("params is NULL");
    return demod_whole_path(c, iq, nframes, params ? &params->demod : nullptr, params, msgs, n_msgs, n_by_stage, flags);
}

}  // extern "C"
