// api_match.hip -- host side of the expected messages: the stage entries ft8gpu_match_candidates and ft8gpu_expect_update
// and the whole path ft8gpu_decode_messages_expected (DESIGN.md "Expected messages"; the kernels are match.hip, the host
// helpers of the table are plain C in ft8_pack.c).
//
// Buffers.  The codewords of the tables (24 bytes per entry plus the live masks), the info records and the host form's
// staging of the states and of status_out live in the context's scratch blocks (ensure_scratch: 0 codewords, 1 states, 2 status_out, 3 info); they grow on the first call that
// needs them.  Everything else is the staging of the messages path.
//
// The slot-major whole path (decode_messages_slot_major; ft8gpu_decode_messages_combined of api_combine.hip runs on it too)
// cuts its [nstreams][nslots] frames into Pieces of at most max_frames frames.  A piece is gathered slot-major (all receivers of
// the piece's first slot, then of its second, ...), so that the front of the pipeline runs once over the piece and the
// slot-by-slot part -- here match, append, update, each one frame per receiver wide -- works on contiguous frames.  One slot per
// receiver (a daemon's call every 15 s) and one receiver are slot-major already: the device form then works on the caller's arrays.
#include "match.h"
#include "ft8gpu_ctx.h"

namespace {

constexpr int kMatchMaxHard = kLdpcN;

int check_match_args(int max_hard_errors) {
    if (max_hard_errors < 0 || max_hard_errors > kMatchMaxHard)
        return ft8_fail("max_hard_errors %d out of range [0, %d]", max_hard_errors, kMatchMaxHard);
    return 0;
}

// rows of `width` bytes between two arrays with different strides (host or device on either side)
hipError_t copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, int rows, hipStream_t s) {
    if (rows == 1 || (dpitch == width && spitch == width)) return hipMemcpyAsync(dst, src, width * rows, hipMemcpyDefault, s);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, (size_t)rows, hipMemcpyDefault, s);
}

}  // namespace

// The caller has checked its arguments and sized its scratch for Pieces(nstreams, nslots, max_frames).rg_max receivers; the
// host form stages the states (state_bytes each) in scratch block 1.  `slot` issues one slot's launches behind the pipeline; column 0
// of n_by_stage is the count in front of them, column 1 the count behind.
int decode_messages_slot_major(ft8gpu_ctx *c, const float *iq, int nstreams, int nslots, void *state, size_t state_bytes,
                               ft8gpu_message *msgs, int32_t *n_msgs, int32_t *n_by_stage, int flags, const SlotStages &slot) {
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    const size_t F = 2 * (size_t)kNSamples * sizeof(float), M = kMaxMessages * sizeof(ft8gpu_message), N = sizeof(int32_t);
    if (ensure_host_staging(c) || ensure_counts_staging(c)) return -1;
    hipStream_t s = c->stream;
    return Pieces(nstreams, nslots, c->max_frames).each([&](int r0, int rg, int s0, int ns, size_t f0) {
        char *user_st = (char *)state + r0 * state_bytes;
        void *st = dev ? user_st : c->d_scratch[1];
        if (!dev && s0 == 0) HIP_TRY(hipMemcpyAsync(st, user_st, rg * state_bytes, hipMemcpyHostToDevice, s));
        const int nfr = rg * ns;                                         // receiver r's slot t is frame f0 + r * nslots + t
        // A piece whose frames are consecutive in the caller's arrays (one receiver, or one slot per receiver) is slot-major
        // as it stands: the device form works on the caller's arrays.  Otherwise gather slot-major; slots past a frame's
        // count keep the caller's bytes, so msgs travels both ways.
        const bool direct = dev && (rg == 1 || nslots == 1);
        const float *piq = direct ? iq + f0 * 2 * (size_t)kNSamples : c->d_iq;
        ft8gpu_message *pm = direct ? msgs + f0 * kMaxMessages : c->d_msgs;
        int32_t *pn = direct ? n_msgs + f0 : c->d_nres;
        int32_t *pb = direct && n_by_stage ? n_by_stage + 2 * f0 : c->d_nbs;
        for (int t = 0; t < ns && !direct; ++t) {
            HIP_TRY(copy_rows((char *)c->d_iq + (size_t)t * rg * F, F, (const char *)iq + (f0 + t) * F, (size_t)nslots * F, F, rg, s));
            HIP_TRY(copy_rows((char *)c->d_msgs + (size_t)t * rg * M, M, (const char *)msgs + (f0 + t) * M, (size_t)nslots * M, M, rg, s));
        }
        if (run_pipeline_messages(c, piq, nfr, pm, pn)) return -1;
        HIP_TRY(hipMemcpy2DAsync(pb, 2 * N, pn, N, N, (size_t)nfr, hipMemcpyDeviceToDevice, s));
        for (int t = 0; t < ns; ++t) {
            const size_t o = (size_t)t * rg;
            if (slot(o, rg, st, pm + o * kMaxMessages, pn + o, pb + 2 * o)) return -1;
        }
        HIP_TRY(hipMemcpy2DAsync(pb + 1, 2 * N, pn, N, N, (size_t)nfr, hipMemcpyDeviceToDevice, s));
        for (int t = 0; t < ns && !direct; ++t) {
            const size_t o = (size_t)t * rg;
            HIP_TRY(copy_rows((char *)msgs + (f0 + t) * M, (size_t)nslots * M, (const char *)c->d_msgs + o * M, M, M, rg, s));
            HIP_TRY(copy_rows(n_msgs + f0 + t, (size_t)nslots * N, c->d_nres + o, N, N, rg, s));
            if (n_by_stage) HIP_TRY(copy_rows(n_by_stage + 2 * (f0 + t), (size_t)nslots * 2 * N, c->d_nbs + 2 * o, 2 * N, 2 * N, rg, s));
        }
        HIP_TRY(hipStreamSynchronize(s));                                // the staging buffers are free for the next piece
        if (!dev && s0 + ns == nslots) {
            HIP_TRY(hipMemcpyAsync(user_st, st, rg * state_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        return 0;
    });
}

extern "C" {

int ft8gpu_match_candidates(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status_in, int nframes, const ft8gpu_expect_state *states,
                            uint32_t max_age, int max_hard_errors, ft8gpu_decode_status *status_out, ft8gpu_match_info *info,
                            int flags) {
    CHECK_COMMON(c, nframes);
    if (check_match_args(max_hard_errors)) return -1;
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status_in || !states || !status_out || !info) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)states & 15) != 0) return ft8_fail("states must be 16-byte aligned");
    if (ensure_messages_buffers(c)) return -1;
    const int mc = c->params.max_candidates;
    const size_t piece = (size_t)(nframes < c->max_frames ? nframes : c->max_frames);
    if (ensure_scratch(c, piece * kExpectWorkBytes, dev ? 0 : piece * sizeof(ft8gpu_expect_state),
                          dev ? 0 : piece * mc * sizeof(ft8gpu_decode_status), dev ? 0 : piece * mc * sizeof(ft8gpu_match_info)))
        return -1;
    StageArg a[kCandRows + 1];
    cand_stage_rows(a, c, { mag, c->d_mag, kMagArray, kIn }, cands, counts, status_in, status_out, c->d_scratch[2], info, c->d_scratch[3],
                    sizeof(ft8gpu_match_info));
    a[kCandRows] = { states, c->d_scratch[1], sizeof(ft8gpu_expect_state), kIn };
    return for_each_chunk(c, nframes, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
        HIP_TRY(launch_expect_encode((const ft8gpu_expect_state *)p[kCandRows], n, max_age, c->d_msgtab, c->d_scratch[0], c->stream));
        HIP_TRY(launch_match((const uint8_t *)p[0], (const ft8gpu_candidate *)p[1], (const int32_t *)p[2],
                             (const ft8gpu_decode_status *)p[3], (ft8gpu_decode_status *)p[4], (ft8gpu_match_info *)p[5], n, mc,
                             c->d_scratch[0], max_hard_errors, c->stream));
        return 0;
    });
}

int ft8gpu_expect_update(ft8gpu_ctx *c, const ft8gpu_message *msgs, const int32_t *n_msgs, int nstreams, int nslots,
                         ft8gpu_expect_state *state, int derive, int flags) {
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
    if (!dev && (ensure_scratch(c, 0, (size_t)cut.rg_max * sizeof(ft8gpu_expect_state), 0, 0) || ensure_msgs_staging(c))) return -1;
    return cut.each([&](int r0, int rg, int, int ns, size_t f0) {
        const StageArg a[] = { { msgs + f0 * kMaxMessages, c->d_msgs, (size_t)ns * kMaxMessages * sizeof(ft8gpu_message), kIn },
                               { n_msgs + f0, c->d_nres, (size_t)ns * sizeof(int32_t), kIn },
                               { state + r0, c->d_scratch[1], sizeof(ft8gpu_expect_state), kInOut } };
        return for_each_chunk(c, rg, flags & FT8GPU_DEVICE_PTRS, a, [&](int n, void *const *p) {
            HIP_TRY(launch_expect_update((const ft8gpu_message *)p[0], (const int32_t *)p[1], n, ns, (ft8gpu_expect_state *)p[2],
                                         derive, c->stream));
            return 0;
        });
    });
}

int ft8gpu_decode_messages_expected(ft8gpu_ctx *c, const float *iq, int nstreams, int nslots, ft8gpu_expect_state *state,
                                    const ft8gpu_expect_params *params, ft8gpu_message *msgs, int32_t *n_msgs,
                                    int32_t *n_by_stage, int flags) {
    if (!c) return ft8_fail("ctx is NULL");
    if (nstreams < 0 || nslots < 0) return ft8_fail("nstreams %d / nslots %d: negative", nstreams, nslots);
    if ((long long)nstreams * nslots > 0x7FFFFFFF) return ft8_fail("nstreams * nslots = %lld frames: too many", (long long)nstreams * nslots);
    if (!params) return ft8_fail("params is NULL");
    if (check_match_args(params->max_hard_errors)) return -1;
    Entry entry_(c);
    HIP_TRY(entry_.err);
    if (nstreams == 0 || nslots == 0) return 0;
    if (!iq || !state || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && (((uintptr_t)msgs | (uintptr_t)state | (uintptr_t)iq) & 15) != 0) return ft8_fail("iq, msgs and state must be 16-byte aligned");
    if (ensure_messages_buffers(c)) return -1;
    const int mc = c->params.max_candidates, rg_max = Pieces(nstreams, nslots, c->max_frames).rg_max;
    if (ensure_scratch(c, (size_t)rg_max * kExpectWorkBytes, dev ? 0 : (size_t)rg_max * sizeof(ft8gpu_expect_state), 0,
                          (size_t)rg_max * mc * sizeof(ft8gpu_match_info)))
        return -1;
    const int gate = params->max_hard_errors, derive = params->derive;
    const uint32_t max_age = params->max_age;
    hipStream_t s = c->stream;
    return decode_messages_slot_major(c, iq, nstreams, nslots, state, sizeof(ft8gpu_expect_state), msgs, n_msgs, n_by_stage, flags,
                                      [=](size_t o, int rg, void *st, ft8gpu_message *dm, int32_t *pn, int32_t *pb) {
        ft8gpu_expect_state *states = (ft8gpu_expect_state *)st;
        ft8gpu_decode_status *status = c->d_status + o * mc;
        HIP_TRY(launch_expect_encode(states, rg, max_age, c->d_msgtab, c->d_scratch[0], s));
        HIP_TRY(launch_match(c->d_mag + o * kMagArray, c->d_cands + o * mc, c->d_counts + o, status, status,
                             (ft8gpu_match_info *)c->d_scratch[3], rg, mc, c->d_scratch[0], gate, s));
        HIP_TRY(launch_append(c->d_mag + o * kMagArray, c->d_base + o * 2 * kNumBin, c->d_cands + o * mc, c->d_counts + o, status,
                              c->d_msgtab, nullptr, rg, mc, c->params.min_score, dm, pn, s));
        HIP_TRY(launch_match_tag(pb, 2, pn, rg, dm, s));
        HIP_TRY(launch_expect_update(dm, pn, rg, 1, states, derive, s));
        return 0;
    });
}

}  // extern "C"
