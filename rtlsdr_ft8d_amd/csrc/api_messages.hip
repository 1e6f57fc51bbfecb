// api_messages.hip -- host side of the messages path: the constant tables of the SNR estimate, the lazily allocated
// buffers, and the stage entries ft8gpu_noise_baseline / ft8gpu_collect_messages (ft8gpu_decode_messages, the whole path,
// lives beside ft8gpu_decode_batch in api_pipeline.hip).
#include "ft8gpu_ctx.h"
#include "ft8_tables.h"

#include <math.h>

namespace {

// Calibration constant K of the SNR estimate: the median of (estimate - truth) over synthesised decodes, measured by
// tools/snr_calibrate.py and recorded in profiles/snr_calibration.json (tests/test_messages_cpu.py holds the two equal).
constexpr double kSnrCalibrationK = 25.16;

// P[v] = 10^((v - 240) / 20): byte v = 2 dB + 240 back to power; T[d] = (1 + 10^((d - 0.5 + K) / 10)) / q with
// q = -ln(0.75), the 25th percentile of exponential noise power in units of its mean.  libm's pow / log, as the numpy
// restatement (tests/ft8_spec_messages.py, math.pow / math.log) evaluates them.
int build_msg_tables(MsgTables *t) {
    for (int v = 0; v < 256; ++v) t->power[v] = pow(10.0, (double)(v - 240) / 20.0);
    const double q = -log(0.75);
    for (int d = kSnrMin; d <= kSnrMax; ++d) t->thr[d - kSnrMin] = (1.0 + pow(10.0, ((double)d - 0.5 + kSnrCalibrationK) / 10.0)) / q;
    for (int m = 0; m < kLdpcM; ++m)
        for (int w = 0; w < 3; ++w)
            t->gen[m][w] = (uint32_t)kFT8_generator[m][4 * w] << 24 | (uint32_t)kFT8_generator[m][4 * w + 1] << 16 |
                           (uint32_t)kFT8_generator[m][4 * w + 2] << 8 | (uint32_t)kFT8_generator[m][4 * w + 3];
    return 0;
}

}  // namespace

// the noise baseline buffer and the tables, on the first messages call (ft8gpu_create's footprint is unchanged)
int ensure_messages_buffers(ft8gpu_ctx *c) {
    if (c->mem.once(&c->d_base, (size_t)c->max_frames * 2 * kNumBin, "the noise baseline")) return -1;
    return c->mem.table(&c->d_msgtab, "the SNR tables", build_msg_tables);
}

extern "C" {

int ft8gpu_noise_baseline(ft8gpu_ctx *c, const uint8_t *mag, int nframes, uint8_t *base, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !base) return ft8_fail("NULL array argument");
    if (ensure_messages_buffers(c)) return -1;
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { base, c->d_base, 2 * kNumBin, kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_noise_baseline((const uint8_t *)p[0], (uint8_t *)p[1], n, c->stream));
        return 0;
    });
}

int ft8gpu_collect_messages(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status, int nframes, ft8gpu_message *msgs, int32_t *n_msgs, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    if (ensure_messages_buffers(c)) return -1;
    const int mc = c->params.max_candidates;
    if (!(flags & FT8GPU_DEVICE_PTRS) && ensure_msgs_staging(c)) return -1;
    // slots past a frame's count keep the caller's bytes; c->d_base is scratch in both forms
    const StageArg a[] = { { mag, c->d_mag, kMagArray, kIn }, { cands, c->d_cands, mc * sizeof(ft8gpu_candidate), kIn },
                           { counts, c->d_counts, sizeof(int32_t), kIn }, { status, c->d_status, mc * sizeof(ft8gpu_decode_status), kIn },
                           { msgs, c->d_msgs, kMaxMessages * sizeof(ft8gpu_message), kInOut }, { n_msgs, c->d_nres, sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_noise_baseline((const uint8_t *)p[0], c->d_base, n, c->stream));
        HIP_TRY(launch_messages((const uint8_t *)p[0], c->d_base, (const ft8gpu_candidate *)p[1], (const int32_t *)p[2],
                                (const ft8gpu_decode_status *)p[3], c->d_msgtab, n, mc, c->params.min_score, (ft8gpu_message *)p[4],
                                (int32_t *)p[5], c->stream));
        return 0;
    });
}

}  // extern "C"
