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
void build_msg_tables(MsgTables *t) {
    for (int v = 0; v < 256; ++v) t->power[v] = pow(10.0, (double)(v - 240) / 20.0);
    const double q = -log(0.75);
    for (int d = kSnrMin; d <= kSnrMax; ++d) t->thr[d - kSnrMin] = (1.0 + pow(10.0, ((double)d - 0.5 + kSnrCalibrationK) / 10.0)) / q;
    for (int m = 0; m < kLdpcM; ++m)
        for (int w = 0; w < 3; ++w)
            t->gen[m][w] = (uint32_t)kFT8_generator[m][4 * w] << 24 | (uint32_t)kFT8_generator[m][4 * w + 1] << 16 |
                           (uint32_t)kFT8_generator[m][4 * w + 2] << 8 | (uint32_t)kFT8_generator[m][4 * w + 3];
}

}  // namespace

// the noise baseline buffer and the tables, on the first messages call (ft8gpu_create's footprint is unchanged)
int ensure_messages_buffers(ft8gpu_ctx *c) {
    if (!c->d_base) HIP_TRY(hipMalloc(&c->d_base, (size_t)c->max_frames * 2 * kNumBin));
    if (!c->d_msgtab) {
        MsgTables t;
        build_msg_tables(&t);
        MsgTables *d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof t));
        if (hipMemcpy(d, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return ft8_fail("uploading the SNR tables failed");
        }
        c->d_msgtab = d;
    }
    return 0;
}

extern "C" {

int ft8gpu_noise_baseline(ft8gpu_ctx *c, const uint8_t *mag, int nframes, uint8_t *base, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !base) return ft8_fail("NULL array argument");
    if (ensure_messages_buffers(c)) return -1;
    const size_t per = 2 * kNumBin;
    for (int f0 = 0; f0 < nframes; f0 += c->max_frames) {
        const int n = (nframes - f0 < c->max_frames) ? nframes - f0 : c->max_frames;
        if (flags & FT8GPU_DEVICE_PTRS) {
            HIP_TRY(launch_noise_baseline(mag + (size_t)f0 * kMagArray, base + (size_t)f0 * per, n, c->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(c->d_mag, mag + (size_t)f0 * kMagArray, (size_t)n * kMagArray, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(launch_noise_baseline(c->d_mag, c->d_base, n, c->stream));
            HIP_TRY(hipMemcpyAsync(base + (size_t)f0 * per, c->d_base, (size_t)n * per, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    return 0;
}

int ft8gpu_collect_messages(ft8gpu_ctx *c, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                            const ft8gpu_decode_status *status, int nframes, ft8gpu_message *msgs, int32_t *n_msgs, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!mag || !cands || !counts || !status || !msgs || !n_msgs) return ft8_fail("NULL array argument");
    if (ensure_messages_buffers(c)) return -1;
    const int mc = c->params.max_candidates;
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (!dev && !c->d_msgs) HIP_TRY(hipMalloc(&c->d_msgs, (size_t)c->max_frames * kMaxMessages * sizeof(ft8gpu_message)));
    for (int f0 = 0; f0 < nframes; f0 += c->max_frames) {
        const int n = (nframes - f0 < c->max_frames) ? nframes - f0 : c->max_frames;
        const uint8_t *dm = dev ? mag + (size_t)f0 * kMagArray : c->d_mag;
        const ft8gpu_candidate *dc = dev ? cands + (size_t)f0 * mc : c->d_cands;
        const int32_t *dn = dev ? counts + f0 : c->d_counts;
        const ft8gpu_decode_status *dst = dev ? status + (size_t)f0 * mc : c->d_status;
        ft8gpu_message *dmsg = dev ? msgs + (size_t)f0 * kMaxMessages : c->d_msgs;
        int32_t *dnm = dev ? n_msgs + f0 : c->d_nres;
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(c->d_mag, mag + (size_t)f0 * kMagArray, (size_t)n * kMagArray, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_cands, cands + (size_t)f0 * mc, (size_t)n * mc * sizeof(ft8gpu_candidate), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_counts, counts + f0, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(c->d_status, status + (size_t)f0 * mc, (size_t)n * mc * sizeof(ft8gpu_decode_status), hipMemcpyHostToDevice, c->stream));
            // slots past a frame's count keep the caller's bytes
            HIP_TRY(hipMemcpyAsync(c->d_msgs, msgs + (size_t)f0 * kMaxMessages, (size_t)n * kMaxMessages * sizeof(ft8gpu_message), hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(launch_noise_baseline(dm, c->d_base, n, c->stream));
        HIP_TRY(launch_messages(dm, c->d_base, dc, dn, dst, c->d_msgtab, n, mc, c->params.min_score, dmsg, dnm, c->stream));
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(msgs + (size_t)f0 * kMaxMessages, c->d_msgs, (size_t)n * kMaxMessages * sizeof(ft8gpu_message), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(n_msgs + f0, c->d_nres, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    return 0;
}

}  // extern "C"
