// api_rx_stream.hip -- host glue of ft8gpu_rx_stream: the RX front end with the filter state carried from one buffer
// into the next (rx_stream.hip).  The host form stages the whole call at once: raw bytes, states, frames and counts go
// through the context's scratch blocks, so the result does not depend on how a caller cuts a stream into calls.
#include "ft8gpu_ctx.h"

#include <string.h>
#include <vector>

extern "C" {

void ft8gpu_rx_state_reset(ft8gpu_rx_state *st) {
    if (st) memset(st, 0, sizeof *st);
}

int ft8gpu_rx_stream(ft8gpu_ctx *c, const uint8_t *raw, int nstreams, int nslots, size_t npairs,
                     ft8gpu_rx_state *state, float *iq, uint32_t *n_out, int normalise, int flags) {
    if (!c) return ft8_fail("ctx is NULL");
    if (nstreams < 0 || nslots < 0) return ft8_fail("nstreams %d / nslots %d: negative", nstreams, nslots);
    Entry entry_(c);
    HIP_TRY(entry_.err);
    if (nstreams == 0 || nslots == 0) return 0;
    if ((long long)nstreams * nslots > c->max_frames)
        return ft8_fail("nstreams * nslots = %lld exceeds the context's max_frames %d", (long long)nstreams * nslots, c->max_frames);
    if (!raw || !state || !iq) return ft8_fail("NULL array argument");
    if (npairs == 0 || npairs % 8 != 0) return ft8_fail("npairs must be a positive multiple of 8 (whole 16-byte units; the reference's buffers are multiples of 8 bytes)");
    if (npairs > (size_t)1 << 40) return ft8_fail("npairs %zu is too large", npairs);
    const bool dev = flags & FT8GPU_DEVICE_PTRS;
    if (dev && ((uintptr_t)raw & 15) != 0) return ft8_fail("raw must be 16-byte aligned");
    if (dev && ((uintptr_t)state & 3) != 0) return ft8_fail("state must be 4-byte aligned");
    // the entry decimationIndex of every stream: the device form reads them back before anything is enqueued
    std::vector<uint32_t> d0((size_t)nstreams);
    if (dev) {
        HIP_TRY(hipMemcpy2DAsync(d0.data(), sizeof(uint32_t), &state->decimationIndex, sizeof(ft8gpu_rx_state), sizeof(uint32_t),
                                 (size_t)nstreams, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        for (int k = 0; k < nstreams; ++k) d0[k] = state[k].decimationIndex;
    }
    for (int k = 0; k < nstreams; ++k)
        if (d0[k] > 750) return ft8_fail("state[%d].decimationIndex = %u: above 750 (not a state rtlsdr_callback can leave)", k, d0[k]);
    const size_t nframes = (size_t)nstreams * nslots;
    const size_t raw_bytes = nframes * npairs * 2, iq_bytes = nframes * 2 * kNSamples * sizeof(float);
    const size_t state_bytes = (size_t)nstreams * sizeof(ft8gpu_rx_state), nout_bytes = nframes * sizeof(uint32_t);
    size_t sums_bytes = 0, p2_bytes = 0;
    rx_stream_scratch(nstreams, nslots, npairs, &sums_bytes, &p2_bytes);
    const size_t stage_at = (p2_bytes + 15) & ~(size_t)15;   // host form: states and counts are staged behind the scratch
    if (!dev) p2_bytes = stage_at + ((state_bytes + 15) & ~(size_t)15) + nout_bytes;
    // scratch: 0 block sums, 1 entry states (and the staging behind them), 2 the host form's frames, 3 its raw bytes
    if (ensure_scratch(c, sums_bytes, p2_bytes, dev ? 0 : iq_bytes, dev ? 0 : raw_bytes)) return -1;
    void *const *sc = c->d_scratch;
    if (dev) {
        HIP_TRY(launch_rx_stream(raw, nstreams, nslots, npairs, state, sc[0], sc[1], iq, n_out, normalise, c->stream));
        return 0;
    }
    ft8gpu_rx_state *d_state = (ft8gpu_rx_state *)((char *)sc[1] + stage_at);
    uint32_t *d_nout = (uint32_t *)((char *)d_state + ((state_bytes + 15) & ~(size_t)15));
    HIP_TRY(hipMemcpyAsync(sc[3], raw, raw_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_state, state, state_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_rx_stream((const uint8_t *)sc[3], nstreams, nslots, npairs, d_state, sc[0], sc[1], (float *)sc[2], d_nout, normalise, c->stream));
    HIP_TRY(hipMemcpyAsync(iq, sc[2], iq_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(state, d_state, state_bytes, hipMemcpyDeviceToHost, c->stream));
    if (n_out) HIP_TRY(hipMemcpyAsync(n_out, d_nout, nout_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
