// api_glue.hip -- the buffer helpers the host files share (declared in ft8gpu_ctx.h), and the host glue of the stages either
// side of the decode path: RX front end (f-1), PSKreporter datagrams (f-4), synthetic frames (f-3).
#include "ft8gpu_ctx.h"

#include <string.h>

int ensure_scratch(ft8gpu_ctx *c, size_t b0, size_t b1, size_t b2, size_t b3) {
    const size_t need[4] = { b0, b1, b2, b3 };
    bool grows = false;
    for (int i = 0; i < 4; ++i) grows |= need[i] > c->scratch_cap[i];
    if (grows) HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 4; ++i)
        if (c->mem.grow(&c->d_scratch[i], &c->scratch_cap[i], need[i], "scratch")) return -1;
    return 0;
}

int ensure_msgs_staging(ft8gpu_ctx *c) {
    return c->mem.once(&c->d_msgs, (size_t)c->max_frames * kMaxMessages * sizeof(ft8gpu_message), "staging of the records");
}

int ensure_host_staging(ft8gpu_ctx *c, bool msgs) {
    if (c->mem.once(&c->d_iq, (size_t)c->max_frames * 2 * kNSamples * sizeof(float), "staging of the frames")) return -1;
    return msgs ? ensure_msgs_staging(c) : 0;
}

int ensure_counts_staging(ft8gpu_ctx *c) {
    return c->mem.once(&c->d_nbs, (size_t)c->max_frames * FT8GPU_MAX_PASSES * 3 * sizeof(int32_t), "staging of the counts by stage");
}

extern "C" {

int ft8gpu_rx_decimate(ft8gpu_ctx *c, const uint8_t *raw, int ncaptures, size_t npairs, float *iq,
                       int normalise, int flags) {
    CHECK_COMMON(c, ncaptures);
    if (ncaptures == 0) return 0;
    if (!raw || !iq) return ft8_fail("NULL array argument");
    if (npairs % 8 != 0) return ft8_fail("npairs must be a multiple of 8 (whole 16-byte units; the reference's buffers are multiples of 8 bytes)");
    const size_t nblocks = npairs / 751 > (size_t)kNSamples ? (size_t)kNSamples : npairs / 751;
    const size_t raw_bytes = (size_t)ncaptures * npairs * 2, iq_bytes = (size_t)ncaptures * 2 * kNSamples * sizeof(float);
    const size_t sums_bytes = (size_t)ncaptures * (nblocks + 1) * 16;
    const size_t p2_bytes = (size_t)ncaptures * ((nblocks + 15) / 16 + 1) * 32 + (size_t)ncaptures * 376 * 4;   // entry states + group totals + partial peaks
    const bool staged = !(flags & FT8GPU_DEVICE_PTRS);
    // scratch: 0 block sums, 1 entry states, 2 the host form's frames, 3 its raw bytes
    if (ensure_scratch(c, sums_bytes, p2_bytes, staged ? iq_bytes : 0, staged ? raw_bytes : 0)) return -1;
    void *const *sc = c->d_scratch;
    if (flags & FT8GPU_DEVICE_PTRS) {
        if (((uintptr_t)raw & 15) != 0) return ft8_fail("raw must be 16-byte aligned");
        HIP_TRY(launch_rx(raw, ncaptures, npairs, sc[0], sc[1], iq, normalise, c->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(sc[3], raw, raw_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_rx((const uint8_t *)sc[3], ncaptures, npairs, sc[0], sc[1], (float *)sc[2], normalise, c->stream));
        HIP_TRY(hipMemcpyAsync(iq, sc[2], iq_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

}  // extern "C"

// ---- f-4: PSKreporter datagrams ------------------------------------------------------------------
// The frame-independent front of the datagram (rtlsdr_ft8d.c:386-482): IPFIX message header, the
// receiver (options) template, the sender template and the receiver record.  The templates are
// generated from their field lists; the lengths that depend on the spot list are patched per frame
// by the kernel.
static int build_report_prefix(const ft8gpu_report_info *info, ReportPrefix *out) {
    struct Field { uint16_t id, len; bool enterprise; };
    static const Field rx_fields[] = { { 0x8002, 0xFFFF, true }, { 0x8004, 0xFFFF, true }, { 0x8008, 0xFFFF, true } };
    static const Field tx_fields[] = { { 0x8001, 0xFFFF, true }, { 0x8005, 4, true }, { 0x8006, 1, true }, { 0x800A, 0xFFFF, true },
                                       { 0x8003, 0xFFFF, true }, { 0x800B, 1, true }, { 0x0096, 4, false } };
    const uint32_t enterprise = 30351;                       // 0x0000768F
    unsigned char *b = out->bytes;
    size_t n = 0;
    auto be16 = [&](uint32_t v) { b[n++] = (unsigned char)(v >> 8); b[n++] = (unsigned char)v; };
    auto be32 = [&](uint32_t v) { be16(v >> 16); be16(v & 0xFFFF); };
    auto fields = [&](const Field *f, int count) {
        for (int i = 0; i < count; ++i) { be16(f[i].id); be16(f[i].len); if (f[i].enterprise) be32(enterprise); }
    };
    auto text = [&](const char *s, size_t cap) -> int {      // one length byte + characters
        const size_t len = strnlen(s, cap);
        if (len == cap) return ft8_fail("ft8gpu_report_info string is not NUL-terminated");
        b[n++] = (unsigned char)len;
        memcpy(b + n, s, len);
        n += len;
        return 0;
    };
    memset(out->bytes, 0, sizeof out->bytes);
    be16(0x000A); be16(0);                                   // version, total length (per frame)
    be32(info->unixtime); be32(info->sequence); be32(info->random_id);
    be16(3); be16(36); be16(0x9992); be16(3); be16(0);       // options template set: id, length, link, fields, scope fields
    fields(rx_fields, 3);
    be16(0);                                                 // padding
    be16(2); be16(60); be16(0x9993); be16(7);                // template set
    fields(tx_fields, 7);
    const size_t rx0 = n;                                    // receiver record
    be16(0x9992); be16(0);
    if (text(info->rcall, sizeof info->rcall) || text(info->rloc, sizeof info->rloc) ||
        text(info->app_version, sizeof info->app_version)) return -1;
    n += (4 - ((n - rx0) & 3)) & 3;                          // zero padding to 4 bytes
    b[rx0 + 2] = (unsigned char)((n - rx0) >> 8);
    b[rx0 + 3] = (unsigned char)(n - rx0);
    out->len = (int32_t)n;
    out->dial_freq = info->dial_freq;
    out->unixtime = info->unixtime;
    return 0;
}

extern "C" {

int ft8gpu_pskreporter_datagrams(ft8gpu_ctx *c, const struct decoder_results *decodes, const int32_t *n_results,
                                 int nframes, const ft8gpu_report_info *info, const uint32_t *unixtimes,
                                 uint8_t *datagrams, int32_t *lengths, int flags) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (!decodes || !n_results || !info || !datagrams || !lengths) return ft8_fail("NULL array argument");
    ReportPrefix pre;
    if (build_report_prefix(info, &pre)) return -1;
    if (flags & FT8GPU_DEVICE_PTRS) {
        if (((uintptr_t)datagrams & 15) != 0) return ft8_fail("datagrams must be 16-byte aligned");
        HIP_TRY(launch_report(decodes, n_results, nframes, pre, unixtimes, datagrams, lengths, c->stream));
        return 0;
    }
    const size_t F = (size_t)c->max_frames;
    HIP_TRY(hipStreamSynchronize(c->stream));              // staging may be regrown below
    if (c->mem.grow(&c->d_rep, &c->rep_cap, F * FT8GPU_DATAGRAM_STRIDE, "staging of the datagrams")) return -1;
    if (c->mem.grow(&c->d_rep_len, &c->rep_len_cap, F * sizeof(int32_t), "staging of the datagram lengths")) return -1;
    if (unixtimes && c->mem.grow(&c->d_rep_time, &c->rep_time_cap, F * sizeof(uint32_t), "staging of the unixtimes")) return -1;
    const StageArg a[] = { { decodes, c->d_decodes, kMaxMessages * sizeof(struct decoder_results), kIn },
                           { n_results, c->d_nres, sizeof(int32_t), kIn }, { unixtimes, c->d_rep_time, sizeof(uint32_t), kIn },
                           { datagrams, c->d_rep, FT8GPU_DATAGRAM_STRIDE, kOut }, { lengths, c->d_rep_len, sizeof(int32_t), kOut } };
    return for_each_chunk(c, nframes, flags, a, [&](int n, void *const *p) {
        HIP_TRY(launch_report((const struct decoder_results *)p[0], (const int32_t *)p[1], n, pre, (const uint32_t *)p[2],
                              (uint8_t *)p[3], (int32_t *)p[4], c->stream));
        return 0;
    });
}

int ft8gpu_synth_frames(ft8gpu_ctx *c, const ft8gpu_synth_signal *signals, int nframes, int nsig,
                        float noise_sigma, uint64_t seed, float *iq_dev) {
    return ft8gpu_synth_frames_at(c, signals, nframes, nsig, noise_sigma, seed, 0, iq_dev);
}

int ft8gpu_synth_frames_at(ft8gpu_ctx *c, const ft8gpu_synth_signal *signals, int nframes, int nsig,
                           float noise_sigma, uint64_t seed, uint64_t first_frame, float *iq_dev) {
    CHECK_COMMON(c, nframes);
    if (nframes == 0) return 0;
    if (nsig < 0 || nsig > 64) return ft8_fail("nsig_per_frame %d out of range [0, 64]", nsig);
    if (!iq_dev || (nsig > 0 && !signals)) return ft8_fail("NULL array argument");
    const size_t bytes = (size_t)nframes * (nsig > 0 ? nsig : 1) * sizeof(ft8gpu_synth_signal);
    if (c->mem.grow(&c->d_sigs, &c->sigs_cap, bytes, "the synthesiser's signals")) return -1;
    if (nsig > 0) HIP_TRY(hipMemcpyAsync(c->d_sigs, signals, (size_t)nframes * nsig * sizeof(ft8gpu_synth_signal), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_synth(c->d_sigs, nframes, nsig, noise_sigma, seed, first_frame, iq_dev, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
