/* gfsk_asan_main.c -- the host code of the GFSK synthesiser under AddressSanitizer / UBSan, as a program of its own
 * (tests/test_gfsk_cpu.py builds and runs it; nothing is loaded into python): the table builders into exactly sized heap blocks,
 * their refusals, and ft8gpu_write_wav / ft8gpu_read_wav on the edge lengths 0, 1 and 180000.
 *   gcc -fsanitize=address,undefined -I include tests/host_asan/gfsk_asan_main.c rtlsdr_ft8d_amd/csrc/ft8_gfsk.c \
 *       rtlsdr_ft8d_amd/csrc/ft8_compat.c rtlsdr_ft8d_amd/csrc/ft8_pack.c -lpthread -lm
 *   ./a.out <a writable directory> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

/* the GPU half of the library, which ft8_compat.c calls, is replaced by failing definitions, as in audio_asan_main.c */
int ft8gpu_create(ft8gpu_ctx **out, int device, int max_frames, const ft8gpu_params *params) {
    (void)device; (void)max_frames; (void)params;
    *out = NULL;
    return -1;
}
void ft8gpu_destroy(ft8gpu_ctx *ctx) { (void)ctx; }
const char *ft8gpu_last_error(void) { return "host sanitizer harness: no GPU half linked"; }
int ft8gpu_decode_batch(ft8gpu_ctx *ctx, const float *iq, int nframes, struct decoder_results *decodes, int32_t *n_results, int flags) {
    (void)ctx; (void)iq; (void)nframes; (void)decodes; (void)n_results; (void)flags;
    return -1;
}
int ft8gpu_set_params(ft8gpu_ctx *ctx, const ft8gpu_params *params) { (void)ctx; (void)params; return -1; }
int ft8gpu_find_sync(ft8gpu_ctx *ctx, const uint8_t *mag, int nframes, ft8gpu_candidate *cands, int32_t *counts, int flags) {
    (void)ctx; (void)mag; (void)nframes; (void)cands; (void)counts; (void)flags;
    return -1;
}
int ft8gpu_decode_candidates(ft8gpu_ctx *ctx, const uint8_t *mag, const ft8gpu_candidate *cands, const int32_t *counts,
                             int nframes, ft8gpu_decode_status *status, int flags) {
    (void)ctx; (void)mag; (void)cands; (void)counts; (void)nframes; (void)status; (void)flags;
    return -1;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "gfsk_asan: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s dir\n", argv[0]);
        return 2;
    }
    static const int kSps[2] = { FT8GPU_GFSK_SPS_IQ, FT8GPU_GFSK_SPS_AUDIO };
    for (int v = 0; v < 2; v++) {
        const int sps = kSps[v];
        uint32_t *q = malloc((size_t)(3 * sps + 1) * sizeof *q);          /* exactly sized: one entry too many is caught */
        float *r = malloc((size_t)(sps / 8) * sizeof *r);
        CHECK(q && r);
        CHECK(ft8gpu_gfsk_pulse(sps, q) == 0 && ft8gpu_gfsk_ramp(sps, r) == 0);
        CHECK(q[0] == 0 && q[3 * sps] == 0 && q[3 * sps / 2] > 0x7F000000u && q[3 * sps / 2] < 0x80000000u);
        CHECK(r[0] == 0.0f && r[sps / 8 - 1] < 1.0f && r[sps / 16] == 0.5f);
        free(q);
        free(r);
    }
    uint32_t one = 7;
    float onef = 7.0f;
    CHECK(ft8gpu_gfsk_pulse(0, &one) == -1 && ft8gpu_gfsk_pulse(511, &one) == -1 && ft8gpu_gfsk_pulse(512, NULL) == -1 && one == 7);
    CHECK(ft8gpu_gfsk_ramp(8, &onef) == -1 && ft8gpu_gfsk_ramp(1920, NULL) == -1 && onef == 7.0f);
    float *gc = malloc(2 * FT8GPU_GFSK_TWIDDLES * sizeof *gc), *gf = malloc(2 * FT8GPU_GFSK_TWIDDLES * sizeof *gf);
    CHECK(gc && gf);
    ft8gpu_gfsk_twiddles(gc, gf);
    ft8gpu_gfsk_twiddles(NULL, gf);
    ft8gpu_gfsk_twiddles(gc, NULL);
    ft8gpu_gfsk_twiddles(NULL, NULL);
    CHECK(gc[0] == 1.0f && gc[1] == 0.0f && gc[2 * 1024 + 1] == 1.0f && gf[0] == 1.0f && gf[2 * 4095 + 1] > 0.0015f);
    free(gc);
    free(gf);

    char path[4096];
    static const int32_t kLengths[3] = { 0, 1, FT8GPU_AUDIO_NSAMPLES };
    for (int v = 0; v < 3; v++) {
        const int32_t n = kLengths[v];
        int16_t *pcm = malloc((size_t)(n ? n : 1) * sizeof *pcm), *back = malloc((size_t)(n ? n : 1) * sizeof *back);
        CHECK(pcm && back);
        for (int32_t i = 0; i < n; i++) pcm[i] = (int16_t)((i * 7919) % 65536 - 32768);
        if (n) pcm[n - 1] = 32767;
        snprintf(path, sizeof path, "%s/edge_%d.wav", argv[1], (int)n);
        CHECK(ft8gpu_write_wav(path, n ? pcm : NULL, n) == 0);
        int32_t got = -1;
        memset(back, 0x5A, (size_t)(n ? n : 1) * sizeof *back);
        CHECK(ft8gpu_read_wav(path, back, n, &got) == 0 && got == n);
        CHECK(n == 0 || memcmp(pcm, back, (size_t)n * sizeof *pcm) == 0);
        if (n > 1) {                                                       /* a cap below the file's length */
            CHECK(ft8gpu_read_wav(path, back, n - 1, &got) == 0 && got == n - 1);
        }
        free(pcm);
        free(back);
    }
    int16_t s = 1;
    snprintf(path, sizeof path, "%s/no-such-directory/x.wav", argv[1]);
    CHECK(ft8gpu_write_wav(path, &s, 1) == -1);
    CHECK(ft8gpu_write_wav(NULL, &s, 1) == -1 && ft8gpu_write_wav(path, NULL, 1) == -1 && ft8gpu_write_wav(path, &s, -1) == -1);
    puts("gfsk_asan ok");
    return 0;
}
