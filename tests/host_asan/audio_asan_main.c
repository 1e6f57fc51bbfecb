/*
 * Host-only sanitizer harness for the .wav reader of csrc/ft8_compat.c (ft8gpu_read_wav): compiled with gcc
 * -fsanitize=address,undefined together with ft8_compat.c and ft8_pack.c and run by tests/test_audio_cpu.py.  The reader gets a
 * valid file, the refused shapes, and a few hundred random byte flips of a valid header; it must never read or write out of
 * bounds.  The GPU half of the library is replaced by failing definitions, as in compat_asan_main.c.
 *   gcc -fsanitize=address,undefined -I include tests/host_asan/audio_asan_main.c rtlsdr_ft8d_amd/csrc/ft8_compat.c \
 *       rtlsdr_ft8d_amd/csrc/ft8_pack.c -lpthread -lm
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

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

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

enum { kSamples = 1000, kHead = 44 };

static void put32(unsigned char *b, uint32_t v) { b[0] = (unsigned char)v; b[1] = (unsigned char)(v >> 8); b[2] = (unsigned char)(v >> 16); b[3] = (unsigned char)(v >> 24); }
static void put16(unsigned char *b, uint32_t v) { b[0] = (unsigned char)v; b[1] = (unsigned char)(v >> 8); }

/* a canonical 44-byte header and kSamples samples s[i] = 7 i - 3000 */
static size_t valid_wav(unsigned char *b) {
    memcpy(b, "RIFF", 4); put32(b + 4, 36 + 2 * kSamples); memcpy(b + 8, "WAVEfmt ", 8); put32(b + 16, 16);
    put16(b + 20, 1); put16(b + 22, 1); put32(b + 24, 12000); put32(b + 28, 24000); put16(b + 32, 2); put16(b + 34, 16);
    memcpy(b + 36, "data", 4); put32(b + 40, 2 * kSamples);
    for (int i = 0; i < kSamples; i++) put16(b + kHead + 2 * i, (uint32_t)(uint16_t)(int16_t)(7 * i - 3000));
    return kHead + 2 * kSamples;
}

static int write_file(const char *path, const unsigned char *b, size_t n) {
    FILE *f = fopen(path, "wb");
    if (!f) return -1;
    const size_t w = n ? fwrite(b, 1, n, f) : 0;
    return fclose(f) == 0 && w == n ? 0 : -1;
}

int main(int argc, char **argv) {
    const char *dir = argc > 1 ? argv[1] : "/tmp";
    char path[512];
    snprintf(path, sizeof path, "%s/audio_asan.wav", dir);
    unsigned char file[kHead + 2 * kSamples + 64], mut[sizeof file];
    const size_t len = valid_wav(file);
    int32_t n = -1;
    /* the output buffer holds exactly `cap` samples: a write past it is caught */
    int16_t *out = malloc(sizeof(int16_t) * kSamples);
    CHECK(out != NULL);

    CHECK(write_file(path, file, len) == 0);
    CHECK(ft8gpu_read_wav(path, out, kSamples, &n) == 0 && n == kSamples);
    for (int i = 0; i < kSamples; i++) CHECK(out[i] == (int16_t)(7 * i - 3000));
    int16_t *small = malloc(sizeof(int16_t) * 10);
    CHECK(small != NULL);
    CHECK(ft8gpu_read_wav(path, small, 10, &n) == 0 && n == 10 && small[9] == (int16_t)(63 - 3000));
    CHECK(ft8gpu_read_wav(path, small, 0, &n) == 0 && n == 0);
    free(small);
    CHECK(ft8gpu_read_wav(path, out, -1, &n) == -1 && ft8gpu_read_wav(NULL, out, 1, &n) == -1 && ft8gpu_read_wav(path, NULL, 1, &n) == -1 &&
          ft8gpu_read_wav(path, out, 1, NULL) == -1);

    /* refused shapes: 8 bit, stereo, 11025 Hz, every truncation of the header, data larger than the file, no data chunk, empty */
    memcpy(mut, file, len); put16(mut + 34, 8);
    CHECK(write_file(path, mut, len) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == -1 && n == 0);
    memcpy(mut, file, len); put16(mut + 22, 2);
    CHECK(write_file(path, mut, len) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == -1 && n == 0);
    memcpy(mut, file, len); put32(mut + 24, 11025);
    CHECK(write_file(path, mut, len) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == -1 && n == 0);
    for (size_t cut = 0; cut < kHead; cut++) CHECK(write_file(path, file, cut) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == -1 && n == 0);
    for (size_t cut = kHead; cut < len; cut += 97) CHECK(write_file(path, file, cut) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == (cut == len ? 0 : -1));
    memcpy(mut, file, len); put32(mut + 40, 0xFFFFFFFFu);
    CHECK(write_file(path, mut, len) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == -1);
    memcpy(mut, file, len); memcpy(mut + 36, "LIST", 4);
    CHECK(write_file(path, mut, len) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == -1);
    /* an odd-sized LIST chunk with its pad byte in front of data: accepted, same samples */
    memcpy(mut, file, 36); memcpy(mut + 36, "LIST", 4); put32(mut + 40, 5); memset(mut + 44, 'x', 6); memcpy(mut + 50, file + 36, len - 36);
    CHECK(write_file(path, mut, len + 14) == 0 && ft8gpu_read_wav(path, out, kSamples, &n) == 0 && n == kSamples && out[1] == (int16_t)(7 - 3000));

    /* random byte flips of the header (and of the odd-chunk variant's): any verdict, no bad access, n within cap */
    uint64_t s = 0x9E3779B97F4A7C15ull;
    int accepted = 0;
    for (int it = 0; it < 600; it++) {
        const int variant = it & 1;
        size_t mlen = len, hlen = kHead;
        if (variant) {
            memcpy(mut, file, 36); memcpy(mut + 36, "LIST", 4); put32(mut + 40, 5); memset(mut + 44, 'x', 6); memcpy(mut + 50, file + 36, len - 36);
            mlen = len + 14; hlen = kHead + 14;
        } else memcpy(mut, file, len);
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const int flips = 1 + (int)(s % 3);
        uint64_t r = s;
        for (int k = 0; k < flips; k++) {
            r = r * 6364136223846793005ull + 1442695040888963407ull;
            mut[(r >> 33) % hlen] ^= (unsigned char)(1u << ((r >> 20) & 7));
        }
        if (it % 5 == 0) { r = r * 6364136223846793005ull + 1442695040888963407ull; mut[(r >> 33) % hlen] = (unsigned char)(r >> 12); }
        CHECK(write_file(path, mut, mlen) == 0);
        const int32_t cap = (it % 3 == 0) ? 17 : kSamples;
        int16_t *o = malloc(sizeof(int16_t) * (size_t)cap);
        CHECK(o != NULL);
        const int rc = ft8gpu_read_wav(path, o, cap, &n);
        CHECK((rc == 0 && n >= 0 && n <= cap) || (rc == -1 && n == 0));
        accepted += rc == 0;
        free(o);
    }
    CHECK(accepted > 0);                                     /* flips of bytes nobody reads (sizes, rates of the fmt tail) still pass */
    remove(path);
    free(out);
    puts("audio_asan ok");
    return 0;
}
