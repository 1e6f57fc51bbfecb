/*
 * Host-only sanitizer harness for the host file of the PCM front end (csrc/ft8_pcm.c): compiled with gcc
 * -fsanitize=address,undefined together with ft8_pcm.c and run by tests/test_pcm_cpu.py.  Every table is written into a heap
 * block of exactly its size, so a write past it is caught; a NULL table and an unknown D are refused without a write; the .wav
 * reader is walked over well-formed files of every accepted layout, over truncated and hostile ones, and with a capacity that
 * cuts the data, each read into a heap block of exactly cap_bytes.
 *   gcc -fsanitize=address,undefined -I include tests/host_asan/pcm_asan_main.c rtlsdr_ft8d_amd/csrc/ft8_pcm.c -lm
 *   ./a.out <directory for the files>
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static void put16(unsigned char *b, unsigned v) { b[0] = (unsigned char)v; b[1] = (unsigned char)(v >> 8); }
static void put32(unsigned char *b, unsigned v) { put16(b, v & 0xffffu); put16(b + 2, v >> 16); }

/* a .wav image: RIFF, fmt (16 bytes, or 40 if extensible), an optional odd-sized chunk, data declaring `declared` bytes */
static size_t wav_image(unsigned char *out, unsigned tag, unsigned channels, unsigned rate, unsigned bits, int extensible, int odd_chunk,
                        unsigned data_bytes, unsigned declared) {
    size_t at = 12;
    memcpy(out, "RIFF\0\0\0\0WAVE", 12);
    const unsigned fmt_len = extensible ? 40 : 16;
    memcpy(out + at, "fmt ", 4);
    put32(out + at + 4, fmt_len);
    unsigned char *f = out + at + 8;
    memset(f, 0, fmt_len);
    put16(f, extensible ? 0xFFFEu : tag);
    put16(f + 2, channels);
    put32(f + 4, rate);
    put32(f + 8, rate * channels * bits / 8);
    put16(f + 12, channels * bits / 8);
    put16(f + 14, bits);
    if (extensible) {
        put16(f + 16, 22);
        put16(f + 18, bits);
        put16(f + 24, tag);
    }
    at += 8 + fmt_len;
    if (odd_chunk) {
        memcpy(out + at, "LIST", 4);
        put32(out + at + 4, 5);
        memset(out + at + 8, 'x', 6);                        /* 5 bytes and the pad */
        at += 8 + 6;
    }
    memcpy(out + at, "data", 4);
    put32(out + at + 4, declared);
    at += 8;
    for (unsigned i = 0; i < data_bytes; i++) out[at + i] = (unsigned char)(i * 7u + 3u);
    at += data_bytes;
    put32(out + 4, (unsigned)at - 8);
    return at;
}

static int write_file(const char *path, const unsigned char *b, size_t n) {
    FILE *f = fopen(path, "wb");
    if (!f) return -1;
    const size_t w = fwrite(b, 1, n, f);
    return fclose(f) == 0 && w == n ? 0 : -1;
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    static const int kD[5] = { 15, 30, 60, 120, 240 };

    /* ---- the tables ---- */
    CHECK(ft8gpu_pcm_decimation(48000) == 15 && ft8gpu_pcm_decimation(768000) == 240 && ft8gpu_pcm_decimation(44100) == 0 &&
          ft8gpu_pcm_decimation(0) == 0 && ft8gpu_pcm_decimation(-48000) == 0 && ft8gpu_pcm_decimation(12000) == 0);
    ft8gpu_pcm_mixer1(15, NULL);
    ft8gpu_pcm_mixer2(NULL);
    ft8gpu_pcm_taps_b(NULL);
    CHECK(ft8gpu_pcm_taps_a(15, NULL) == -1);
    float one = 7.0f;
    ft8gpu_pcm_mixer1(16, &one);                             /* an unknown D writes nothing */
    CHECK(ft8gpu_pcm_taps_a(0, &one) == -1 && ft8gpu_pcm_taps_a(45, &one) == -1 && ft8gpu_pcm_taps_a(-15, &one) == -1 && one == 7.0f);
    for (int i = 0; i < 5; i++) {
        const int D = kD[i], M = D / 3, n1 = 16 * D, na = 8 * M + 1;
        float *w1 = malloc(sizeof(float) * 2 * (size_t)n1), *h = malloc(sizeof(float) * (size_t)na);
        CHECK(w1 && h);
        ft8gpu_pcm_mixer1(D, w1);
        CHECK(ft8gpu_pcm_taps_a(D, h) == na);
        CHECK(w1[0] == 1.0f && w1[1] == -0.0f && fabsf(w1[2 * (4 * D)]) < 1e-7f && w1[2 * (4 * D) + 1] == -1.0f);
        for (int k = 0; k < n1; k++) CHECK(fabs((double)w1[2 * k] * w1[2 * k] + (double)w1[2 * k + 1] * w1[2 * k + 1] - 1.0) < 1e-6);
        double sum = 0.0;
        for (int k = 0; k < na; k++) {
            CHECK(h[k] == h[na - 1 - k]);                    /* symmetric about 4 M */
            sum += h[k];
        }
        CHECK(fabs(sum - 1.0) < 1e-5 && h[4 * M] > 0.0f);
        free(h);
        free(w1);
    }
    float *w2 = malloc(sizeof(float) * 2 * FT8GPU_PCM_MIX2), *hb = malloc(sizeof(float) * FT8GPU_PCM_TAPS_B);
    CHECK(w2 && hb);
    memset(hb, 0xA5, sizeof(float) * FT8GPU_PCM_TAPS_B);
    ft8gpu_pcm_mixer2(w2);
    ft8gpu_pcm_taps_b(hb);
    CHECK(w2[0] == 1.0f && w2[2 * 384 + 1] == -1.0f && hb[47] == 0.0f && hb[23] > 0.3f && hb[23] < 0.34f);
    for (int k = 0; k < 47; k++) CHECK(hb[k] == hb[46 - k]);
    free(hb);
    free(w2);

    /* ---- the reader ---- */
    char path[1024];
    snprintf(path, sizeof path, "%s/pcm_asan.wav", argv[1]);
    unsigned char *img = malloc(4096);
    CHECK(img != NULL);
    int format, rate;
    int32_t ns;
    static const struct { unsigned tag, channels, bits; int ext, fmt; } kGood[] = {
        { 1, 1, 16, 0, FT8GPU_PCM_S16 }, { 1, 2, 16, 0, FT8GPU_PCM_S16 | FT8GPU_PCM_COMPLEX }, { 3, 1, 32, 0, FT8GPU_PCM_F32 },
        { 3, 2, 32, 0, FT8GPU_PCM_F32 | FT8GPU_PCM_COMPLEX }, { 1, 2, 16, 1, FT8GPU_PCM_S16 | FT8GPU_PCM_COMPLEX },
        { 3, 2, 32, 1, FT8GPU_PCM_F32 | FT8GPU_PCM_COMPLEX } };
    for (size_t g = 0; g < sizeof kGood / sizeof kGood[0]; g++)
        for (int odd = 0; odd < 2; odd++) {
            const unsigned frame = kGood[g].channels * kGood[g].bits / 8, data = 37 * frame + 3;    /* stray bytes behind the last sample */
            const size_t n = wav_image(img, kGood[g].tag, kGood[g].channels, 192000, kGood[g].bits, kGood[g].ext, odd, data, data);
            CHECK(write_file(path, img, n) == 0);
            for (int cut = 0; cut < 2; cut++) {
                const size_t cap = cut ? 10 * frame + 1 : 37 * frame;   /* exactly what is read, or less */
                unsigned char *out = malloc(cap);
                CHECK(out != NULL);
                CHECK(ft8gpu_read_wav_pcm(path, out, cap, &format, &rate, &ns) == 0);
                CHECK(format == kGood[g].fmt && rate == 192000 && ns == (cut ? 10 : 37));
                CHECK(memcmp(out, img + n - data, (size_t)ns * frame) == 0);
                free(out);
            }
        }
    unsigned char sink[64];
    /* refused, each with nothing written past its block */
    static const struct { unsigned tag, channels, rate, bits; } kBad[] = {
        { 1, 1, 48000, 8 }, { 1, 1, 48000, 24 }, { 1, 3, 48000, 16 }, { 1, 1, 44100, 16 }, { 1, 1, 12000, 16 }, { 3, 1, 48000, 16 },
        { 1, 2, 48000, 32 }, { 3, 2, 48000, 64 }, { 2, 1, 48000, 16 }, { 1, 0, 48000, 16 }, { 1, 1, 0, 16 }, { 1, 1, 0xFFFFFFFFu, 16 } };
    for (size_t b = 0; b < sizeof kBad / sizeof kBad[0]; b++) {
        const size_t n = wav_image(img, kBad[b].tag, kBad[b].channels, kBad[b].rate, kBad[b].bits, 0, 0, 32, 32);
        CHECK(write_file(path, img, n) == 0);
        CHECK(ft8gpu_read_wav_pcm(path, sink, sizeof sink, &format, &rate, &ns) == -1 && ns == 0 && format == -1 && rate == 0);
    }
    /* every truncation of a good file: refused or read, never past the file or the block */
    const size_t full = wav_image(img, 1, 2, 48000, 16, 1, 1, 40, 40);
    for (size_t n = 0; n < full; n++) {
        CHECK(write_file(path, img, n) == 0);
        const int rc = ft8gpu_read_wav_pcm(path, sink, sizeof sink, &format, &rate, &ns);
        CHECK(rc == -1 && ns == 0);
    }
    /* a data chunk that declares more than the file holds; a zero-length data chunk; a 0-byte capacity */
    size_t n = wav_image(img, 1, 1, 48000, 16, 0, 0, 40, 4000);
    CHECK(write_file(path, img, n) == 0 && ft8gpu_read_wav_pcm(path, sink, sizeof sink, &format, &rate, &ns) == -1);
    n = wav_image(img, 1, 1, 48000, 16, 0, 0, 0, 0);
    CHECK(write_file(path, img, n) == 0 && ft8gpu_read_wav_pcm(path, sink, sizeof sink, &format, &rate, &ns) == 0 && ns == 0 && rate == 48000);
    n = wav_image(img, 1, 1, 48000, 16, 0, 0, 40, 40);
    CHECK(write_file(path, img, n) == 0 && ft8gpu_read_wav_pcm(path, sink, 0, &format, &rate, &ns) == 0 && ns == 0);
    CHECK(ft8gpu_read_wav_pcm(path, sink, 1, &format, &rate, &ns) == 0 && ns == 0);
    /* NULL arguments and a missing file */
    CHECK(ft8gpu_read_wav_pcm(NULL, sink, 8, &format, &rate, &ns) == -1 && ft8gpu_read_wav_pcm(path, NULL, 8, &format, &rate, &ns) == -1);
    CHECK(ft8gpu_read_wav_pcm(path, sink, 8, NULL, &rate, &ns) == -1 && ft8gpu_read_wav_pcm(path, sink, 8, &format, NULL, &ns) == -1);
    CHECK(ft8gpu_read_wav_pcm(path, sink, 8, &format, &rate, NULL) == -1);
    remove(path);
    CHECK(ft8gpu_read_wav_pcm(path, sink, 8, &format, &rate, &ns) == -1);
    free(img);
    puts("pcm_asan ok");
    return 0;
}
