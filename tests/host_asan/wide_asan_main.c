/*
 * Host-only sanitizer harness for the tables of the wideband RX front end (csrc/ft8_wide.c): compiled with gcc
 * -fsanitize=address,undefined together with ft8_wide.c and run by tests/test_wide_cpu.py.  Every table is written into a heap
 * block of exactly its size, so a write past it is caught; a NULL table is refused without a write; the values are checked
 * against the properties the header states.
 *   gcc -fsanitize=address,undefined -I include tests/host_asan/wide_asan_main.c rtlsdr_ft8d_amd/csrc/ft8_wide.c -lm
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(void) {
    int16_t *w1 = malloc(sizeof(int16_t) * 2 * FT8GPU_WIDE_MIX1);
    float *w2 = malloc(sizeof(float) * 2 * FT8GPU_WIDE_MIX2);
    float *h = malloc(sizeof(float) * FT8GPU_WIDE_TAPS);
    CHECK(w1 && w2 && h);
    memset(h, 0xA5, sizeof(float) * FT8GPU_WIDE_TAPS);

    ft8gpu_wide_mixer1(NULL);                                /* refused: nothing to write to */
    ft8gpu_wide_mixer2(NULL);
    ft8gpu_wide_taps(NULL);
    ft8gpu_wide_mixer1(w1);
    ft8gpu_wide_mixer2(w2);
    ft8gpu_wide_taps(h);

    CHECK(w1[0] == 32767 && w1[1] == 0 && w1[2 * 1500] == 0 && w1[2 * 1500 + 1] == -32767 && w1[2 * 3000] == -32767);
    for (int i = 0; i < FT8GPU_WIDE_MIX1; i++) {
        const double a = 2.0 * M_PI * (double)i / FT8GPU_WIDE_MIX1;
        CHECK(fabs((double)w1[2 * i] - 32767.0 * cos(a)) <= 0.5 + 1e-9 && fabs((double)w1[2 * i + 1] + 32767.0 * sin(a)) <= 0.5 + 1e-9);
        /* the complex product of a byte pair with an entry stays below 2^23 */
        CHECK(128.0 * (fabs((double)w1[2 * i]) + fabs((double)w1[2 * i + 1])) < 8388608.0);
    }
    CHECK(w2[0] == 1.0f && w2[1] == -0.0f && fabsf(w2[2 * 768]) < 1e-7f && w2[2 * 768 + 1] == -1.0f);
    for (int i = 0; i < FT8GPU_WIDE_MIX2; i++) CHECK(fabs((double)w2[2 * i] * w2[2 * i] + (double)w2[2 * i + 1] * w2[2 * i + 1] - 1.0) < 1e-6);

    double sum = 0.0;
    for (int i = 0; i < 95; i++) {
        CHECK(h[i] == h[94 - i]);                            /* symmetric about 47 */
        sum += h[i];
    }
    CHECK(fabs(sum - 1.0) < 1e-6 && h[95] == 0.0f && h[47] > 0.1f && h[47] < 0.3f);

    /* a second call writes the same bytes */
    float *h2 = malloc(sizeof(float) * FT8GPU_WIDE_TAPS);
    CHECK(h2 != NULL);
    ft8gpu_wide_taps(h2);
    CHECK(memcmp(h, h2, sizeof(float) * FT8GPU_WIDE_TAPS) == 0);
    free(h2);
    free(h);
    free(w2);
    free(w1);
    puts("wide_asan ok");
    return 0;
}
