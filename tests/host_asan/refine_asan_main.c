/* Stand-alone driver of the host side of the refined time and frequency (csrc/ft8_refine.c) for AddressSanitizer and
 * UBSan: the estimate on edge records and on records that are no device output, the table into buffers of every short
 * length, each allocated at its exact size so that a byte too many is caught.  tests/test_refine_cpu.py builds and runs it. */
#include "ft8gpu.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static void fill(ft8gpu_message *m, ft8gpu_refined *r, int to, int ts, int fo, int fs, int e, float p0, float p1, float p2, float noise) {
    memset(m, 0, sizeof *m);
    memset(r, 0, sizeof *r);
    memset(m->text, 'X', sizeof m->text);                     /* no terminator: the table must stop at 25 characters */
    m->cand.time_offset = (int16_t)to; m->cand.time_sub = (uint8_t)ts;
    m->cand.freq_offset = (int16_t)fo; m->cand.freq_sub = (uint8_t)fs;
    m->snr_db = -12; m->dt_s = 1.25f; m->freq_hz = 1234.5f;
    r->e_best = (int16_t)e; r->valid = 1;
    r->pt[0] = p0; r->pt[1] = p1; r->pt[2] = p2;
    r->pf[0] = p0 / 4; r->pf[1] = p0; r->pf[2] = p1; r->pf[3] = p2; r->pf[4] = p2 / 4;
    r->noise = noise;
}

int main(void) {
    enum { N = 12 };
    /* exact-size heap arrays: reading record N is a heap overflow */
    ft8gpu_message *m = malloc(N * sizeof *m);
    ft8gpu_refined *r = malloc(N * sizeof *r);
    CHECK(m && r);
    fill(&m[0], &r[0], 5, 1, 160, 0, 3, 80.0f, 100.0f, 90.0f, 2.0f);
    fill(&m[1], &r[1], -12, 0, 0, 0, -16, 0.0f, 100.0f, 99.0f, 0.5f);
    fill(&m[2], &r[2], 23, 1, 248, 1, 16, 99.0f, 100.0f, 0.0f, 0.5f);
    fill(&m[3], &r[3], 0, 0, 0, 0, -16, 0.0f, 0.0f, 0.0f, 0.0f);
    fill(&m[4], &r[4], 32767, 255, -32768, 255, 32767, 3.0e38f, 3.4e38f, 3.0e38f, 1.0e-45f);
    fill(&m[5], &r[5], -32768, 0, 32767, 255, -32768, INFINITY, INFINITY, INFINITY, INFINITY);
    fill(&m[6], &r[6], 1, 1, 1, 1, 0, NAN, NAN, NAN, NAN);
    fill(&m[7], &r[7], 1, 1, 1, 1, 0, 5.0f, 4.0f, 5.0f, -1.0f);
    fill(&m[8], &r[8], 1, 1, 1, 1, 200, 7.0f, 7.0f, 7.0f, 7.0f);
    fill(&m[9], &r[9], 4, 0, 100, 0, 0, 50.0f, 100.0f, 50.0f, 150.0f);
    fill(&m[10], &r[10], 4, 0, 100, 0, 0, 1.0e-45f, 2.0e-45f, 1.0e-45f, 1.0e-45f);
    fill(&m[11], &r[11], 4, 0, 100, 0, 0, 50.0f, 100.0f, 50.0f, 2.0f);
    r[11].valid = 0;
    m[11].dt_s = -3.0e38f; m[11].freq_hz = 3.4e38f;           /* no decode: the longest line "%5.2f %6.1f" can print */
    for (int i = 0; i < N; i++) {
        float dt = 77.0f, hz = 77.0f, snr = 77.0f;
        const int rc = ft8gpu_refined_estimate(&m[i], &r[i], &dt, &hz, &snr);
        if (i == 11) { CHECK(rc == -1 && dt == 77.0f && hz == 77.0f && snr == 77.0f); continue; }
        CHECK(rc == 0 && snr >= -30.0f && snr <= 49.0f && !isnan(dt) && !isnan(hz));
    }
    float dt, hz, snr;
    CHECK(ft8gpu_refined_estimate(&m[0], &r[0], &dt, &hz, &snr) == 0);
    CHECK(fabsf(dt - (256.0f * 11 + 256 + 32 * (3 + 1.0f / 6)) / 3200.0f) < 1e-5f && fabsf(hz - 3.125f * (320 + 1.0f / 6)) < 1e-3f);
    CHECK(ft8gpu_refined_estimate(&m[1], &r[1], &dt, &hz, &snr) == 0 && fabsf(dt - (256.0f * -24 + 256 - 512) / 3200.0f) < 1e-6f);
    CHECK(ft8gpu_refined_estimate(&m[3], &r[3], &dt, &hz, &snr) == 0 && snr == -30.0f);
    CHECK(ft8gpu_refined_estimate(NULL, &r[0], &dt, &hz, &snr) == -1 && ft8gpu_refined_estimate(&m[0], NULL, &dt, &hz, &snr) == -1);
    CHECK(ft8gpu_refined_estimate(&m[0], &r[0], NULL, &hz, &snr) == -1 && ft8gpu_refined_estimate(&m[0], &r[0], &dt, NULL, &snr) == -1);
    CHECK(ft8gpu_refined_estimate(&m[0], &r[0], &dt, &hz, NULL) == -1);

    const int need = ft8gpu_format_messages_refined(m, r, N, NULL, 0);
    CHECK(need > 0);
    char *whole = malloc((size_t)need + 1);
    CHECK(whole && ft8gpu_format_messages_refined(m, r, N, whole, (size_t)need + 1) == need && (int)strlen(whole) == need);
    for (int cap = 1; cap <= need + 1; cap++) {                /* every truncation, each in a buffer of exactly cap bytes */
        char *out = malloc((size_t)cap);
        CHECK(out != NULL);
        memset(out, 'Z', (size_t)cap);
        CHECK(ft8gpu_format_messages_refined(m, r, N, out, (size_t)cap) == need);
        CHECK((int)strlen(out) == (cap - 1 < need ? cap - 1 : need) && !strncmp(out, whole, strlen(out)));
        free(out);
    }
    char one[1] = { 'Q' };
    CHECK(ft8gpu_format_messages_refined(m, r, N, one, 0) == need && one[0] == 'Q');       /* cap 0: nothing is written */
    CHECK(ft8gpu_format_messages_refined(NULL, r, 1, one, 1) == -1 && ft8gpu_format_messages_refined(m, NULL, 1, one, 1) == -1);
    CHECK(ft8gpu_format_messages_refined(NULL, NULL, 0, one, 1) == 0 && one[0] == 0);
    free(whole);
    free(m);
    free(r);
    printf("refine_asan ok\n");
    return 0;
}
