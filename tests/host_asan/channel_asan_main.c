/* channel_asan_main.c -- the host code of the fading channel under AddressSanitizer / UBSan, as a program of its own
 * (tests/test_channel_cpu.py builds and runs it; nothing is loaded into python): ft8gpu_channel_taps into exactly sized heap
 * blocks, ft8gpu_channel_check on every refusal, and ft8gpu_channel_clip into exactly sized outputs with signals that begin
 * before the clip and paths that run past its end, in both modes, at the shortest and an odd clip length.
 *   gcc -fsanitize=address,undefined -I include tests/host_asan/channel_asan_main.c rtlsdr_ft8d_amd/csrc/ft8_gfsk.c -lm
 *   ./a.out */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "channel_asan: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(void) {
    uint32_t *gstep = malloc(FT8GPU_CHANNEL_TAPS * sizeof *gstep), *theta = malloc(FT8GPU_CHANNEL_TAPS * sizeof *theta);
    CHECK(gstep && theta);
    CHECK(ft8gpu_channel_taps(~0ull, ~0ull, 63, 1, 20.0f, gstep, theta) == 0);
    CHECK(gstep[0] > 0x80000000u && gstep[15] < 0x80000000u && gstep[0] + gstep[15] == 0);
    CHECK(ft8gpu_channel_taps(1, 2, 3, 0, 0.0f, gstep, NULL) == 0 && gstep[0] == 0 && gstep[15] == 0);
    CHECK(ft8gpu_channel_taps(1, 2, 3, 0, 1.0f, NULL, theta) == 0 && ft8gpu_channel_taps(1, 2, 3, 0, 1.0f, NULL, NULL) == 0);
    CHECK(ft8gpu_channel_taps(1, 2, 3, 2, 1.0f, gstep, theta) == -1 && ft8gpu_channel_taps(1, 2, 3, 0, 20.5f, gstep, theta) == -1);
    CHECK(ft8gpu_channel_taps(1, 2, 3, 0, NAN, gstep, theta) == -1 && ft8gpu_channel_taps(1, 2, 3, 0, -1.0f, gstep, theta) == -1);
    free(gstep);
    free(theta);

    const ft8gpu_channel presets[4] = { FT8GPU_CHANNEL_QUIET, FT8GPU_CHANNEL_MODERATE, FT8GPU_CHANNEL_DISTURBED, FT8GPU_CHANNEL_FLUTTER };
    for (int k = 0; k < 4; k++) CHECK(ft8gpu_channel_check(&presets[k]) == 0);
    ft8gpu_channel c = FT8GPU_CHANNEL_MODERATE;
    c.spread_hz = NAN;            CHECK(ft8gpu_channel_check(&c) == 1);
    c.spread_hz = 20.0f;          CHECK(ft8gpu_channel_check(&c) == 0);
    c.delay_ms = 10.5f;           CHECK(ft8gpu_channel_check(&c) == 2);
    c.delay_ms = 10.0f;           CHECK(ft8gpu_channel_check(&c) == 0);
    c.path2_gain = -0.5f;         CHECK(ft8gpu_channel_check(&c) == 3);
    c.path2_gain = INFINITY;      CHECK(ft8gpu_channel_check(&c) == 3);
    c.mode = 2;                   CHECK(ft8gpu_channel_check(&c) == 4);
    c.mode = FT8GPU_CHANNEL_NONE; CHECK(ft8gpu_channel_check(&c) == 0);   /* mode 0: the other fields are not looked at */
    CHECK(ft8gpu_channel_check(NULL) == 4);

    /* three signals: from before the clip, to behind its end with the longest delay, and unfaded */
    ft8gpu_synth_signal sig[3];
    memset(sig, 0, sizeof sig);
    for (int s = 0; s < 3; s++) {
        for (int j = 0; j < FT8GPU_NN; j++) sig[s].tones[j] = (uint8_t)((j * 5 + s) & 7);
        sig[s].amplitude = 1.0f;
    }
    sig[0].f0_hz = 700.0f;  sig[0].t0_s = -0.5f;
    sig[1].f0_hz = 1500.5f; sig[1].t0_s = 2.36f;
    sig[2].f0_hz = 0.0f;    sig[2].t0_s = 14.99f;
    ft8gpu_channel ch[3] = { FT8GPU_CHANNEL_FLUTTER, { 0.0f, 10.0f, 4.0f, FT8GPU_CHANNEL_FADED }, { NAN, NAN, NAN, FT8GPU_CHANNEL_NONE } };
    float *iq = malloc(2 * 48000 * sizeof *iq);                            /* exactly sized: one sample too many is caught */
    CHECK(iq);
    CHECK(ft8gpu_channel_clip(FT8GPU_GFSK_IQ, sig, ch, 3, 0, 7, 1ull << 40, iq) == 0);
    CHECK(iq[0] != 0.0f && iq[47999] != 0.0f && iq[48000] != 0.0f && isfinite(iq[95999]));
    CHECK(ft8gpu_channel_clip(FT8GPU_GFSK_IQ, sig, NULL, 3, 0, 7, 0, iq) == 0);
    CHECK(ft8gpu_channel_clip(FT8GPU_GFSK_IQ, NULL, NULL, 0, 0, 7, 0, iq) == 0 && iq[0] == 0.0f && iq[95999] == 0.0f);
    free(iq);
    static const int kLengths[4] = { 1, 7, 20011, FT8GPU_AUDIO_NSAMPLES };
    for (int v = 0; v < 4; v++) {
        float *pcm = malloc((size_t)kLengths[v] * sizeof *pcm);
        CHECK(pcm);
        CHECK(ft8gpu_channel_clip(FT8GPU_GFSK_AUDIO, sig, ch, 3, kLengths[v], 7, 3, pcm) == 0);
        CHECK(isfinite(pcm[0]) && isfinite(pcm[kLengths[v] - 1]));
        if (v >= 2) CHECK(pcm[6000] != 0.0f);
        free(pcm);
    }
    float one = 7.0f;
    ch[1].delay_ms = 10.5f;
    CHECK(ft8gpu_channel_clip(FT8GPU_GFSK_AUDIO, sig, ch, 3, 1, 7, 3, &one) == -1 && one == 7.0f);
    ch[1].delay_ms = 10.0f;
    CHECK(ft8gpu_channel_clip(FT8GPU_GFSK_AUDIO, sig, ch, 3, 0, 7, 3, &one) == -1 && ft8gpu_channel_clip(FT8GPU_GFSK_AUDIO, sig, ch, 65, 1, 7, 3, &one) == -1);
    CHECK(ft8gpu_channel_clip(2, sig, ch, 3, 1, 7, 3, &one) == -1 && ft8gpu_channel_clip(FT8GPU_GFSK_AUDIO, sig, ch, 3, 1, 7, 3, NULL) == -1);
    sig[0].tones[78] = 8;
    CHECK(ft8gpu_channel_clip(FT8GPU_GFSK_AUDIO, sig, ch, 3, 1, 7, 3, &one) == -1 && one == 7.0f);
    puts("channel_asan ok");
    return 0;
}
