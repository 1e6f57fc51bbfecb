/*
 * ft8_gen.c -- one FT8 message as a 12 kHz mono 16-bit .wav that any FT8 decoder (or a rig's audio input) takes, with
 * libft8gpu.so from plain C: ft8gpu_pack77, ft8gpu_encode, ft8gpu_synth_gfsk_audio_faded (GFSK as it is on the air, int16, the
 * largest sample at half of full scale; with --spread, --delay or --path2 over a fading HF channel), then ft8gpu_write_wav.
 *
 *   gcc -O2 -std=gnu17 -I include examples/ft8_gen.c -L rtlsdr_ft8d_amd -lft8gpu -Wl,-rpath,$PWD/rtlsdr_ft8d_amd -o ft8_gen
 *   ./ft8_gen "CQ K1ABC FN42" 1500 out.wav [t0] [--spread HZ] [--delay MS] [--path2 GAIN] [--seed N]
 * 1500: the frequency of tone 0 in Hz; t0: the signal's start within the 15 s clip in seconds (default 0.5).
 * --spread: two-sided Doppler spread of each path in Hz, 0 .. 20; --delay: delay of the second path in ms, 0 .. 10; --path2: its
 * amplitude relative to the first, 0 .. 4 (default 1 once --delay is given, else 0: one path); --seed: another draw of the fading.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

int main(int argc, char **argv) {
    const char *pos[4] = { NULL, NULL, NULL, NULL };
    int npos = 0, faded = 0, path2_set = 0;
    ft8gpu_channel ch = { 0.0f, 0.0f, 0.0f, FT8GPU_CHANNEL_NONE };
    unsigned long long seed = 0;
    for (int i = 1; i < argc; i++) {
        const int opt = !strcmp(argv[i], "--spread") ? 1 : !strcmp(argv[i], "--delay") ? 2 : !strcmp(argv[i], "--path2") ? 3 :
                        !strcmp(argv[i], "--seed") ? 4 : 0;
        if (opt && i + 1 >= argc) npos = 5;                                 /* an option without its value: the usage line */
        else if (opt == 1) { ch.spread_hz = (float)atof(argv[++i]); faded = 1; }
        else if (opt == 2) { ch.delay_ms = (float)atof(argv[++i]); faded = 1; }
        else if (opt == 3) { ch.path2_gain = (float)atof(argv[++i]); faded = path2_set = 1; }
        else if (opt == 4) seed = strtoull(argv[++i], NULL, 0);
        else if (npos < 4) pos[npos++] = argv[i];
        else npos = 5;
    }
    if (npos < 3 || npos > 4) {
        fprintf(stderr, "usage: %s \"MESSAGE\" f0_hz out.wav [t0_s] [--spread HZ] [--delay MS] [--path2 GAIN] [--seed N]\n", argv[0]);
        return 2;
    }
    if (faded) {
        ch.mode = FT8GPU_CHANNEL_FADED;
        if (!path2_set && ch.delay_ms > 0.0f) ch.path2_gain = 1.0f;
    }
    uint8_t payload[10];
    if (ft8gpu_pack77(pos[0], payload) != 0) {
        fprintf(stderr, "%s: fits no FT8 message type\n", pos[0]);
        return 1;
    }
    ft8gpu_synth_signal sig;
    memset(&sig, 0, sizeof sig);
    ft8gpu_encode(payload, sig.tones);
    sig.f0_hz = (float)atof(pos[1]);
    sig.t0_s = npos > 3 ? (float)atof(pos[3]) : 0.5f;
    sig.amplitude = 1.0f;

    static int16_t pcm[FT8GPU_AUDIO_NSAMPLES];
    ft8gpu_ctx *ctx = NULL;
    if (ft8gpu_create(&ctx, 0, 1, NULL) != 0) {
        fprintf(stderr, "ft8gpu_create: %s\n", ft8gpu_last_error());
        return 1;
    }
    int rc = ft8gpu_synth_gfsk_audio_faded(ctx, &sig, &ch, 1, 1, FT8GPU_AUDIO_NSAMPLES, 0.0f, seed, 0, 0.5f, FT8GPU_AUDIO_S16, pcm,
                                           FT8GPU_HOST_PTRS);
    if (rc != 0) fprintf(stderr, "ft8gpu_synth_gfsk_audio_faded: %s\n", ft8gpu_last_error());
    ft8gpu_destroy(ctx);
    if (rc == 0) rc = ft8gpu_write_wav(pos[2], pcm, FT8GPU_AUDIO_NSAMPLES);    /* the writer has said why if it fails */
    if (rc == 0) {
        printf("%s: \"%s\" at %g Hz from %g s, %d samples", pos[2], pos[0], (double)sig.f0_hz, (double)sig.t0_s, FT8GPU_AUDIO_NSAMPLES);
        if (faded) printf(", spread %g Hz, path 2 %g at %g ms", (double)ch.spread_hz, (double)ch.path2_gain, (double)ch.delay_ms);
        printf("\n");
    }
    return rc != 0;
}
