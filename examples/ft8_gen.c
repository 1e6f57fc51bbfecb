/*
 * ft8_gen.c -- one FT8 message as a 12 kHz mono 16-bit .wav that any FT8 decoder (or a rig's audio input) takes, with
 * libft8gpu.so from plain C: ft8gpu_pack77, ft8gpu_encode, ft8gpu_synth_gfsk_audio (GFSK as it is on the air, int16, the largest
 * sample at half of full scale), then ft8gpu_write_wav.
 *
 *   gcc -O2 -std=gnu17 -I include examples/ft8_gen.c -L rtlsdr_ft8d_amd -lft8gpu -Wl,-rpath,$PWD/rtlsdr_ft8d_amd -o ft8_gen
 *   ./ft8_gen "CQ K1ABC FN42" 1500 out.wav [t0]
 * 1500: the frequency of tone 0 in Hz; t0: the signal's start within the 15 s clip in seconds (default 0.5).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ft8gpu.h"

int main(int argc, char **argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s \"MESSAGE\" f0_hz out.wav [t0_s]\n", argv[0]);
        return 2;
    }
    uint8_t payload[10];
    if (ft8gpu_pack77(argv[1], payload) != 0) {
        fprintf(stderr, "%s: fits no FT8 message type\n", argv[1]);
        return 1;
    }
    ft8gpu_synth_signal sig;
    memset(&sig, 0, sizeof sig);
    ft8gpu_encode(payload, sig.tones);
    sig.f0_hz = (float)atof(argv[2]);
    sig.t0_s = argc > 4 ? (float)atof(argv[4]) : 0.5f;
    sig.amplitude = 1.0f;

    static int16_t pcm[FT8GPU_AUDIO_NSAMPLES];
    ft8gpu_ctx *ctx = NULL;
    if (ft8gpu_create(&ctx, 0, 1, NULL) != 0) {
        fprintf(stderr, "ft8gpu_create: %s\n", ft8gpu_last_error());
        return 1;
    }
    int rc = ft8gpu_synth_gfsk_audio(ctx, &sig, 1, 1, FT8GPU_AUDIO_NSAMPLES, 0.0f, 0, 0, 0.5f, FT8GPU_AUDIO_S16, pcm, FT8GPU_HOST_PTRS);
    if (rc != 0) fprintf(stderr, "ft8gpu_synth_gfsk_audio: %s\n", ft8gpu_last_error());
    ft8gpu_destroy(ctx);
    if (rc == 0) rc = ft8gpu_write_wav(argv[3], pcm, FT8GPU_AUDIO_NSAMPLES);   /* the writer has said why if it fails */
    if (rc == 0) printf("%s: \"%s\" at %g Hz from %g s, %d samples\n", argv[3], argv[1], (double)sig.f0_hz, (double)sig.t0_s, FT8GPU_AUDIO_NSAMPLES);
    return rc != 0;
}
