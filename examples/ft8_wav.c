/*
 * ft8_wav.c -- decode one 12 kHz mono 16-bit .wav (a WSJT-X save, an ft8_lib test clip, a web receiver's recording) with
 * libft8gpu.so from plain C: ft8gpu_read_wav, then ft8gpu_decode_audio over the bands that start at 0 Hz and at 1500 Hz
 * (base bins 0 and 240: together 0 .. 3100 Hz of the audio), then the ft8gpu_format_messages table.
 *
 *   gcc -O2 -std=gnu17 -I include examples/ft8_wav.c -L rtlsdr_ft8d_amd -lft8gpu -Wl,-rpath,$PWD/rtlsdr_ft8d_amd -o ft8_wav
 *   ./ft8_wav clip.wav [device]
 */
#include <stdio.h>
#include <stdlib.h>

#include "ft8gpu.h"

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s clip.wav [device]\n", argv[0]);
        return 2;
    }
    static int16_t pcm[FT8GPU_AUDIO_NSAMPLES];
    int32_t nsamples = 0;
    if (ft8gpu_read_wav(argv[1], pcm, FT8GPU_AUDIO_NSAMPLES, &nsamples) != 0) return 1;   /* the reader has said why */
    if (nsamples < 1) {
        fprintf(stderr, "%s: no samples\n", argv[1]);
        return 1;
    }
    printf("%s: %d samples, %.2f s\n", argv[1], (int)nsamples, (double)nsamples / FT8GPU_AUDIO_RATE);

    enum { kBands = 2 };
    static const int32_t base_bin[kBands] = { 0, 240 };
    static ft8gpu_message msgs[FT8GPU_K_MAX_MESSAGES * kBands];
    int32_t n_msgs = 0;
    ft8gpu_ctx *ctx = NULL;
    if (ft8gpu_create(&ctx, argc > 2 ? atoi(argv[2]) : 0, kBands, NULL) != 0) {
        fprintf(stderr, "ft8gpu_create: %s\n", ft8gpu_last_error());
        return 1;
    }
    int rc = ft8gpu_decode_audio(ctx, pcm, FT8GPU_AUDIO_S16, 1, nsamples, base_bin, kBands, msgs, &n_msgs, FT8GPU_HOST_PTRS);
    if (rc != 0) fprintf(stderr, "ft8gpu_decode_audio: %s\n", ft8gpu_last_error());
    else {
        /* the formatter prints up to 50 records a call */
        for (int32_t at = 0; at < n_msgs; at += FT8GPU_K_MAX_MESSAGES) {
            char text[FT8GPU_K_MAX_MESSAGES * 96];
            const int32_t n = n_msgs - at < FT8GPU_K_MAX_MESSAGES ? n_msgs - at : FT8GPU_K_MAX_MESSAGES;
            if (ft8gpu_format_messages(msgs + at, n, text, sizeof text) >= 0) fputs(text, stdout);
        }
        printf("%d messages\n", (int)n_msgs);
    }
    ft8gpu_destroy(ctx);
    return rc != 0;
}
