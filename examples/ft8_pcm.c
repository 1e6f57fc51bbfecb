/*
 * ft8_pcm.c -- decode one .wav at 48 .. 768 kHz with libft8gpu.so from plain C: a sound card's recording (one channel, real) or
 * an SDR program's baseband recording (two channels: I, Q), 16-bit PCM or 32-bit float.  ft8gpu_read_wav_pcm, then
 * ft8gpu_decode_pcm over the channels named on the command line, then the ft8gpu_format_messages table.  A frequency is the
 * channel's lower edge in Hz on the file's own axis (0 Hz is the centre of an I/Q recording); the channel is the 1600 Hz above
 * it.  With no frequency a one-channel file is decoded at 0 and 1500 Hz (0 .. 3100 Hz, as ft8gpu_decode_audio does by default)
 * and an I/Q file at -800 Hz (the 1600 Hz around its centre).
 *
 *   gcc -O2 -std=gnu17 -I include examples/ft8_pcm.c -L rtlsdr_ft8d_amd -lft8gpu -Wl,-rpath,$PWD/rtlsdr_ft8d_amd -o ft8_pcm
 *   ./ft8_pcm file.wav [freq_hz ...]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "ft8gpu.h"

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.wav [freq_hz ...]\n", argv[0]);
        return 2;
    }
    if (argc - 2 > FT8GPU_PCM_MAX_CHANNELS) {
        fprintf(stderr, "%s: at most %d frequencies\n", argv[0], FT8GPU_PCM_MAX_CHANNELS);
        return 2;
    }
    const size_t cap = (size_t)FT8GPU_PCM_MAX_SAMPLES * 2 * sizeof(float);
    void *pcm = malloc(cap);
    static ft8gpu_message msgs[FT8GPU_K_MAX_MESSAGES * FT8GPU_PCM_MAX_CHANNELS];
    if (!pcm) {
        fprintf(stderr, "%s: out of memory\n", argv[0]);
        return 1;
    }
    int format = 0, rate = 0;
    int32_t nsamples = 0;
    if (ft8gpu_read_wav_pcm(argv[1], pcm, cap, &format, &rate, &nsamples) != 0) {          /* the reader has said why */
        free(pcm);
        return 1;
    }
    if (nsamples < 1) {
        fprintf(stderr, "%s: no samples\n", argv[1]);
        free(pcm);
        return 1;
    }
    const int iq = (format & FT8GPU_PCM_COMPLEX) != 0;
    printf("%s: %d %s samples at %d Hz, %.2f s\n", argv[1], (int)nsamples, iq ? "I/Q" : "real", rate, (double)nsamples / rate);

    int32_t freq_bin[FT8GPU_PCM_MAX_CHANNELS];
    int nchannels = argc - 2;
    for (int i = 0; i < nchannels; i++) freq_bin[i] = (int32_t)lrint(atof(argv[2 + i]) / 6.25);
    if (nchannels == 0) {
        if (iq) {
            freq_bin[0] = -128;
            nchannels = 1;
        } else {
            freq_bin[0] = 0;
            freq_bin[1] = 240;
            nchannels = 2;
        }
    }
    int32_t n_msgs = 0;
    ft8gpu_ctx *ctx = NULL;
    if (ft8gpu_create(&ctx, 0, nchannels, NULL) != 0) {
        fprintf(stderr, "ft8gpu_create: %s\n", ft8gpu_last_error());
        free(pcm);
        return 1;
    }
    int rc = ft8gpu_decode_pcm(ctx, pcm, format, rate, 1, nsamples, freq_bin, nchannels, msgs, &n_msgs, FT8GPU_HOST_PTRS);
    if (rc != 0) fprintf(stderr, "ft8gpu_decode_pcm: %s\n", ft8gpu_last_error());
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
    free(pcm);
    return rc != 0;
}
