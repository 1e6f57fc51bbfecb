/*
 * ft8_wide.c -- decode one raw 2.4 Msps capture (unsigned 8-bit I/Q as rtl_sdr writes it, up to 15 s) with libft8gpu.so from
 * plain C: every dial frequency named on the command line, as an offset in Hz from the capture's centre, becomes a channel of
 * ft8gpu_decode_wide (offsets are rounded to the 6.25 Hz grid), then the ft8gpu_format_messages table.  The 7 MHz sub-bands from
 * a capture centred on 7.060 MHz:  ./ft8_wide cap.u8 -19000 -4000 11000 14000
 *
 *   gcc -O2 -std=gnu17 -I include examples/ft8_wide.c -L rtlsdr_ft8d_amd -lft8gpu -Wl,-rpath,$PWD/rtlsdr_ft8d_amd -lm -o ft8_wide
 *   ./ft8_wide capture.u8 offset_hz [offset_hz ...]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "ft8gpu.h"

int main(int argc, char **argv) {
    if (argc < 3 || argc - 2 > FT8GPU_WIDE_MAX_CHANNELS) {
        fprintf(stderr, "usage: %s capture.u8 offset_hz [offset_hz ...]   (1 .. %d dial offsets from the capture's centre)\n", argv[0],
                FT8GPU_WIDE_MAX_CHANNELS);
        return 2;
    }
    const int nchannels = argc - 2;
    int32_t freq_bin[FT8GPU_WIDE_MAX_CHANNELS];
    for (int b = 0; b < nchannels; b++) freq_bin[b] = (int32_t)lrint(atof(argv[2 + b]) / 6.25);

    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 1;
    }
    uint8_t *raw = malloc(2 * (size_t)FT8GPU_WIDE_MAX_PAIRS);
    if (!raw) {
        fprintf(stderr, "out of memory\n");
        fclose(f);
        return 1;
    }
    const size_t got = fread(raw, 1, 2 * (size_t)FT8GPU_WIDE_MAX_PAIRS, f);
    fclose(f);
    const size_t npairs = got / 16 * 8;                     /* whole 16-byte units */
    if (npairs == 0) {
        fprintf(stderr, "%s: fewer than 8 I/Q pairs\n", argv[1]);
        free(raw);
        return 1;
    }
    printf("%s: %zu pairs, %.2f s, %d channels\n", argv[1], npairs, (double)npairs / FT8GPU_WIDE_RATE, nchannels);

    ft8gpu_message *msgs = malloc(sizeof(ft8gpu_message) * FT8GPU_K_MAX_MESSAGES * (size_t)nchannels);
    int32_t n_msgs = 0;
    ft8gpu_ctx *ctx = NULL;
    if (!msgs || ft8gpu_create(&ctx, 0, nchannels, NULL) != 0) {
        fprintf(stderr, "ft8gpu_create: %s\n", msgs ? ft8gpu_last_error() : "out of memory");
        free(msgs);
        free(raw);
        return 1;
    }
    int rc = ft8gpu_decode_wide(ctx, raw, 1, npairs, freq_bin, nchannels, msgs, &n_msgs, FT8GPU_HOST_PTRS);
    if (rc != 0) fprintf(stderr, "ft8gpu_decode_wide: %s\n", ft8gpu_last_error());
    else {
        /* the formatter prints up to 50 records a call; freq_hz is relative to the capture's centre, pad[0] the channel */
        for (int32_t at = 0; at < n_msgs; at += FT8GPU_K_MAX_MESSAGES) {
            char text[FT8GPU_K_MAX_MESSAGES * 96];
            const int32_t n = n_msgs - at < FT8GPU_K_MAX_MESSAGES ? n_msgs - at : FT8GPU_K_MAX_MESSAGES;
            if (ft8gpu_format_messages(msgs + at, n, text, sizeof text) >= 0) fputs(text, stdout);
        }
        printf("%d messages\n", (int)n_msgs);
    }
    ft8gpu_destroy(ctx);
    free(msgs);
    free(raw);
    return rc != 0;
}
