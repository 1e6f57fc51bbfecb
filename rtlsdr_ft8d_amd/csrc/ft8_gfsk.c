/* ft8_gfsk.c -- host tables of the GFSK synthesiser (include/ft8gpu.h "GFSK synthesis") and the .wav writer.
 * Plain C, no GPU. */
#include "../../include/ft8gpu.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

static int gfsk_sps_ok(int sps) { return sps == FT8GPU_GFSK_SPS_IQ || sps == FT8GPU_GFSK_SPS_AUDIO; }

/* Q[k], k = 0 .. 3 sps: the running sum of the sampled pulse in units of 2^-32 turn, in the operation order the header states */
int ft8gpu_gfsk_pulse(int sps, uint32_t *out) {
    if (!out || !gfsk_sps_ok(sps)) return -1;
    const double c = M_PI * sqrt(2.0 / log(2.0));
    double sum = 0.0;
    for (int k = 0; k <= 3 * sps; k++) {
        out[k] = (uint32_t)((unsigned long long)llrint((4294967296.0 * sum) / (double)sps) & 0xFFFFFFFFull);
        const double t = ((double)k - 1.5 * (double)sps) / (double)sps;
        const double p = 0.5 * (erf((2.0 * c) * (t + 0.5)) - erf((2.0 * c) * (t - 0.5)));
        sum = sum + p;
    }
    return 0;
}

/* r[k] = 0.5 (1 - cos(pi k / nr)), k = 0 .. nr - 1, nr = sps / 8 */
int ft8gpu_gfsk_ramp(int sps, float *out) {
    if (!out || !gfsk_sps_ok(sps)) return -1;
    const int nr = sps / 8;
    for (int k = 0; k < nr; k++) out[k] = (float)(0.5 * (1.0 - cos(M_PI * (double)k / (double)nr)));
    return 0;
}

/* gc[i] = (cos, sin)(2 pi i / 4096), gf[i] = (cos, sin)(2 pi i / 2^24), each the float of the double value */
void ft8gpu_gfsk_twiddles(float *coarse, float *fine) {
    for (int i = 0; i < FT8GPU_GFSK_TWIDDLES; i++) {
        if (coarse) {
            const double a = 2.0 * M_PI * (double)i / 4096.0;
            coarse[2 * i] = (float)cos(a);
            coarse[2 * i + 1] = (float)sin(a);
        }
        if (fine) {
            const double a = 2.0 * M_PI * (double)i / 16777216.0;
            fine[2 * i] = (float)cos(a);
            fine[2 * i + 1] = (float)sin(a);
        }
    }
}

/* ---- the .wav writer: the 44-byte canonical header ft8gpu_read_wav (ft8_compat.c) reads back ---------------------------------- */
static void put_le32(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }
static void put_le16(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); }

int ft8gpu_write_wav(const char *path, const int16_t *pcm, int32_t nsamples) {
    if (!path || nsamples < 0 || (!pcm && nsamples > 0)) {
        fprintf(stderr, "ft8gpu: ft8gpu_write_wav: NULL argument or negative count\n");
        return -1;
    }
    FILE *f = fopen(path, "wb");
    if (!f) {
        fprintf(stderr, "ft8gpu: cannot open %s (%s)\n", path, strerror(errno));
        return -1;
    }
    const uint32_t bytes = 2u * (uint32_t)nsamples;
    unsigned char head[44];
    memcpy(head, "RIFF", 4);
    put_le32(head + 4, 36u + bytes);
    memcpy(head + 8, "WAVEfmt ", 8);
    put_le32(head + 16, 16);                                /* the fmt chunk's length */
    put_le16(head + 20, 1);                                 /* PCM */
    put_le16(head + 22, 1);                                 /* mono */
    put_le32(head + 24, FT8GPU_AUDIO_RATE);
    put_le32(head + 28, 2u * FT8GPU_AUDIO_RATE);            /* bytes per second */
    put_le16(head + 32, 2);                                 /* bytes per sample frame */
    put_le16(head + 34, 16);                                /* bits per sample */
    memcpy(head + 36, "data", 4);
    put_le32(head + 40, bytes);
    int ok = fwrite(head, 1, sizeof head, f) == sizeof head;
    /* samples go out little-endian whatever the host's order */
    unsigned char block[4096];
    for (int32_t done = 0; ok && done < nsamples;) {
        int32_t n = nsamples - done;
        if (n > (int32_t)(sizeof block / 2)) n = (int32_t)(sizeof block / 2);
        for (int32_t i = 0; i < n; i++) put_le16(block + 2 * i, (uint16_t)pcm[done + i]);
        ok = fwrite(block, 2, (size_t)n, f) == (size_t)n;
        done += n;
    }
    if (fclose(f) != 0) ok = 0;
    if (!ok) {
        fprintf(stderr, "ft8gpu: %s: write error\n", path);
        return -1;
    }
    return 0;
}
