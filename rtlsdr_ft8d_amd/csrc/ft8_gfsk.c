/* ft8_gfsk.c -- host tables of the GFSK synthesiser (include/ft8gpu.h "GFSK synthesis"), the fading channel's taps and its rule
 * on the host ("Fading channel"), and the .wav writer.  Plain C, no GPU. */
#include "../../include/ft8gpu.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
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

/* ---- the fading channel (include/ft8gpu.h "Fading channel"): taps, the refusals, and the whole rule for one clip on the host ---- */
static const double kQuantiles[FT8GPU_CHANNEL_TAPS] = FT8GPU_CHANNEL_QUANTILES;

static uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

int ft8gpu_channel_taps(uint64_t seed, uint64_t clip, uint32_t signal, uint32_t path, float spread_hz, uint32_t *gstep, uint32_t *theta) {
    if (!(spread_hz >= 0.0f && spread_hz <= 20.0f) || path > 1) return -1;
    const uint64_t key = mix64(seed ^ 0x4641444531ull);
    for (int m = 0; m < FT8GPU_CHANNEL_TAPS; m++) {
        if (gstep) {
            const double f = ((double)spread_hz / 2.0) * kQuantiles[m];
            gstep[m] = (uint32_t)(int64_t)llrint(f / 100.0 * 4294967296.0);
        }
        if (theta) theta[m] = (uint32_t)(mix64(key ^ mix64((clip << 12) + ((uint64_t)signal << 5) + ((uint64_t)path << 4) + (uint64_t)m)) >> 32);
    }
    return 0;
}

int ft8gpu_channel_check(const ft8gpu_channel *ch) {
    if (!ch || ch->mode > FT8GPU_CHANNEL_FADED) return 4;
    if (ch->mode == FT8GPU_CHANNEL_NONE) return 0;
    if (!(ch->spread_hz >= 0.0f && ch->spread_hz <= 20.0f)) return 1;      /* a NaN fails every comparison */
    if (!(ch->delay_ms >= 0.0f && ch->delay_ms <= 10.0f)) return 2;
    if (!(ch->path2_gain >= 0.0f && ch->path2_gain <= 4.0f)) return 3;
    return 0;
}

typedef struct { float c, s; } pair_t;

/* the grid values of one path, G[0 .. 1264] */
static void channel_grid(const uint32_t *gstep, const uint32_t *theta, float w, const pair_t *gc, const pair_t *gf, pair_t *G) {
    for (uint32_t j = 0; j < FT8GPU_CHANNEL_GRID; j++) {
        float sc = 0.0f, ss = 0.0f;
        for (int m = 0; m < FT8GPU_CHANNEL_TAPS; m++) {
            const uint32_t ph = theta[m] + gstep[m] * j;
            const pair_t c = gc[ph >> 20], f = gf[(ph >> 8) & 4095u];
            const float co = c.c * f.c - c.s * f.s, si = c.s * f.c + c.c * f.s;
            sc = sc + co;
            ss = ss + si;
        }
        G[j].c = w * (0.25f * sc);
        G[j].s = w * (0.25f * ss);
    }
}

int ft8gpu_channel_clip(int mode, const ft8gpu_synth_signal *signals, const ft8gpu_channel *channels, int nsig, int nsamples,
                        uint64_t seed, uint64_t clip, float *out) {
    if ((mode != FT8GPU_GFSK_IQ && mode != FT8GPU_GFSK_AUDIO) || !out || nsig < 0 || nsig > FT8GPU_GFSK_MAX_SIGNALS || (nsig > 0 && !signals)) return -1;
    const int iq = mode == FT8GPU_GFSK_IQ;
    if (!iq && (nsamples < 1 || nsamples > FT8GPU_AUDIO_NSAMPLES)) return -1;
    const int rate = iq ? 3200 : FT8GPU_AUDIO_RATE, sps = iq ? FT8GPU_GFSK_SPS_IQ : FT8GPU_GFSK_SPS_AUDIO;
    const int S = iq ? FT8GPU_CHANNEL_STEP_IQ : FT8GPU_CHANNEL_STEP_AUDIO, len = iq ? 48000 : nsamples, span = FT8GPU_NN * sps, nr = sps / 8;
    for (int s = 0; s < nsig; s++) {
        const ft8gpu_synth_signal *sg = &signals[s];
        if (!isfinite(sg->f0_hz) || !isfinite(sg->t0_s) || !isfinite(sg->amplitude) || fabsf(sg->f0_hz) >= (float)rate ||
            (!iq && sg->f0_hz < 0.0f) || fabsf(sg->t0_s) > 60.0f) return -1;
        for (int j = 0; j < FT8GPU_NN; j++) if (sg->tones[j] > 7) return -1;
        if (channels && ft8gpu_channel_check(&channels[s])) return -1;
    }
    uint32_t *Q = malloc((size_t)(3 * sps + 1) * sizeof *Q);
    float *ramp = malloc((size_t)nr * sizeof *ramp);
    pair_t *gc = malloc(FT8GPU_GFSK_TWIDDLES * sizeof *gc), *gf = malloc(FT8GPU_GFSK_TWIDDLES * sizeof *gf);
    pair_t *x = malloc((size_t)span * sizeof *x), *G = malloc(FT8GPU_CHANNEL_GRID * sizeof *G);
    int rc = Q && ramp && gc && gf && x && G ? 0 : -1;
    if (!rc) {
        ft8gpu_gfsk_pulse(sps, Q);
        ft8gpu_gfsk_ramp(sps, ramp);
        ft8gpu_gfsk_twiddles(&gc[0].c, &gf[0].c);
        float *re = out, *im = iq ? out + 48000 : NULL;
        for (int i = 0; i < len; i++) {
            re[i] = 0.0f;
            if (im) im[i] = 0.0f;
        }
        for (int s = 0; s < nsig; s++) {
            const ft8gpu_synth_signal *sg = &signals[s];
            const uint32_t step = (uint32_t)(unsigned long long)llrint((double)sg->f0_hz * 4294967296.0 / (double)rate);
            const int start = (int)lrintf(sg->t0_s * (float)rate);
            uint8_t e[FT8GPU_NN + 2];
            memcpy(e + 1, sg->tones, FT8GPU_NN);
            e[0] = e[1];
            e[FT8GPU_NN + 1] = e[FT8GPU_NN];
            for (int n = 0; n < span; n++) {                                /* the unfaded contribution (xr, xi) */
                const int m = n / sps, k = n - m * sps;
                const uint32_t phi = step * (uint32_t)n + (uint32_t)e[m] * Q[k + 2 * sps] + (uint32_t)e[m + 1] * Q[k + sps] + (uint32_t)e[m + 2] * Q[k];
                const pair_t c = gc[phi >> 20], f = gf[(phi >> 8) & 4095u];
                const float env = n < nr ? ramp[n] : (n >= span - nr ? ramp[span - 1 - n] : 1.0f);
                const float a = sg->amplitude * env;
                x[n].c = a * (c.c * f.c - c.s * f.s);
                x[n].s = a * (c.s * f.c + c.c * f.s);
            }
            if (!channels || channels[s].mode == FT8GPU_CHANNEL_NONE) {
                for (int n = 0; n < span; n++) {
                    const int i = start + n;
                    if (i < 0 || i >= len) continue;
                    re[i] = re[i] + x[n].c;
                    if (im) im[i] = im[i] + x[n].s;
                }
                continue;
            }
            const ft8gpu_channel *ch = &channels[s];
            const float g2 = ch->path2_gain, r = sqrtf(1.0f + g2 * g2);
            const float w[2] = { 1.0f / r, g2 / r };
            const int d = (int)lrintf(ch->delay_ms * (float)rate / 1000.0f);
            for (uint32_t p = 0; p < (g2 == 0.0f ? 1u : 2u); p++) {
                uint32_t gstep[FT8GPU_CHANNEL_TAPS], theta[FT8GPU_CHANNEL_TAPS];
                ft8gpu_channel_taps(seed, clip, (uint32_t)s, p, ch->spread_hz, gstep, theta);
                channel_grid(gstep, theta, w[p], gc, gf, G);
                for (int n = 0; n < span; n++) {
                    const int i = start + (p ? d : 0) + n;
                    if (i < 0 || i >= len) continue;
                    const int j = n / S, k = n - j * S;
                    const float t = (float)k / (float)S;
                    const float Gr = G[j].c + (G[j + 1].c - G[j].c) * t, Gi = G[j].s + (G[j + 1].s - G[j].s) * t;
                    re[i] = re[i] + (x[n].c * Gr - x[n].s * Gi);
                    if (im) im[i] = im[i] + (x[n].c * Gi + x[n].s * Gr);
                }
            }
        }
    }
    free(Q); free(ramp); free(gc); free(gf); free(x); free(G);
    return rc;
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
