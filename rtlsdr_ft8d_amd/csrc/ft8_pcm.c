/* ft8_pcm.c -- host side of the PCM front end that needs no GPU (include/ft8gpu.h "PCM front end"): the two mixer tables and the
 * taps of both stages, in the operation order the header states, and the .wav reader of its captures.  Plain C. */
#include "../../include/ft8gpu.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

/* the decimation of a rate the front end takes, 0 for any other */
int ft8gpu_pcm_decimation(int rate) {
    static const int kD[] = { 15, 30, 60, 120, 240 };
    for (int i = 0; i < 5; i++)
        if (rate == 3200 * kD[i]) return kD[i];
    return 0;
}

static int pcm_known_d(int D) { return D > 0 && ft8gpu_pcm_decimation(3200 * D) == D; }

/* w1[i] = (cos, -sin)(2 pi i / (16 D)), each the float of the double value */
void ft8gpu_pcm_mixer1(int D, float *out) {
    if (!out || !pcm_known_d(D)) return;
    const int n = 16 * D;
    for (int i = 0; i < n; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)n;
        out[2 * i] = (float)cos(a);
        out[2 * i + 1] = (float)-sin(a);
    }
}

/* w2[i] = (cos, -sin)(2 pi i / 1536) */
void ft8gpu_pcm_mixer2(float out[2 * FT8GPU_PCM_MIX2]) {
    if (!out) return;
    for (int i = 0; i < FT8GPU_PCM_MIX2; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)FT8GPU_PCM_MIX2;
        out[2 * i] = (float)cos(a);
        out[2 * i + 1] = (float)-sin(a);
    }
}

static double pcm_i0(double x) {
    double s = 1.0, term = 1.0;
    for (int k = 1; k < 40; k++) {
        const double q = x / (2.0 * (double)k);
        term = term * (q * q);
        s = s + term;
    }
    return s;
}

/* h[k] = (float)(t[k] / s), t[k] = (sinc((2 cutoff * d) / rate) * I0(9 sqrt(1 - (d / half)^2))) / I0(9), d = k - half,
 * k = 0 .. 2 half; s = the sum of t, k ascending from 0 */
static void pcm_kaiser_lowpass(int half, double cutoff, double rate, float *out) {
    double t[8 * 80 + 1], s = 0.0;
    const int n = 2 * half + 1;
    for (int k = 0; k < n; k++) {
        const double d = (double)(k - half);
        const double pu = M_PI * (((2.0 * cutoff) * d) / rate);
        const double sinc = d == 0.0 ? 1.0 : sin(pu) / pu;
        const double w = d / (double)half;
        const double x = 9.0 * sqrt(1.0 - w * w);
        t[k] = (sinc * pcm_i0(x)) / pcm_i0(9.0);
    }
    for (int k = 0; k < n; k++) s = s + t[k];
    for (int k = 0; k < n; k++) out[k] = (float)(t[k] / s);
}

/* stage A: 8 M + 1 taps centred on 4 M, M = D / 3, cutoff 4000 Hz at 3200 D sps; returns the number of taps, -1 for an unknown D */
int ft8gpu_pcm_taps_a(int D, float *out) {
    if (!out || !pcm_known_d(D)) return -1;
    const int M = D / 3;
    pcm_kaiser_lowpass(4 * M, 4000.0, 3200.0 * (double)D, out);
    return 8 * M + 1;
}

/* stage B: 47 taps centred on 23, cutoff 1600 Hz at 9600 sps, and h[47] = 0 */
void ft8gpu_pcm_taps_b(float out[FT8GPU_PCM_TAPS_B]) {
    if (!out) return;
    pcm_kaiser_lowpass(23, 1600.0, 9600.0, out);
    out[47] = 0.0f;
}

/* ---- .wav reader: RIFF/WAVE, PCM 16 bit or IEEE float 32 bit (plain or extensible), one or two channels, one of the five rates.
 * The file is walked chunk by chunk against its real length, as ft8gpu_read_wav walks it. */
static uint32_t le32(const unsigned char *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }
static uint32_t le16(const unsigned char *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8; }

static int wav_refuse(FILE *f, const char *path, const char *what) {
    fprintf(stderr, "ft8gpu: %s: %s\n", path, what);
    if (f) fclose(f);
    return -1;
}

int ft8gpu_read_wav_pcm(const char *path, void *out, size_t cap_bytes, int *format, int *rate, int32_t *nsamples) {
    if (nsamples) *nsamples = 0;
    if (format) *format = -1;
    if (rate) *rate = 0;
    if (!path || !out || !format || !rate || !nsamples) { fprintf(stderr, "ft8gpu: ft8gpu_read_wav_pcm: NULL argument\n"); return -1; }
    FILE *f = fopen(path, "rb");
    if (!f) return wav_refuse(NULL, path, "cannot be opened");
    char what[200];
    long size = -1;
    if (fseek(f, 0, SEEK_END) == 0) size = ftell(f);
    if (size < 0 || fseek(f, 0, SEEK_SET) != 0) return wav_refuse(f, path, "cannot determine the file's length");
    if (size == 0) return wav_refuse(f, path, "empty file");
    unsigned char head[40];
    if (size < 12 || fread(head, 1, 12, f) != 12) {
        snprintf(what, sizeof what, "truncated header: %ld bytes, a RIFF/WAVE header takes 12", size);
        return wav_refuse(f, path, what);
    }
    if (memcmp(head, "RIFF", 4) != 0 || memcmp(head + 8, "WAVE", 4) != 0) {
        snprintf(what, sizeof what, "not a RIFF/WAVE file: it starts with bytes %02x %02x %02x %02x, form type %02x %02x %02x %02x",
                 head[0], head[1], head[2], head[3], head[8], head[9], head[10], head[11]);
        return wav_refuse(f, path, what);
    }
    long at = 12;                                           /* offset of the next chunk header */
    int have_fmt = 0, fmt = 0, got_rate = 0;
    size_t frame_bytes = 0;                                 /* bytes of one sample (both components of a complex one) */
    for (;;) {
        if (at + 8 > size) {
            if (at >= size) return wav_refuse(f, path, have_fmt ? "no data chunk" : "no fmt and no data chunk");
            snprintf(what, sizeof what, "truncated header: %ld stray bytes where a chunk header takes 8", size - at);
            return wav_refuse(f, path, what);
        }
        if (fseek(f, at, SEEK_SET) != 0 || fread(head, 1, 8, f) != 8) return wav_refuse(f, path, "read error in a chunk header");
        const uint32_t len = le32(head + 4);
        const long body = at + 8, left = size - body;
        if (memcmp(head, "data", 4) == 0) {
            if (!have_fmt) return wav_refuse(f, path, "data chunk in front of the fmt chunk");
            if ((long long)len > (long long)left) {
                snprintf(what, sizeof what, "data chunk declares %u bytes, the file holds %ld behind its header", (unsigned)len, left);
                return wav_refuse(f, path, what);
            }
            size_t n = (size_t)len / frame_bytes;
            if (n > cap_bytes / frame_bytes) n = cap_bytes / frame_bytes;
            const size_t most = (size_t)FT8GPU_PCM_MAX_SAMPLES_PER_D * (size_t)(got_rate / 3200);       /* 15 s */
            if (n > most) n = most;
            if (n && fread(out, frame_bytes, n, f) != n) return wav_refuse(f, path, "read error in the data chunk");
            *nsamples = (int32_t)n;
            *format = fmt;
            *rate = got_rate;
            fclose(f);
            return 0;
        }
        if ((long long)len > (long long)left) {
            char id[5] = { 0 };
            for (int i = 0; i < 4; i++) id[i] = head[i] >= 0x20 && head[i] < 0x7f ? (char)head[i] : '?';
            snprintf(what, sizeof what, "truncated header: chunk '%s' declares %u bytes, the file holds %ld behind its header",
                     id, (unsigned)len, left);
            return wav_refuse(f, path, what);
        }
        if (memcmp(head, "fmt ", 4) == 0) {
            const uint32_t take = len < 40 ? len : 40;
            if (len < 16 || fread(head, 1, take, f) != take) {
                snprintf(what, sizeof what, "truncated header: fmt chunk of %u bytes, PCM takes 16", (unsigned)len);
                return wav_refuse(f, path, what);
            }
            uint32_t tag = le16(head);
            const uint32_t channels = le16(head + 2), hz = le32(head + 4), bits = le16(head + 14);
            if (tag == 0xFFFE) {                            /* extensible: the sub-format's first two bytes are the tag */
                if (len < 40) {
                    snprintf(what, sizeof what, "truncated header: extensible fmt chunk of %u bytes, it takes 40", (unsigned)len);
                    return wav_refuse(f, path, what);
                }
                tag = le16(head + 24);
            }
            const int d = hz <= 768000u ? ft8gpu_pcm_decimation((int)hz) : 0;
            if (!((tag == 1 && bits == 16) || (tag == 3 && bits == 32)) || channels < 1 || channels > 2 || d == 0) {
                snprintf(what, sizeof what,
                         "format tag %u, %u channel(s), %u Hz, %u bit: only PCM (tag 1) at 16 bit or IEEE float (tag 3) at 32 bit, "
                         "one or two channels, 48000, 96000, 192000, 384000 or 768000 Hz is read",
                         (unsigned)tag, (unsigned)channels, (unsigned)hz, (unsigned)bits);
                return wav_refuse(f, path, what);
            }
            fmt = (tag == 3 ? FT8GPU_PCM_F32 : 0) | (channels == 2 ? FT8GPU_PCM_COMPLEX : 0);
            frame_bytes = (size_t)(bits / 8) * channels;
            got_rate = (int)hz;
            have_fmt = 1;
        }
        at = body + (long)len + (long)(len & 1u);           /* chunks are padded to an even size */
    }
}
