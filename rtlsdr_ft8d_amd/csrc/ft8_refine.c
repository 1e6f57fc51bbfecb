/* ft8_refine.c -- host side of the refined time and frequency (include/ft8gpu.h "refined time and frequency"): seconds, hertz
 * and decibels from the powers the refine stage writes, and the message table with them.  Plain C, no GPU. */
#include "../../include/ft8gpu.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

/* vertex of the parabola through (-1, a), (0, b), (1, c), clamped to half a step; 0 where the three points have no maximum */
static double vertex(double a, double b, double c) {
    if (!isfinite(a) || !isfinite(b) || !isfinite(c)) return 0.0;
    const double den = a - 2.0 * b + c;
    if (!(den < 0.0)) return 0.0;
    const double v = 0.5 * (a - c) / den;
    return v < -0.5 ? -0.5 : (v > 0.5 ? 0.5 : v);
}

int ft8gpu_refined_estimate(const ft8gpu_message *msg, const ft8gpu_refined *r, float *dt_s, float *freq_hz, float *snr_db) {
    if (!msg || !r || !dt_s || !freq_hz || !snr_db || !r->valid) return -1;
    const int T = 2 * msg->cand.time_offset + msg->cand.time_sub;
    const int F = 2 * msg->cand.freq_offset + msg->cand.freq_sub;
    const int e = r->e_best;
    const double vt = (e - 1 < -FT8GPU_REFINE_RANGE || e + 1 > FT8GPU_REFINE_RANGE) ? 0.0 : vertex(r->pt[0], r->pt[1], r->pt[2]);
    *dt_s = (float)((256.0 * T + FT8GPU_REFINE_LEAD + FT8GPU_REFINE_STEP * (e + vt)) / 3200.0);
    int us = 1;
    for (int u = 2; u <= 3; ++u)
        if (r->pf[u] > r->pf[us]) us = u;
    *freq_hz = (float)(3.125 * (F + (us - 2) + vertex(r->pf[us - 1], r->pf[us], r->pf[us + 1])));
    const double noise = r->noise, sig = r->pf[2];
    double snr;
    if (!(noise > 0.0) || !isfinite(noise)) {
        snr = sig > 0.0 ? 49.0 : -30.0;
    } else {
        double s = sig - noise;
        if (!(s > FLT_MIN)) s = FLT_MIN;
        snr = 10.0 * log10(s / noise * 6.25 / 2500.0);
        if (!(snr > -30.0)) snr = -30.0;
        if (snr > 49.0) snr = 49.0;
    }
    *snr_db = (float)snr;
    return 0;
}

int ft8gpu_format_messages_refined(const ft8gpu_message *msgs, const ft8gpu_refined *refined, int32_t n, char *out, size_t cap) {
    char line[96];
    size_t at = 0;
    if (out && cap) out[0] = 0;
    if (n > 0 && (!msgs || !refined)) return -1;
    for (int32_t i = 0; i < n && i < FT8GPU_K_MAX_MESSAGES; i++) {
        float dt = msgs[i].dt_s, freq = msgs[i].freq_hz, snr = (float)msgs[i].snr_db;
        (void)ft8gpu_refined_estimate(&msgs[i], &refined[i], &dt, &freq, &snr);
        int len = snprintf(line, sizeof line, "%3d %5.2f %6.1f ~  %.25s\n", (int)lrintf(snr), (double)dt, (double)freq, msgs[i].text);
        if (len < 0) continue;
        if ((size_t)len >= sizeof line) len = (int)sizeof line - 1;           /* a record that is no decode may hold any float */
        if (out && at < cap) {
            const size_t room = cap - at - 1, k = (size_t)len < room ? (size_t)len : room;
            memcpy(out + at, line, k);
            out[at + k] = 0;
        }
        at += (size_t)len;
    }
    return (int)at;
}
