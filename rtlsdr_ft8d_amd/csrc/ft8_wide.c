/* ft8_wide.c -- host tables of the wideband RX front end (include/ft8gpu.h "wideband RX"): the two mixer tables and the taps of
 * the second stage, in the operation order the header states.  Plain C, no GPU. */
#include "../../include/ft8gpu.h"

#include <math.h>

/* w1[i] = (lrint(32767 cos), -lrint(32767 sin))(2 pi i / 6000) */
void ft8gpu_wide_mixer1(int16_t out[2 * FT8GPU_WIDE_MIX1]) {
    if (!out) return;
    for (int i = 0; i < FT8GPU_WIDE_MIX1; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)FT8GPU_WIDE_MIX1;
        out[2 * i] = (int16_t)lrint(32767.0 * cos(a));
        out[2 * i + 1] = (int16_t)-lrint(32767.0 * sin(a));
    }
}

/* w2[i] = (cos, -sin)(2 pi i / 3072), each the float of the double value */
void ft8gpu_wide_mixer2(float out[2 * FT8GPU_WIDE_MIX2]) {
    if (!out) return;
    for (int i = 0; i < FT8GPU_WIDE_MIX2; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)FT8GPU_WIDE_MIX2;
        out[2 * i] = (float)cos(a);
        out[2 * i + 1] = (float)-sin(a);
    }
}

static double wide_i0(double x) {
    double s = 1.0, term = 1.0;
    for (int k = 1; k < 40; k++) {
        const double q = x / (2.0 * (double)k);
        term = term * (q * q);
        s = s + term;
    }
    return s;
}

enum { kKaiser = 93, kWideTaps = 95 };

/* t[k] = sinc(d / 6) * kaiser(93, beta 9)[k], d = k - 46; 0 outside 0 .. 92 */
static double wide_kaiser_sinc(int k) {
    if (k < 0 || k >= kKaiser) return 0.0;
    const double d = (double)(k - (kKaiser - 1) / 2);
    const double pu = M_PI * ((3200.0 * d) / 19200.0);
    const double sinc = d == 0.0 ? 1.0 : sin(pu) / pu;
    const double w = d / (double)((kKaiser - 1) / 2);
    const double x = 9.0 * sqrt(1.0 - w * w);
    return (sinc * wide_i0(x)) / wide_i0(9.0);
}

/* h = t * [-a, 1 + 2 a, -a], a = 0.1685, normalised to sum 1: 95 taps centred on 47, and h[95] = 0 */
void ft8gpu_wide_taps(float out[FT8GPU_WIDE_TAPS]) {
    if (!out) return;
    const double a = 0.1685;
    double hh[kWideTaps], s = 0.0;
    for (int i = 0; i < kWideTaps; i++)
        hh[i] = ((1.0 + 2.0 * a) * wide_kaiser_sinc(i - 1) - a * wide_kaiser_sinc(i)) - a * wide_kaiser_sinc(i - 2);
    for (int i = 0; i < kWideTaps; i++) s = s + hh[i];
    for (int i = 0; i < kWideTaps; i++) out[i] = (float)(hh[i] / s);
    for (int i = kWideTaps; i < FT8GPU_WIDE_TAPS; i++) out[i] = 0.0f;
}
