/* ft8_subtract.c -- host tables of the subtraction in the I/Q samples (include/ft8gpu.h "subtraction in the I/Q samples").
 * Plain C, no GPU. */
#include "../../include/ft8gpu.h"

#include <math.h>

/* w4[i] = (cos, -sin)(2 pi i / 4096), each the float of the double value, as build_tables forms the waterfall's table */
void ft8gpu_subtract_twiddles(float *out) {
    if (!out) return;
    for (int i = 0; i < FT8GPU_SUBTRACT_TABLE; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)FT8GPU_SUBTRACT_TABLE;
        out[2 * i] = (float)cos(a);
        out[2 * i + 1] = (float)(-sin(a));
    }
}

/* ---- tables of the audio front end (include/ft8gpu.h "12 kHz audio") ---------------------------------------------------------- */
/* wm[i] = (cos, -sin)(2 pi i / 1920), formed as w4 above */
void ft8gpu_audio_mixer(float out[2 * FT8GPU_AUDIO_MIX]) {
    if (!out) return;
    for (int i = 0; i < FT8GPU_AUDIO_MIX; i++) {
        const double a = 2.0 * M_PI * (double)i / (double)FT8GPU_AUDIO_MIX;
        out[2 * i] = (float)cos(a);
        out[2 * i + 1] = (float)(-sin(a));
    }
}

/* I0(x) = 1 + sum over k = 1 .. 39 of T_k, T_k = T_(k-1) * (x / (2 k))^2 */
static double audio_i0(double x) {
    double s = 1.0, term = 1.0;
    for (int k = 1; k <= 39; k++) {
        const double q = x / (2.0 * (double)k);
        term = term * (q * q);
        s = s + term;
    }
    return s;
}

/* the Kaiser low-pass of the rule, in the operation order the header states */
void ft8gpu_audio_taps(float out[FT8GPU_AUDIO_TAPS]) {
    if (!out) return;
    const double i0_8 = audio_i0(8.0);
    for (int k = 0; k < FT8GPU_AUDIO_TAPS - 1; k++) {
        const double d = (double)(k - 79);
        const double pu = M_PI * ((3200.0 * d) / 48000.0);
        const double sinc = k == 79 ? 1.0 : sin(pu) / pu;
        const double w = d / 80.0;
        const double x = 8.0 * sqrt(1.0 - w * w);
        out[k] = (float)((((8.0 * (3200.0 / 48000.0)) * sinc) * audio_i0(x)) / i0_8);
    }
    out[FT8GPU_AUDIO_TAPS - 1] = 0.0f;
}

/* inv[n] = (float)(1.0 / (32 n)), n = 1 .. 2 * FT8GPU_SUBTRACT_SMOOTH + 1; inv[0] = 0 (not part of the ABI) */
__attribute__((visibility("hidden"))) void ft8_subtract_inv_table(float *inv) {
    inv[0] = 0.0f;
    for (int n = 1; n <= 2 * FT8GPU_SUBTRACT_SMOOTH + 1; n++) inv[n] = (float)(1.0 / (32.0 * (double)n));
}
